// The canonical top-k order, stated once: comparisons, order-preserving keys and LDS sorted-list inserts of every top-k kernel.
//
// THE ORDER.  Every result list is sorted by score descending, then index ascending; with unique indices that is a strict total
// order.  The EMPTY entry is (-inf, RG_IDX_NONE): it is behind every real entry (real indices are below INT_MAX), so lists are
// initialised with it and it fills the places behind the last real entry.  cand_better is the order's one definition; every
// key below is an integer image of it, so that a maximum, a radix digit or an atomicMax can stand for the comparison.
//
// TWO KEY MAPS, which differ in the zeros:
//   * order_key / order_unkey (unsigned): larger float -> larger key, and -0 and +0 are ONE key, because the order compares
//     them equal (a tie, broken by index).  The inverse returns +0 for both.  Whatever SELECTS or RANKS entries by key needs
//     this: the radix selects (rows.hip, topk_large.hip), the pair key below.  A map that told the zeros apart would put
//     every -0 behind every +0 whatever their indices.
//   * f2ord / ord2f (signed; small_f2u / small_u2f are the same map shifted to unsigned, nonzero for every non-NaN float):
//     larger float -> larger int, -0 BELOW +0, the inverse returns the exact bits.  One instruction cheaper.  Right wherever
//     only monotonicity is needed and the word is decoded back to a float before anything is compared with it: the group
//     maxima of the bound passes (atomicMax), the k-th-score statistics words.  A maximum over {-0, +0} decodes to +0, which
//     compares equal to both, so no bound moves.  Never rank entries of a result list with it.
//
// NaN.  cand_better never prefers a NaN and never prefers anything to one (both comparisons are false), so it is no order
// on NaN scores; the kernels' scores are finite by contract, and the large-k selection drops NaN elements before it makes
// keys.  The maps stay monotone in the BITS: a NaN with the sign bit clear lands above +inf, one with it set below -inf
// (small_f2u of the all-ones NaN is 0), and both inverses return a NaN's bits unchanged.
//
// THE PAIR KEY.  pair_key(score, id) = order_key(score) << 32 | ~id: its unsigned order is the canonical order (larger key =
// better).  id == RG_IDX_NONE marks the empty entry, which is key 0, below every real pair (order_key(-inf) > 0).  Kernels that
// compare keys as two 32-bit words (wave_select, the scored rescoring) build them from order_key and pair_lo.
//
// The first part is plain C++ (g++ -std=c++17, no HIP header: tools/check_topk_order.cpp walks every float through it); the
// inserts at the end are device code.
#pragma once
#include <limits.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RG_ORDER_FN __host__ __device__ __forceinline__
#else
#define RG_ORDER_FN inline
#endif

#define RG_IDX_NONE INT_MAX

namespace ragraph {

RG_ORDER_FN bool cand_better(float s1, int i1, float s2, int i2) { return (s1 > s2) || (s1 == s2 && i1 < i2); }
// With a third word (a list or lane number) behind the index: identical entries of different lists -- the empty ones -- still
// order one way, so that ranks are a permutation and every lane agrees on one winner.
RG_ORDER_FN bool cand_better(float s1, int i1, int l1, float s2, int i2, int l2) {
  return (s1 > s2) || (s1 == s2 && (i1 < i2 || (i1 == i2 && l1 < l2)));
}

RG_ORDER_FN unsigned order_key(float f) {
  unsigned b = __builtin_bit_cast(unsigned, f);
  if (b == 0x80000000u) b = 0u;  // -0 == +0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
RG_ORDER_FN float order_unkey(unsigned key) {
  return __builtin_bit_cast(float, (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

RG_ORDER_FN int f2ord(float f) {
  const int b = __builtin_bit_cast(int, f);
  return b >= 0 ? b : b ^ 0x7FFFFFFF;
}
RG_ORDER_FN float ord2f(int o) { return __builtin_bit_cast(float, o >= 0 ? o : o ^ 0x7FFFFFFF); }
RG_ORDER_FN unsigned small_f2u(float f) { return (unsigned)f2ord(f) ^ 0x80000000u; }
RG_ORDER_FN float small_u2f(unsigned u) { return ord2f((int)(u ^ 0x80000000u)); }

// (the key's low word; its high word is order_key(score).  pair_key_real: the caller knows the pair is no empty entry, or
// discards the key of one)
RG_ORDER_FN unsigned pair_lo(int id) { return ~(unsigned)id; }
RG_ORDER_FN unsigned long long pair_key_real(float s, int id) { return ((unsigned long long)order_key(s) << 32) | pair_lo(id); }
RG_ORDER_FN unsigned long long pair_key(float s, int id) { return id == RG_IDX_NONE ? 0ull : pair_key_real(s, id); }
RG_ORDER_FN float pair_score(unsigned long long key) { return order_unkey((unsigned)(key >> 32)); }
RG_ORDER_FN int pair_id(unsigned lo) { return (int)~lo; }   // (of the low word)

#if defined(__HIPCC__)
// ---- sorted k-lists (k <= 64), lane p of a wave = entry p --------------------------------------------------------------------
// Wave-cooperative insert into a list that lives in LDS as [k][stride], column q: one ballot finds the position (the entries
// that stay ahead of the candidate are a prefix), one shuffle shifts the rest.  All 64 lanes must call it with wave-uniform
// (q, s, idx).  Returns the new k-th best score.
__device__ __forceinline__ float lds_insert_coop(float* ls, int* li, int q, int k, int stride, float s, int idx, int lane) {
  const bool mine = lane < k;
  float es = mine ? ls[lane * stride + q] : 0.f;
  int ei = mine ? li[lane * stride + q] : 0;
  const unsigned long long ahead = __ballot(mine && cand_better(es, ei, s, idx));
  const int pos = __popcll(ahead);
  const float us = __shfl_up(es, 1);
  const int ui = __shfl_up(ei, 1);
  if (pos < k) {  // wave-uniform
    if (lane == pos) {
      es = s;
      ei = idx;
    } else if (lane > pos) {
      es = us;
      ei = ui;
    }
    if (mine && lane >= pos) {
      ls[lane * stride + q] = es;
      li[lane * stride + q] = ei;
    }
  }
  return __shfl(es, k - 1);
}

// Lane-private insert into the list at ls / li (already offset to this lane's column): shift from the end.  For the DENSE
// regime (the first tiles of a stream, when most lanes hold candidates): the lanes' queries insert in parallel, where the
// cooperative insert would take the candidates one at a time.
__device__ __forceinline__ void lds_insert_lane(float* ls, int* li, int k, int stride, float s, int idx) {
  if (!cand_better(s, idx, ls[(k - 1) * stride], li[(k - 1) * stride])) return;
  int p = k - 1;
  while (p > 0) {
    const float ps = ls[(p - 1) * stride];
    const int pi = li[(p - 1) * stride];
    if (!cand_better(s, idx, ps, pi)) break;
    ls[p * stride] = ps;
    li[p * stride] = pi;
    --p;
  }
  ls[p * stride] = s;
  li[p * stride] = idx;
}
#endif  // __HIPCC__

}  // namespace ragraph
