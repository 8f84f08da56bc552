// Exact top-k CONTINUED over rows appended to a bank (ragraph_topk_cosine_tail_f32).
//
// The reference's bank only grows (RAGraph_node/ragraph_utils/ToyGraphBase.py:116-119, finetune-rag.py:97) and its search is
// torch.topk over all rows (SimilarityFunctions.py:6-16 + ToyGraphBase.py:66-67).  Here the rows a bank had when its copies,
// groups and learnt bounds were made keep all of that (the SEALED part, ragraph_amd/kernels_index.py); the rows appended since
// (the TAIL, a few dozen to a few thousand) are searched by this kernel, which starts from the sealed search's finished
// canonical list (the SEED) and returns the canonical top-k of both -- the bits of one search over all rows.
//
// One launch.  The inner loop is the small-batch streaming kernel's (topk_cosine.hip: topk_smallb_kernel): 16 queries are the
// B operand of v_mfma_f32_16x16x4_f32, normalised in the kernel by the row-norm tree (the bits of ragraph_normalize_rows_f32),
// every wave streams its own 16 KiB key tiles through a wave-private LDS transpose image, a score is the natural-order fmaf
// chain from +0, and a key is offered to the wave's sorted k-list (LDS) only when it reaches max(the seed's k-th score, the
// list's k-th).  The seed's k-th score bounds the final k-th from below from the first key on -- what thr_init is to that
// kernel after its pre-pass -- so on a tail that holds nothing better no list is ever touched.
//   * grid = (groups of 16 queries) x S slices of the tail; workgroup = 4 waves (k = 64 lists: 4 x 8 KiB next to 4 x 16 KiB).
//   * S = 1 (short tails, or enough query groups to fill the chip): the workgroup merges its four wave lists WITH the seed and
//     writes the result.  Nothing else runs.
//   * S > 1 (a long tail under few queries: the stream needs more than one workgroup's loads in flight): a workgroup leaves
//     its sorted list per query in the workspace (agent-scope stores, no L2 write-back: see topk_small.hip) and takes a ticket
//     of its query group; the last to arrive merges the S lists with the seed.  The tickets are cleared by a memset node
//     in front of the launch (the workspace carries no state between calls).
//   * every merge is a merge of SORTED lists: the workgroup's (four wave lists, the seed) by rank -- an entry's place in the
//     result is its place in its own list plus, per other list, the prefix a binary search finds --, the last arriver's (up to 32
//     slices, the seed) by the lists' heads.  A seed entry travels as the int r - k < 0 (r its position): below every tail key's
//     local number, as its index is below idx_base_tail, and ascending with r as the seed's canonical order; the lane that
//     places it turns it back into an int64 index.  No list leaves LDS except the S > 1 partials.
#include "common.h"
#include "topk_order.h"

namespace ragraph {

template <int D>
struct TailCfg {
  static constexpr int WAVES = 4;
  static constexpr int THREADS = WAVES * 64;
  static constexpr int SUB = 256 / D;              // 16-key MFMA sub-tiles per 16 KiB tile
  static constexpr int TILE_KEYS = 16 * SUB;
  static constexpr int ROW = D + 2;                // floats: conflict-free ds_read_b32 of the MFMA k-slots
  static constexpr int TILE_FLOATS = TILE_KEYS * ROW;
  static constexpr int RPI = 256 / D;              // rows covered by one wave-wide float4 load instruction
  static int per_wave_floats(int k) { return TILE_FLOATS + 2 * k * 16; }
  static size_t lds_bytes(int k) { return (size_t)WAVES * sizeof(float) * per_wave_floats(k) + 16; }
};

constexpr int TAIL_MAX_SLICES = 32;   // (with the seed <= 64 lists, one head per lane; staged in ONE wave's 16 KiB + lists of LDS)

struct TailParams {
  const float* Q = nullptr;        // [B,D] raw queries
  const float* Kt = nullptr;       // [T,D] normalised tail rows
  int64_t B = 0;
  int T = 0, k = 0;
  int G = 0, S = 0;                // query groups of 16, slices of the tail
  int64_t base = 0;                // index of tail key 0
  const float* seed_s = nullptr;   // [B,k]
  const int64_t* seed_i = nullptr;
  float* out_s = nullptr;
  int64_t* out_i = nullptr;
  float* part_s = nullptr;         // S > 1: [G*16][S][k]
  int* part_i = nullptr;
  int* tickets = nullptr;          // S > 1: [G], zero at the launch
};

// Merge of nlists sorted lists of k entries by RANK: entry `pos` of list a has `pos` entries of its own list in front of it and, in
// every other list b, the prefix that a binary search finds (canonical order, with the list number as the last word so that
// identical empty entries (-inf, RG_IDX_NONE) of different lists still order one way).  Its rank is the sum, the ranks are a
// permutation, and the entries of rank < k are the merged list.  No cross-lane traffic and no dependent rounds: with the four
// wave lists and the seed at k = 10 a lane makes 16 LDS probes where a merge by heads took 10 rounds of 18 wave shuffles
// (measured: 4 queries per wave cost 20 us of a 40-row tail's call that way).
template <typename Get, typename Put>
__device__ __forceinline__ void merge_ranked(int nsets, int nlists, int k, int lane, Get get, Put put) {
  const int M = nlists * k;   // per set (a query): the lanes take (set, entry) pairs, so a wave merges its queries side by side
  for (int c = lane; c < nsets * M; c += 64) {
    const int set = c / M, e = c - set * M;
    const int a = e / k, pos = e - a * k;
    float es;
    int ei;
    get(set, a, pos, es, ei);
    int rank = pos;
    for (int b = 0; b < nlists; ++b) {
      if (b == a) continue;
      int lo = 0, hi = k;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        float bs;
        int bi;
        get(set, b, mid, bs, bi);
        // (the three-word cand_better, written out: calling it here changed the kernel's instructions)
        if (bs > es || (bs == es && (bi < ei || (bi == ei && b < a)))) lo = mid + 1;
        else hi = mid;
      }
      rank += lo;
    }
    if (rank < k) put(set, rank, es, ei);
  }
}

// Merge of nlists <= 64 sorted lists of k entries by their HEADS (the last merge over up to 32 slices and the seed, where a
// rank would cost a binary search per entry and list): lane g < nlists holds the head of list g, a round is one wave argmax
// -- canonical order, the holder's lane as the last word, so that every lane agrees on ONE winner even among identical empty
// entries --, the winner's lane advances.  Lane r < k returns round r's winner in (rs, ri).
template <typename Next>
__device__ __forceinline__ void merge_heads(int nlists, int k, int lane, Next next, float& rs, int& ri) {
  float hs = RG_NEG_INF;
  int hi = RG_IDX_NONE, hp = 0;
  if (lane < nlists) next(0, hs, hi);
  rs = RG_NEG_INF;
  ri = RG_IDX_NONE;
  for (int r = 0; r < k; ++r) {
    float ws = hs;
    int wi = hi, wl = lane;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float os = __shfl_xor(ws, off);
      const int oi = __shfl_xor(wi, off);
      const int ol = __shfl_xor(wl, off);
      if (cand_better(os, oi, ol, ws, wi, wl)) {
        ws = os;
        wi = oi;
        wl = ol;
      }
    }
    if (lane == r) {
      rs = ws;
      ri = wi;
    }
    if (lane == wl && lane < nlists) {
      ++hp;
      hs = RG_NEG_INF;
      hi = RG_IDX_NONE;
      if (hp < k) next(hp, hs, hi);
    }
  }
}

template <int D>
__global__ void __launch_bounds__(256) topk_tail_kernel(TailParams p) {
  using C = TailCfg<D>;
  extern __shared__ float4 smem4[];
  float* smem = reinterpret_cast<float*>(smem4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, sl = lane >> 4;
  const int k = p.k;
  const int per_wave = C::TILE_FLOATS + 2 * k * 16;  // tile | ls[k][16] | li[k][16]  (one sorted list per query)
  float* tile = smem + wave * per_wave;
  float* ls = tile + C::TILE_FLOATS;
  int* li = reinterpret_cast<int*>(ls + k * 16);
  int* misc = reinterpret_cast<int*>(smem + C::WAVES * per_wave);

  const int G = p.G, S = p.S;
  const int grp = blockIdx.x % G, slice = blockIdx.x / G;
  const int64_t qbase = (int64_t)grp * 16;
  const int nq = (int)min((int64_t)16, p.B - qbase);  // queries of this group

  // B operand: query j, k-slots sl, sl + 4, ...; normalised here by the tree of normalize_rows_kernel (bit-identical), as the
  // small-batch kernel of ragraph_topk_cosine_f32 does.  Queries >= B are clamped; their lists are never offered to.
  float breg[D / 4];
  {
    // (a row is at most 64 float4 chunks: lane l holds chunk l or nothing.  All 16 rows are requested before the first is
    // reduced -- one trip to memory, not sixteen: at 40 tail rows this prologue is most of the kernel)
    float my_d = 1.f;
    float4 v16[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int64_t row = qbase + (jj < nq ? jj : nq - 1);
      v16[jj] = lane < D / 4 ? reinterpret_cast<const float4*>(p.Q + row * D)[lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      float pp = 0.f;
      pp = fmaf(v16[jj].x, v16[jj].x, pp);
      pp = fmaf(v16[jj].y, v16[jj].y, pp);
      pp = fmaf(v16[jj].z, v16[jj].z, pp);
      pp = fmaf(v16[jj].w, v16[jj].w, pp);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) pp = __fadd_rn(pp, __shfl_xor(pp, off));
      const float d = fmaxf(sqrtf(pp), 1e-12f);
      if (jj == (j < nq ? j : nq - 1)) my_d = d;
    }
    const int64_t q = (qbase + j < p.B) ? qbase + j : p.B - 1;
    const float4* qp = reinterpret_cast<const float4*>(p.Q + q * D);
#pragma unroll
    for (int m = 0; m < D / 4; ++m) {
      const float4 v = qp[m];
      const float x = sl == 0 ? v.x : sl == 1 ? v.y : sl == 2 ? v.z : v.w;
      breg[m] = x / my_d;
    }
  }
  for (int i = lane; i < k * 16; i += 64) {
    ls[i] = RG_NEG_INF;
    li[i] = RG_IDX_NONE;
  }

  const int T = p.T;
  const int ntiles = (T + C::TILE_KEYS - 1) / C::TILE_KEYS;
  const int gw = slice * C::WAVES + wave, nw = S * C::WAVES;
  const bool live = j < nq;
  // the seed's k-th score: a key that only ties it has the higher index and never displaces the seed's entry, and a key below
  // it cannot be selected at all (-inf where the seed is padded: every key is offered)
  const float thr_floor = live ? p.seed_s[(qbase + j) * k + k - 1] : RG_NEG_INF;
  float thr = live ? thr_floor : __builtin_huge_valf();

  float4 pre[16];
  const int lrow = lane / (D / 4), lcol = 4 * (lane % (D / 4));
  auto load_tile = [&](int t) {
    const int key0 = t * C::TILE_KEYS + lrow;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      int r = key0 + i * C::RPI;
      if (r > T - 1) r = T - 1;   // (rows past the tail: a clamped reload, never offered)
      pre[i] = *reinterpret_cast<const float4*>(p.Kt + (int64_t)r * D + lcol);
    }
  };

  int t = gw;
  if (t < ntiles) load_tile(t);
  for (; t < ntiles; t += nw) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float* d = tile + (lrow + i * C::RPI) * C::ROW + lcol;
      *reinterpret_cast<float2*>(d) = make_float2(pre[i].x, pre[i].y);
      *reinterpret_cast<float2*>(d + 2) = make_float2(pre[i].z, pre[i].w);
    }
    const int tn = t + nw;
    load_tile(tn < ntiles ? tn : t);  // next tile in flight under this tile's MFMAs
    __builtin_amdgcn_sched_barrier(0);

#pragma unroll 1
    for (int sub = 0; sub < C::SUB; ++sub) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* a = tile + (sub * 16 + j) * C::ROW + sl;
#pragma unroll
      for (int m = 0; m < D / 4; ++m) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * m], breg[m], acc, 0, 0, 0);

      const float mx = fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3]));
      if (__any(mx >= thr)) {   // (NaN compares false: never offered)
        const int key_base = t * C::TILE_KEYS + sub * 16 + 4 * sl;
        unsigned mask = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (acc[r] >= thr && key_base + r < T) mask |= 1u << r;
#define RG_TAIL_PRUNE() \
  _Pragma("unroll") for (int r = 0; r < 4; ++r) if ((mask >> r & 1u) && acc[r] < thr) mask &= ~(1u << r)
        unsigned long long pend = __ballot(mask != 0);
        if (__popcll(pend) > 8) {
          // DENSE regime (a padded seed, or a tail full of winners): lane-private inserts, the 4 lanes of a query take turns
          while (pend) {
            const int r0 = __ffs(mask) - 1;
            const float my_sc = r0 == 1 ? acc[1] : r0 == 2 ? acc[2] : r0 == 3 ? acc[3] : acc[0];
#pragma unroll 1
            for (int ss = 0; ss < 4; ++ss) {
              if (mask != 0 && sl == ss) lds_insert_lane(ls + j, li + j, k, 16, my_sc, key_base + r0);
            }
            mask &= mask - 1;
            if (live) thr = fmaxf(thr_floor, ls[(k - 1) * 16 + j]);
            RG_TAIL_PRUNE();
            pend = __ballot(mask != 0);
          }
        }
        while (pend) {
          // the wave inserts the candidates one at a time, all 64 lanes cooperating on each insert
          const int src = __ffsll((long long)pend) - 1;          // wave-uniform: lowest lane with a candidate
          const int r0 = __ffs(mask) - 1;                        // (meaningful on lane src)
          const float my_sc = r0 == 1 ? acc[1] : r0 == 2 ? acc[2] : r0 == 3 ? acc[3] : acc[0];
          const float sc = __shfl(my_sc, src);
          const int idx = __shfl(key_base + r0, src);
          const int q = src & 15;
          const float nthr = lds_insert_coop(ls, li, q, k, 16, sc, idx, lane);
          if (live && j == q) thr = fmaxf(thr_floor, nthr);
          if (lane == src) mask &= mask - 1;
          RG_TAIL_PRUNE();
          pend = __ballot(mask != 0);
        }
#undef RG_TAIL_PRUNE
      }
    }
  }

  // ---- workgroup merge: the 4 wave lists of a query (+ the seed when this workgroup saw the whole tail) ----------------------
  __syncthreads();
  {
    // this wave's queries: wave, wave + 4, ... (set number qi <-> query wave + 4 qi), merged side by side.  The seeds' scores
    // wait in this wave's tile area, free now: the binary searches probe LDS, not memory.
    const int nsets = nq > wave ? (nq - wave + C::WAVES - 1) / C::WAVES : 0;
    float* seed_l = tile;
    if (S == 1)
      for (int c = lane; c < nsets * k; c += 64) seed_l[c] = p.seed_s[(qbase + wave + C::WAVES * (c / k)) * k + c % k];
    __builtin_amdgcn_wave_barrier();
    merge_ranked(nsets, C::WAVES + (S == 1 ? 1 : 0), k, lane, [&](int qi, int g, int pos, float& s, int& i) {
      if (g < C::WAVES) {
        const float* wl = smem + g * per_wave + C::TILE_FLOATS;
        const int q = wave + C::WAVES * qi;
        s = wl[pos * 16 + q];
        i = reinterpret_cast<const int*>(wl + k * 16)[pos * 16 + q];
      } else {
        s = seed_l[qi * k + pos];
        i = pos - k;
      }
    }, [&](int qi, int r, float rs, int ri) {
      const int64_t qg = qbase + wave + C::WAVES * qi;
      if (S == 1) {
        p.out_s[qg * k + r] = rs;
        p.out_i[qg * k + r] = ri < 0 ? p.seed_i[qg * k + ri + k] : ri == RG_IDX_NONE ? INT64_MAX : p.base + ri;
      } else {
        const int64_t o = (qg * S + slice) * k + r;
        __hip_atomic_store(p.part_s + o, rs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p.part_i + o, ri, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    });
  }
  if (S == 1) return;

  // ---- the group's LAST workgroup merges the S slices' lists with the seed (the ticket of topk_small.hip: agent-scope
  // stores acknowledged, then a relaxed read-modify-write; no __threadfence, which would write the L2 back) ------------------
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) misc[0] = __hip_atomic_fetch_add(p.tickets + grp, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == S - 1;
  __syncthreads();
  if (!misc[0]) return;
  for (int q = wave; q < nq; q += C::WAVES) {
    const int64_t row = (qbase + q) * k;
    // stage the S lists in this wave's region (the stream's buffers are free now): [S][k] scores | [S][k] numbers
    float* st_s = tile;
    int* st_i = reinterpret_cast<int*>(tile + S * k);
    for (int c = lane; c < S * k; c += 64) {
      const int64_t o = (qbase + q) * S * k + c;
      st_s[c] = __hip_atomic_load(p.part_s + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      st_i[c] = __hip_atomic_load(p.part_i + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    float* seed_l = tile + 2 * S * k;   // (may reach into this wave's own list area: merged and left behind above)
    if (lane < k) seed_l[lane] = p.seed_s[row + lane];
    __builtin_amdgcn_wave_barrier();
    float rs;
    int ri;
    merge_heads(S + 1, k, lane, [&](int pos, float& s, int& i) {
      if (lane < S) {
        s = st_s[lane * k + pos];
        i = st_i[lane * k + pos];
      } else {
        s = seed_l[pos];
        i = pos - k;
      }
    }, rs, ri);
    if (lane < k) {
      p.out_s[row + lane] = rs;
      p.out_i[row + lane] = ri < 0 ? p.seed_i[row + ri + k] : ri == RG_IDX_NONE ? INT64_MAX : p.base + ri;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

struct TailPlan {
  int G, S;
  size_t part_s_off, part_i_off, tickets_off, total;
};

// S slices: one workgroup (4 waves, 16 KiB in flight each) takes a tail of up to 32 tiles alone; beyond that every wave gets
// about 4 tiles, as far as 32 slices and about two workgroups per CU over all query groups go.
static TailPlan tail_plan(int64_t B, int64_t T, int D, int k) {
  TailPlan pl;
  pl.G = (int)cdiv(B, 16);
  const int64_t tiles = cdiv(T, 16 * (256 / D));
  int64_t S = 1;
  if (tiles > 32) {
    S = cdiv(tiles, 16);
    if (S > TAIL_MAX_SLICES) S = TAIL_MAX_SLICES;
    const int64_t room = 2 * (int64_t)device_cus_multiple_of_8() / pl.G;
    if (S > room) S = room;
    if (S < 1) S = 1;
  }
  pl.S = (int)S;
  const size_t lists = pl.S > 1 ? (size_t)pl.G * 16 * pl.S * k : 0;
  pl.part_s_off = 0;
  pl.part_i_off = align_up(lists * sizeof(float), 256);
  pl.tickets_off = pl.part_i_off + align_up(lists * sizeof(int), 256);
  pl.total = pl.tickets_off + align_up((pl.S > 1 ? (size_t)pl.G : 0) * sizeof(int), 256) + 256;
  return pl;
}

static bool tail_shape_ok(int64_t B, int64_t T, int D, int k) {
  return B >= 1 && B < ((int64_t)1 << 31) && T >= 1 && T <= RAGRAPH_TOPK_TAIL_MAX && (D == 64 || D == 128 || D == 256) &&
         k >= 1 && k <= RAGRAPH_TOPK_MAX;
}

template <int D>
static int launch_tail(const TailParams& p, hipStream_t st) {
  using C = TailCfg<D>;
  static DeviceOnce lds_once;  // per device (common.h)
  if (hipError_t e = raise_dynamic_lds(lds_once, &topk_tail_kernel<D>, 160 * 1024); e != hipSuccess) {
    set_error("topk_cosine_tail: cannot raise dynamic LDS limit: %s", hipGetErrorString(e));
    return RAGRAPH_EDEVICE;
  }
  hipLaunchKernelGGL((topk_tail_kernel<D>), dim3((unsigned)((int64_t)p.G * p.S)), dim3(C::THREADS), C::lds_bytes(p.k), st, p);
  RG_CHECK_LAUNCH("topk_cosine_tail");
  return RAGRAPH_OK;
}

}  // namespace ragraph

using namespace ragraph;

extern "C" size_t ragraph_topk_cosine_tail_workspace_bytes(int64_t B, int64_t T, int D, int k) {
  if (!tail_shape_ok(B, T, D, k)) return 0;
  return tail_plan(B, T, D, k).total;
}

extern "C" int ragraph_topk_cosine_tail_f32(const float* Q, int64_t B, const float* Kn_tail, int64_t T, int D, int k,
                                            int64_t idx_base_tail, const float* seed_scores, const int64_t* seed_idx,
                                            float* out_scores, int64_t* out_idx, void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(Q && Kn_tail && seed_scores && seed_idx && out_scores && out_idx && ws, RAGRAPH_EINVAL,
             "topk_cosine_tail: null pointer");
  RG_REQUIRE(B >= 1 && B < ((int64_t)1 << 31), RAGRAPH_EINVAL, "topk_cosine_tail: B=%lld out of range", (long long)B);
  RG_REQUIRE(T >= 1 && T <= RAGRAPH_TOPK_TAIL_MAX, RAGRAPH_EINVAL,
             "topk_cosine_tail: T=%lld outside 1..%d (RAGRAPH_TOPK_TAIL_MAX): fold the tail into the bank", (long long)T,
             RAGRAPH_TOPK_TAIL_MAX);
  RG_REQUIRE(k >= 1 && k <= RAGRAPH_TOPK_MAX, RAGRAPH_EINVAL, "topk_cosine_tail: k=%d outside 1..%d (RAGRAPH_TOPK_MAX)", k,
             RAGRAPH_TOPK_MAX);
  RG_REQUIRE(idx_base_tail >= 0, RAGRAPH_EINVAL, "topk_cosine_tail: idx_base_tail=%lld is negative", (long long)idx_base_tail);
  RG_REQUIRE(D == 64 || D == 128 || D == 256, RAGRAPH_EUNSUPPORTED,
             "topk_cosine_tail: D=%d (the fused widths are 64, 128, 256: pad the rows as ragraph_amd.KeyIndex does)", D);
  RG_REQUIRE(aligned16(Q) && aligned16(Kn_tail), RAGRAPH_EINVAL, "topk_cosine_tail: Q and Kn_tail must be 16-B aligned");
  RG_REQUIRE((const void*)out_scores != (const void*)seed_scores && (const void*)out_idx != (const void*)seed_idx,
             RAGRAPH_EINVAL, "topk_cosine_tail: out must not alias the seed");
  const TailPlan pl = tail_plan(B, T, D, k);
  RG_REQUIRE(ws_bytes >= pl.total, RAGRAPH_EWORKSPACE, "topk_cosine_tail: workspace %zu < %zu bytes", ws_bytes, pl.total);
  hipStream_t st = as_stream(stream);
  char* w = static_cast<char*>(ws);
  TailParams p;
  p.Q = Q;
  p.Kt = Kn_tail;
  p.B = B;
  p.T = (int)T;
  p.k = k;
  p.G = pl.G;
  p.S = pl.S;
  p.base = idx_base_tail;
  p.seed_s = seed_scores;
  p.seed_i = seed_idx;
  p.out_s = out_scores;
  p.out_i = out_idx;
  if (pl.S > 1) {
    p.part_s = reinterpret_cast<float*>(w + pl.part_s_off);
    p.part_i = reinterpret_cast<int*>(w + pl.part_i_off);
    p.tickets = reinterpret_cast<int*>(w + pl.tickets_off);
    if (hipError_t e = hipMemsetAsync(p.tickets, 0, (size_t)pl.G * sizeof(int), st); e != hipSuccess) {
      set_error("topk_cosine_tail: clearing the tickets failed: %s", hipGetErrorString(e));
      return RAGRAPH_EDEVICE;
    }
  }
  return D == 64 ? launch_tail<64>(p, st) : D == 128 ? launch_tail<128>(p, st) : launch_tail<256>(p, st);
}
