// Ordered top-k for 64 < k <= RAGRAPH_TOPK_ORDERED_MAX: torch.topk(S, k, sorted=True) over a materialised score matrix,
// canonical order (score descending, index ascending).  The reference's k comes from the data: retrieve_num = num_class + 1
// (RAGraph_node/ragraph_utils/ToyGraphBase.py:22), doubled with noise (:63-64); a constructor argument in the few-shot
// flavour (RAGraph_node_fewshot/ragraph_utils/ToyGraphBase.py:16,22,64).
//
// One workgroup per (chunk, row); a row of fewer than 65536 elements is one chunk.  Every element is a 32-bit key
// (topk_order.h order_key: larger float -> larger unsigned, -0 == +0, NaN dropped) and a 32-bit index, packed as the u64
// (~key << 32) | index, whose ascending order IS the canonical order.
//   1. histogram pass: an LDS histogram of the top 11 key bits; a block scan finds the bin that holds the k-th key.
//      If the keys above that bin plus its members do not fit the LDS buffer (cap >= 2k), the bin is refined by a pass
//      over the next 11 bits, then the last 10 (heavy ties, quantised or constant rows).  A chunk that fits the buffer
//      whole skips this pass.
//   2. compaction pass: every key above the bin and every member of it go to the LDS buffer (slots by wave-aggregated LDS
//      atomics: the buffer is sorted next, so the slot order does not matter).  When the bin is one exact key value and
//      still too large, only the `need` lowest-index members are taken: each wave walks a contiguous quarter of the
//      chunk in index order and ranks its ties after a count pass over the earlier quarters.
//   3. bitonic sort of the buffer in LDS; the first k are written.
// A chunked row writes k packed candidates per chunk to the workspace; the candidate rows (G * k per row) go through the
// same kernel until one chunk is left.  Deterministic: no global atomics, the result is a sorted set of unique u64.
#include "common.h"
#include "topk_large.h"
#include "topk_order.h"

namespace ragraph {

constexpr int64_t LARGE_CHUNKED_ROW = 65536;  // rows of at least this many elements are cut into chunks
constexpr int LARGE_MAX_CAP = 8192;           // LDS buffer entries for k = 4096: 64 KiB
constexpr int LARGE_LDS_EXTRA = 64;           // scalars behind the buffer
constexpr unsigned long long LARGE_NONE = ~0ull;

struct LargeArgs {
  const void* src;  // float [B, ld] or packed u64 [B, ld]
  int64_t n, ld, chunk;
  int k, cap;
  unsigned idx_off;
  unsigned long long* cand_out;  // out_i == nullptr: row b, chunk g -> cand_out + b * cand_ld + g * k
  int64_t cand_ld;
  float* out_s;
  int64_t* out_i;
  const float* score_src;
  int64_t score_ld, idx_base;
};

// The 4 elements [p, p + 4) of a row (clipped at `end`) as (key, index); bit r of the result: element r exists and is a
// candidate (not NaN / not a sentinel).
template <bool CAND>
__device__ __forceinline__ unsigned large_load4(const void* row, int64_t p, int64_t end, bool vec, unsigned idx_off,
                                                unsigned key[4], unsigned idx[4]) {
  unsigned valid = 0;
  if constexpr (CAND) {
    const unsigned long long* r = static_cast<const unsigned long long*>(row);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long c = (p + j < end) ? r[p + j] : LARGE_NONE;
      key[j] = ~(unsigned)(c >> 32);
      idx[j] = (unsigned)c;
      valid |= (c != LARGE_NONE) ? (1u << j) : 0u;
    }
  } else {
    const float* r = static_cast<const float*>(row);
    float f[4];
    if (vec && p + 4 <= end) {
      const float4 v = *reinterpret_cast<const float4*>(r + p);
      f[0] = v.x;
      f[1] = v.y;
      f[2] = v.z;
      f[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = (p + j < end) ? r[p + j] : __builtin_nanf("");
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      key[j] = order_key(f[j]);
      idx[j] = idx_off + (unsigned)(p + j);
      valid |= (f[j] == f[j]) ? (1u << j) : 0u;
    }
  }
  return valid;
}

// Wave w walks [e0 + w * seg, ...) of the chunk in index order, 4 x 256 elements in flight per step; lane l owns elements
// 4l .. 4l + 3 of every 256.  f(key, idx, valid) is called by the whole wave, the 4 groups in index order.
template <bool CAND, typename F>
__device__ __forceinline__ void large_walk(const void* row, int64_t e0, int64_t e1, bool vec, unsigned idx_off, int wave,
                                           int lane, F&& f) {
  const int64_t seg = (e1 - e0 + 15) / 16 * 4;
  const int64_t s0 = e0 + wave * seg;
  const int64_t s1 = s0 + seg < e1 ? s0 + seg : e1;
  for (int64_t base = s0; base < s1; base += 1024) {
    unsigned key[4][4], idx[4][4], valid[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) valid[u] = large_load4<CAND>(row, base + 256 * u + 4 * lane, s1, vec, idx_off, key[u], idx[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) f(key[u], idx[u], valid[u]);
  }
}

// Exclusive prefix over the lanes (and the wave total) of a per-lane count c in 0..4.
__device__ __forceinline__ unsigned wave_prefix4(unsigned c, int lane, unsigned& total) {
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long b0 = __ballot(c & 1u), b1 = __ballot(c & 2u), b2 = __ballot(c & 4u);
  total = (unsigned)(__popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2));
  return (unsigned)(__popcll(b0 & below) + 2 * __popcll(b1 & below) + 4 * __popcll(b2 & below));
}

// The bin of hist[nb] (counted from the top) that holds the need-th key.  first: need = min(k, total keys), stored in
// sc[4].  Results in sc: [5] bin, [6] keys in higher bins, [7] keys in the bin, [8] total.
__device__ __forceinline__ void large_pick(const unsigned* hist, int nb, bool first, unsigned need_in, unsigned* sc, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int per = nb / 256;
  const int top = nb - per * tid - 1;  // this thread's bins: top, top - 1, ..., top - per + 1
  unsigned s = 0;
  for (int j = 0; j < per; ++j) s += hist[top - j];
  unsigned x = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned v = __shfl_up(x, off);
    if (lane >= off) x += v;
  }
  if (lane == 63) sc[wave] = x;
  __syncthreads();
  unsigned excl = x - s, total = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) excl += sc[w];
    total += sc[w];
  }
  const unsigned need = first ? (need_in < total ? need_in : total) : need_in;
  if (tid == 0) {
    sc[4] = need;
    sc[8] = total;
  }
  if (need >= 1 && excl < need && excl + s >= need) {  // exactly one thread
    unsigned acc = excl;
    for (int j = 0; j < per; ++j) {
      const unsigned h = hist[top - j];
      if (acc + h >= need) {
        sc[5] = (unsigned)(top - j);
        sc[6] = acc;
        sc[7] = h;
        break;
      }
      acc += h;
    }
  }
  __syncthreads();
}

template <bool CAND>
__global__ void __launch_bounds__(256) topk_large_kernel(LargeArgs a) {
  extern __shared__ unsigned long long large_lds[];
  unsigned long long* buf = large_lds;                       // [cap] candidates
  unsigned* hist = reinterpret_cast<unsigned*>(large_lds);  // [<= 2048] during the histogram passes (aliases buf)
  unsigned* sc = reinterpret_cast<unsigned*>(large_lds + a.cap);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.y, g = blockIdx.x;
  const int64_t e0 = g * a.chunk;
  const int64_t e1 = e0 + a.chunk < a.n ? e0 + a.chunk : a.n;
  const char* rowc = static_cast<const char*>(a.src) + b * a.ld * (CAND ? 8 : 4);
  const void* row = rowc;
  const bool vec = !CAND && ((reinterpret_cast<uintptr_t>(rowc + e0 * 4) & 15u) == 0);
  const unsigned k = (unsigned)a.k, cap = (unsigned)a.cap;

  unsigned lo = 0u, hi = 0xFFFFFFFFu, need = 0u, kk = 0u;
  bool exact = false;
  const bool whole = e1 - e0 <= (int64_t)cap;  // every candidate fits: no histogram
  if (!whole) {
    unsigned prefix = 0u, mask = 0u;
    for (int pass = 0; pass < 3; ++pass) {
      const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
      const int nb = pass == 2 ? 1024 : 2048;
      for (int i = tid; i < nb; i += 256) hist[i] = 0u;
      __syncthreads();
      large_walk<CAND>(row, e0, e1, vec, a.idx_off, wave, lane, [&](const unsigned* key, const unsigned*, unsigned valid) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (((valid >> j) & 1u) && (key[j] & mask) == prefix) atomicAdd(&hist[(key[j] >> shift) & (unsigned)(nb - 1)], 1u);
      });
      __syncthreads();
      large_pick(hist, nb, pass == 0, pass == 0 ? k : need, sc, tid);
      if (pass == 0) {
        kk = sc[4];
        need = kk;
        if (kk == 0u) break;  // every element is NaN: padding only
      }
      const unsigned d = sc[5], acc = sc[6], inbin = sc[7];
      __syncthreads();  // (sc and hist are rewritten by the next pass)
      need -= acc;
      prefix |= d << shift;
      mask |= (unsigned)(nb - 1) << shift;
      if ((kk - need) + inbin <= cap) break;
      if (pass == 2) exact = true;  // one key value, more members than the buffer: the lowest `need` indices
    }
    lo = prefix;
    hi = prefix | ~mask;
  }

  // ---- compaction
  unsigned tie_base = 0u;
  if (tid == 0) sc[9] = 0u;
  if (!whole && kk == 0u) {
    // nothing to select
  } else {
    if (exact) {  // ties before this wave's quarter, in index order
      unsigned t = 0u;
      large_walk<CAND>(row, e0, e1, vec, a.idx_off, wave, lane, [&](const unsigned* key, const unsigned*, unsigned valid) {
#pragma unroll
        for (int j = 0; j < 4; ++j) t += ((valid >> j) & 1u) && key[j] == lo;
      });
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off);
      if (lane == 0) sc[10 + wave] = t;
      __syncthreads();
      for (int w = 0; w < wave; ++w) tie_base += sc[10 + w];
    }
    __syncthreads();
    large_walk<CAND>(row, e0, e1, vec, a.idx_off, wave, lane, [&](const unsigned* key, const unsigned* idx, unsigned valid) {
      unsigned sel = 0u, tie = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool v = (valid >> j) & 1u;
        sel |= (v && key[j] > hi) ? (1u << j) : 0u;
        tie |= (v && key[j] >= lo && key[j] <= hi) ? (1u << j) : 0u;
      }
      if (exact) {
        unsigned ttot;
        unsigned rank = tie_base + wave_prefix4((unsigned)__popc(tie), lane, ttot);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((tie >> j) & 1u) {
            if (rank < need) sel |= 1u << j;
            ++rank;
          }
        tie_base += ttot;
      } else {
        sel |= tie;
      }
      if (__any(sel != 0u)) {
        unsigned tot;
        const unsigned pre = wave_prefix4((unsigned)__popc(sel), lane, tot);
        unsigned base = 0u;
        if (lane == 0) base = atomicAdd(&sc[9], tot);
        unsigned pos = __shfl(base, 0) + pre;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((sel >> j) & 1u) {
            if (pos < cap) buf[pos] = ((unsigned long long)(~key[j]) << 32) | idx[j];
            ++pos;
          }
      }
    });
  }
  __syncthreads();
  unsigned count = sc[9];
  if (count > cap) count = cap;  // (cannot happen: the passes bound it)
  if (whole) kk = count < k ? count : k;

  // ---- bitonic sort of buf[0, n2), padded with sentinels
  unsigned n2 = 1u;
  while (n2 < count) n2 <<= 1;
  for (unsigned i = count + tid; i < n2; i += 256) buf[i] = LARGE_NONE;
  __syncthreads();
  for (unsigned size = 2; size <= n2; size <<= 1) {
    for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
      for (unsigned t = tid; t < n2 / 2; t += 256) {
        const unsigned i = 2 * t - (t & (stride - 1)), j = i + stride;
        const unsigned long long x = buf[i], y = buf[j];
        if ((x > y) == ((i & size) == 0)) {
          buf[i] = y;
          buf[j] = x;
        }
      }
      __syncthreads();
    }
  }

  // ---- the first k
  for (unsigned r = tid; r < k; r += 256) {
    const unsigned long long c = r < kk ? buf[r] : LARGE_NONE;
    if (a.out_i) {
      float s = RG_NEG_INF;
      int64_t i = INT64_MAX;
      if (c != LARGE_NONE) {
        const unsigned ix = (unsigned)c;
        s = a.score_src ? a.score_src[b * a.score_ld + ix] : order_unkey(~(unsigned)(c >> 32));
        i = (int64_t)ix + a.idx_base;
      }
      a.out_s[b * k + r] = s;
      a.out_i[b * k + r] = i;
    } else {
      a.cand_out[b * a.cand_ld + g * k + r] = c;
    }
  }
}

static int large_cap(int64_t k) {
  int c = 2048;
  while (c < 2 * k) c <<= 1;
  return c;
}
static int64_t large_chunk(int64_t n, int64_t k) {
  if (n < LARGE_CHUNKED_ROW) return n;
  int64_t c = 16384;  // a chunk yields k candidates: >= 16x shrink per level
  while (c < 16 * k && c < LARGE_CHUNKED_ROW) c <<= 1;
  return c;
}

// Sizes of the two ping-pong candidate buffers of the chunk levels (level l writes buffer l & 1; levels shrink).
static void large_level_bytes(int64_t B, int64_t n, int64_t k, size_t bytes[2]) {
  bytes[0] = bytes[1] = 0;
  for (int lvl = 0;; ++lvl) {
    const int64_t G = cdiv(n, large_chunk(n, k));
    if (G == 1) break;
    const size_t sz = align_up((size_t)B * G * k * sizeof(unsigned long long), 256);
    if (sz > bytes[lvl & 1]) bytes[lvl & 1] = sz;
    n = G * k;
  }
}

size_t large_select_ws_bytes(int64_t B, int64_t n, int64_t k) {
  size_t bytes[2];
  large_level_bytes(B, n, k, bytes);
  return bytes[0] + bytes[1];
}

template <bool CAND>
static int launch_large(const LargeArgs& a, int64_t B, int64_t G, hipStream_t st) {
  static DeviceOnce once;
  if (hipError_t e = raise_dynamic_lds(once, &topk_large_kernel<CAND>, LARGE_MAX_CAP * 8 + LARGE_LDS_EXTRA); e != hipSuccess) {
    set_error("topk_rows_large: cannot raise the LDS limit: %s", hipGetErrorString(e));
    return RAGRAPH_EDEVICE;
  }
  const size_t lds = (size_t)a.cap * 8 + LARGE_LDS_EXTRA;
  for (int64_t b0 = 0; b0 < B; b0 += 65535) {  // grid.y <= 65535
    const int64_t nb = B - b0 < 65535 ? B - b0 : 65535;
    LargeArgs ab = a;
    ab.src = static_cast<const char*>(a.src) + b0 * a.ld * (CAND ? 8 : 4);
    if (a.out_i) {
      ab.out_s = a.out_s + b0 * a.k;
      ab.out_i = a.out_i + b0 * a.k;
      if (a.score_src) ab.score_src = a.score_src + b0 * a.score_ld;
    } else {
      ab.cand_out = a.cand_out + b0 * a.cand_ld;
    }
    hipLaunchKernelGGL(topk_large_kernel<CAND>, dim3((unsigned)G, (unsigned)nb), dim3(256), lds, st, ab);
    RG_CHECK_LAUNCH("topk_rows_large");
  }
  return RAGRAPH_OK;
}

int large_select(const float* S, const unsigned long long* C, int64_t B, int64_t n, int64_t ld, int64_t k,
                 unsigned idx_off, const float* score_src, int64_t score_ld, int64_t idx_base, unsigned long long* cand_out,
                 int64_t cand_ld, float* out_s, int64_t* out_i, void* ws, hipStream_t st) {
  size_t bytes[2];
  large_level_bytes(B, n, k, bytes);
  unsigned long long* pp[2] = {static_cast<unsigned long long*>(ws),
                               reinterpret_cast<unsigned long long*>(static_cast<char*>(ws) + bytes[0])};
  LargeArgs a;
  a.k = (int)k;
  a.cap = large_cap(k);
  a.score_src = score_src;
  a.score_ld = score_ld;
  a.idx_base = idx_base;
  const void* src = C ? static_cast<const void*>(C) : static_cast<const void*>(S);
  bool cand = C != nullptr;
  for (int lvl = 0;; ++lvl) {
    a.src = src;
    a.n = n;
    a.ld = ld;
    a.chunk = large_chunk(n, k);
    a.idx_off = cand ? 0u : idx_off;
    const int64_t G = cdiv(n, a.chunk);
    if (G == 1) {
      a.cand_out = cand_out;
      a.cand_ld = cand_ld;
      a.out_s = out_s;
      a.out_i = out_i;
      return cand ? launch_large<true>(a, B, 1, st) : launch_large<false>(a, B, 1, st);
    }
    a.cand_out = pp[lvl & 1];
    a.cand_ld = G * k;
    a.out_s = nullptr;
    a.out_i = nullptr;
    const int rc = cand ? launch_large<true>(a, B, G, st) : launch_large<false>(a, B, G, st);
    if (rc != RAGRAPH_OK) return rc;
    src = pp[lvl & 1];
    cand = true;
    n = G * k;
    ld = G * k;
  }
}

}  // namespace ragraph

using namespace ragraph;

extern "C" size_t ragraph_topk_rows_large_workspace_bytes(int64_t B, int64_t N, int64_t k) {
  if (B < 1 || N < 1 || k < 1 || k > N || k > RAGRAPH_TOPK_ORDERED_MAX) return 0;
  return large_select_ws_bytes(B, N, k);
}

extern "C" int ragraph_topk_rows_large_f32(const float* S, int64_t B, int64_t N, int64_t ld, int64_t k, float* out_scores,
                                           int64_t* out_idx, void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(S && out_scores && out_idx, RAGRAPH_EINVAL, "topk_rows_large: null pointer");
  RG_REQUIRE(B >= 0 && N >= 1 && ld >= N, RAGRAPH_EINVAL, "topk_rows_large: bad shape");
  RG_REQUIRE(k >= 1 && k <= N, RAGRAPH_EINVAL, "topk_rows_large: k=%lld out of range for N=%lld", (long long)k, (long long)N);
  RG_REQUIRE(k <= RAGRAPH_TOPK_ORDERED_MAX, RAGRAPH_EUNSUPPORTED, "topk_rows_large: k=%lld > %d (RAGRAPH_TOPK_ORDERED_MAX)",
             (long long)k, RAGRAPH_TOPK_ORDERED_MAX);
  RG_REQUIRE(N < (int64_t)INT_MAX, RAGRAPH_EUNSUPPORTED, "topk_rows_large: N must fit int32");
  if (B == 0) return RAGRAPH_OK;
  const size_t need = large_select_ws_bytes(B, N, k);
  RG_REQUIRE(need == 0 || (ws && ws_bytes >= need), RAGRAPH_EWORKSPACE, "topk_rows_large: workspace %zu < %zu", ws_bytes, need);
  return large_select(S, nullptr, B, N, ld, k, 0u, S, ld, 0, nullptr, 0, out_scores, out_idx, ws, as_stream(stream));
}
