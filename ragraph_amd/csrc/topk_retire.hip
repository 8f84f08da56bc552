// Retired rows behind a live index (ragraph_topk_drop_rows_f32, ragraph_rows_retire_u32).
//
// A bank that shrinks keeps its physical rows -- and with them every copy, duplicate group and learnt bound of
// ragraph_amd/kernels_index.py -- and marks the rows taken out in a bitmap (bit r & 31 of word r >> 5).  A search then asks
// for k + r keys, r the number of retired rows, and this kernel drops the retired entries from the finished canonical lists:
// the canonical top-(k + r) of all rows is the first k + r rows of ONE total order (score descending, index ascending), at
// most r of them are retired, so the first k live entries of the list are the first k live rows of that order -- the bits
// of a search over the live rows alone (a row's score does not depend on which other rows exist).  DESIGN.md section 4.21.
//
// One wave per list, four lists per workgroup.  The list is taken in chunks of 64 entries, one lane per entry: the lane
// tests its row's bit, the wave ballots, a live entry's place is the running count plus the ballot's bits below the lane,
// and it is stored when that place is below k_out.  The wave leaves the loop once k_out entries are out: with r retired rows
// among a million a list of k + r entries is read as far as its first k live ones, one chunk for every k + r <= 64.  Scores
// are copied, never recomputed.  Plain vector loads and stores, no LDS, no workspace.
#include "common.h"

namespace ragraph {

constexpr int DROP_WAVES = 4;

struct DropParams {
  const float* scores = nullptr;    // [B, k_in]
  const int64_t* idx = nullptr;
  int64_t B = 0;
  int k_in = 0, k_out = 0;
  int64_t idx_base = 0;
  const uint32_t* bitmap = nullptr; // cdiv(n_rows, 32) words
  int64_t n_rows = 0;
  float* out_s = nullptr;           // [B, k_out]
  int64_t* out_i = nullptr;
  int* short_lists = nullptr;
};

__global__ void __launch_bounds__(DROP_WAVES * 64) topk_drop_rows_kernel(DropParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t list = (int64_t)blockIdx.x * DROP_WAVES + wave;
  if (list >= p.B) return;   // (wave-uniform)
  const float* s = p.scores + list * p.k_in;
  const int64_t* ix = p.idx + list * p.k_in;
  float* os = p.out_s + list * p.k_out;
  int64_t* oi = p.out_i + list * p.k_out;
  const unsigned long long below = (1ull << lane) - 1ull;
  int out = 0;   // live entries found so far (wave-uniform)
  for (int c0 = 0; c0 < p.k_in && out < p.k_out; c0 += 64) {
    const int e = c0 + lane;
    float sc = RG_NEG_INF;
    int64_t id = INT64_MAX;
    bool live = false;
    if (e < p.k_in) {
      sc = s[e];
      id = ix[e];
      // (unsigned: a padding entry's INT64_MAX, or any index below idx_base, lands beyond n_rows and is dropped unread)
      const uint64_t r = (uint64_t)id - (uint64_t)p.idx_base;
      if (r < (uint64_t)p.n_rows) live = ((p.bitmap[r >> 5] >> (r & 31)) & 1u) == 0;
    }
    const unsigned long long alive = __ballot(live);
    const int pos = out + __popcll(alive & below);
    if (live && pos < p.k_out) {
      os[pos] = sc;
      oi[pos] = id;
    }
    out += __popcll(alive);
  }
  if (out < p.k_out) {   // a short list: padded as a shard's list is, and counted
    for (int e = out + lane; e < p.k_out; e += 64) {
      os[e] = RG_NEG_INF;
      oi[e] = INT64_MAX;
    }
    if (lane == 0) __hip_atomic_fetch_add(p.short_lists, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(256) rows_retire_kernel(const int64_t* rows, int64_t m, int64_t n_rows, uint32_t* bitmap) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m) return;
  const uint64_t r = (uint64_t)rows[t];
  if (r < (uint64_t)n_rows) atomicOr(bitmap + (r >> 5), 1u << (r & 31));
}

}  // namespace ragraph

using namespace ragraph;

extern "C" int ragraph_topk_drop_rows_f32(const float* scores, const int64_t* idx, int64_t B, int k_in, int64_t idx_base,
                                          const uint32_t* bitmap, int64_t n_rows, int k_out, float* out_scores,
                                          int64_t* out_idx, int* short_lists, void* stream) {
  RG_REQUIRE(scores && idx && bitmap && out_scores && out_idx && short_lists, RAGRAPH_EINVAL, "topk_drop_rows: null pointer");
  RG_REQUIRE(B >= 1 && B < ((int64_t)1 << 31), RAGRAPH_EINVAL, "topk_drop_rows: B=%lld out of range", (long long)B);
  RG_REQUIRE(k_in >= 1 && k_in <= RAGRAPH_TOPK_ORDERED_MAX, RAGRAPH_EINVAL,
             "topk_drop_rows: k_in=%d outside 1..%d (RAGRAPH_TOPK_ORDERED_MAX)", k_in, RAGRAPH_TOPK_ORDERED_MAX);
  RG_REQUIRE(k_out >= 1 && k_out <= k_in, RAGRAPH_EINVAL, "topk_drop_rows: k_out=%d outside 1..k_in=%d", k_out, k_in);
  RG_REQUIRE(n_rows >= 1, RAGRAPH_EINVAL, "topk_drop_rows: n_rows=%lld is not positive", (long long)n_rows);
  RG_REQUIRE(idx_base >= 0, RAGRAPH_EINVAL, "topk_drop_rows: idx_base=%lld is negative", (long long)idx_base);
  RG_REQUIRE((const void*)out_scores != (const void*)scores && (const void*)out_idx != (const void*)idx, RAGRAPH_EINVAL,
             "topk_drop_rows: out must not alias the lists");
  DropParams p;
  p.scores = scores;
  p.idx = idx;
  p.B = B;
  p.k_in = k_in;
  p.k_out = k_out;
  p.idx_base = idx_base;
  p.bitmap = bitmap;
  p.n_rows = n_rows;
  p.out_s = out_scores;
  p.out_i = out_idx;
  p.short_lists = short_lists;
  hipLaunchKernelGGL(topk_drop_rows_kernel, dim3((unsigned)cdiv(B, DROP_WAVES)), dim3(DROP_WAVES * 64), 0, as_stream(stream), p);
  RG_CHECK_LAUNCH("topk_drop_rows");
  return RAGRAPH_OK;
}

extern "C" int ragraph_rows_retire_u32(const int64_t* rows, int64_t m, int64_t n_rows, uint32_t* bitmap, void* stream) {
  RG_REQUIRE(bitmap && (rows || m == 0), RAGRAPH_EINVAL, "rows_retire: null pointer");
  RG_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), RAGRAPH_EINVAL, "rows_retire: m=%lld out of range", (long long)m);
  RG_REQUIRE(n_rows >= 1, RAGRAPH_EINVAL, "rows_retire: n_rows=%lld is not positive", (long long)n_rows);
  if (m == 0) return RAGRAPH_OK;
  hipLaunchKernelGGL(rows_retire_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, as_stream(stream), rows, m, n_rows, bitmap);
  RG_CHECK_LAUNCH("rows_retire");
  return RAGRAPH_OK;
}
