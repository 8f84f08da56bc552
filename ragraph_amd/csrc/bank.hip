// Toy-bank construction on the device: the deterministic arithmetic of
//   InverseSampling.compute_sample_prob / pagerank_algorithm / degree_centrality_algorithm
//       RAGraph_node/ragraph_utils/InverseSampling.py:6-56 (dense); RAGraph_edge/modules/ragraph_utils/InverseSampling.py:6-62
//       (sparse, same recurrence with the dangling mass added explicitly)
//   PositionAwareEncoder.floyd_warshall / encode_position_aware_code   RAGraph_node/ragraph_utils/PositionAwareEncoder.py:6-48
// batched over resource graphs, with no host round trip inside: the reference runs them per 40-node graph in Python
// (a dense mat-vec and a host-side convergence test per power iteration; a Python double loop per position code).
//
// pagerank: the graphs of a batch are the segments [graph_ptr[g], graph_ptr[g+1]) of one block-diagonal CSR (a single
// big graph is one segment).  One power iteration = two launches: `step` (every node pulls its in-neighbours' mass: one
// fmaf chain in CSR order) and `check` (one workgroup per graph: L1 change in a fixed order, the reference's
// break-BEFORE-assign -- a converged graph keeps the previous iterate, as pagerank_algorithm returns it --, the
// dangling mass for the next step).  The host enqueues max_iter iterations back to back; converged graphs turn their
// launches into no-ops through a device flag, nothing is read back in between.
#include "common.h"
#include "rng.h"
#include "sortscan.h"

namespace ragraph {

constexpr int PR_THREADS = 256;

// deterministic block sum (fixed tree) of one value per thread
__device__ __forceinline__ float block_sum_256(float v, float* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = __fadd_rn(v, __shfl_xor(v, off));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  const float t = __fadd_rn(__fadd_rn(sh[0], sh[1]), __fadd_rn(sh[2], sh[3]));
  __syncthreads();
  return t;
}

// p = 1/N_g, done = 0, dangling[g] = (sum over the graph's zero-out-degree nodes of 1/N_g) / N_g
__global__ void __launch_bounds__(PR_THREADS) pagerank_init_kernel(const float* __restrict__ out_deg,
                                                                   const int64_t* __restrict__ graph_ptr,
                                                                   float* __restrict__ p, float* __restrict__ dangling,
                                                                   int* __restrict__ done, int* __restrict__ iters) {
  __shared__ float sh[4];
  const int g = blockIdx.x;
  const int64_t lo = graph_ptr[g], hi = graph_ptr[g + 1];
  const float n = (float)(hi - lo);
  const float p0 = 1.0f / n;
  float dang = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += PR_THREADS) {
    p[i] = p0;
    if (out_deg[i] == 0.f) dang = __fadd_rn(dang, p0);
  }
  dang = block_sum_256(dang, sh);
  if (threadIdx.x == 0) {
    dangling[g] = dang / n;
    done[g] = hi > lo ? 0 : 1;
    iters[g] = 0;
  }
}

// new_p[j] = (1 - d)/N + d * (sum_i adj[i][j] / out_deg[i] * p[i] + dangling)   for every node j of an unconverged graph
__global__ void __launch_bounds__(PR_THREADS) pagerank_step_kernel(const int64_t* __restrict__ rowptrT,
                                                                   const int32_t* __restrict__ colT,
                                                                   const float* __restrict__ valT,
                                                                   const float* __restrict__ out_deg,
                                                                   const int64_t* __restrict__ graph_ptr,
                                                                   const int32_t* __restrict__ graph_of, int64_t n, float d,
                                                                   const float* __restrict__ p, const float* __restrict__ dangling,
                                                                   const int* __restrict__ done, float* __restrict__ new_p) {
  const int64_t j = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  if (j >= n) return;
  const int g = graph_of[j];
  if (done[g]) return;
  const float ng = (float)(graph_ptr[g + 1] - graph_ptr[g]);
  float s = 0.f;
  for (int64_t e = rowptrT[j]; e < rowptrT[j + 1]; ++e) {
    const int i = colT[e];
    s = fmaf(valT[e] / out_deg[i], p[i], s);  // (a dangling node has no out-edge, so out_deg[i] != 0 here)
  }
  new_p[j] = __fadd_rn((1.0f - d) / ng, __fmul_rn(d, __fadd_rn(s, dangling[g])));
}

// one workgroup per graph: ||new_p - p||_1 < eps ? keep p and mark done : p = new_p; dangling mass of the new iterate
__global__ void __launch_bounds__(PR_THREADS) pagerank_check_kernel(const float* __restrict__ out_deg,
                                                                    const int64_t* __restrict__ graph_ptr, float eps,
                                                                    float* __restrict__ p, const float* __restrict__ new_p,
                                                                    float* __restrict__ dangling, int* __restrict__ done,
                                                                    int* __restrict__ iters) {
  __shared__ float sh[4];
  const int g = blockIdx.x;
  if (done[g]) return;
  const int64_t lo = graph_ptr[g], hi = graph_ptr[g + 1];
  float diff = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += PR_THREADS) diff = __fadd_rn(diff, fabsf(__fsub_rn(new_p[i], p[i])));
  diff = block_sum_256(diff, sh);
  if (diff < eps) {  // InverseSampling.py:41-43: break before `p = new_p`
    if (threadIdx.x == 0) done[g] = 1;
    return;
  }
  const float n = (float)(hi - lo);
  float dang = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += PR_THREADS) {
    const float v = new_p[i];
    p[i] = v;
    if (out_deg[i] == 0.f) dang = __fadd_rn(dang, v);
  }
  dang = block_sum_256(dang, sh);
  if (threadIdx.x == 0) {
    dangling[g] = dang / n;
    iters[g] += 1;
  }
}

// InverseSampling.compute_sample_prob (:6-19): importance = alpha * pagerank + (1 - alpha) * degree / (N - 1);
// prob = (1 / (importance + eps)) / sum over the graph.  One workgroup per graph, fixed-order sum.
__global__ void __launch_bounds__(PR_THREADS) sample_prob_kernel(const float* __restrict__ pagerank,
                                                                 const float* __restrict__ col_sum,
                                                                 const int64_t* __restrict__ graph_ptr, float alpha, float eps,
                                                                 float* __restrict__ prob) {
  __shared__ float sh[4];
  const int g = blockIdx.x;
  const int64_t lo = graph_ptr[g], hi = graph_ptr[g + 1];
  const float nm1 = (float)(hi - lo - 1);
  float tot = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += PR_THREADS) {
    const float imp = __fadd_rn(__fmul_rn(alpha, pagerank[i]), __fmul_rn(1.0f - alpha, col_sum[i] / nm1));
    const float inv = 1.0f / __fadd_rn(imp, eps);
    prob[i] = inv;
    tot = __fadd_rn(tot, inv);
  }
  tot = block_sum_256(tot, sh);
  for (int64_t i = lo + threadIdx.x; i < hi; i += PR_THREADS) prob[i] = prob[i] / tot;
}

// row sums of a CSR matrix (sequential fp32 adds in CSR order): out-degrees; on the transposed CSR: column sums
__global__ void __launch_bounds__(256) csr_row_sums_kernel(const int64_t* __restrict__ rowptr, const float* __restrict__ val,
                                                           int64_t n, float* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  float s = 0.f;
  for (int64_t e = rowptr[r]; e < rowptr[r + 1]; ++e) s = __fadd_rn(s, val[e]);
  out[r] = s;
}

// Batched Floyd-Warshall + position codes for G small graphs of n <= 64 nodes each (the sampled toy graphs: n = 10): one
// workgroup per graph, the distance matrix in LDS.  dist init as PositionAwareEncoder.py:38-41 (0 -> inf, diagonal 0),
// then n min-plus steps (row k and column k are fixed points of step k, so the in-place update is race-free between
// barriers); code[u][a] = 1 / (dist[u][anchor_a] + 1) if that distance < dis_q else 0 (:14-22).
__global__ void __launch_bounds__(256) fw_position_batch_kernel(const float* __restrict__ adj, int n,
                                                                const int64_t* __restrict__ anchors, int A, float dis_q,
                                                                float* __restrict__ dist_out, float* __restrict__ code_out) {
  __shared__ float d[64 * 64];
  const int g = blockIdx.x;
  const float* a = adj + (int64_t)g * n * n;
  for (int e = threadIdx.x; e < n * n; e += 256) {
    const int i = e / n, j = e % n;
    const float v = a[e];
    d[e] = (i == j) ? 0.f : (v == 0.f ? __builtin_huge_valf() : v);
  }
  __syncthreads();
  for (int kk = 0; kk < n; ++kk) {
    for (int e = threadIdx.x; e < n * n; e += 256) {
      const int i = e / n, j = e % n;
      const float via = __fadd_rn(d[i * n + kk], d[kk * n + j]);
      if (via < d[e]) d[e] = via;
    }
    __syncthreads();
  }
  if (dist_out)
    for (int e = threadIdx.x; e < n * n; e += 256) dist_out[(int64_t)g * n * n + e] = d[e];
  for (int e = threadIdx.x; e < n * A; e += 256) {
    const int u = e / A, ai = e % A;
    const float dd = d[u * n + (int)anchors[(int64_t)g * A + ai]];
    code_out[(int64_t)g * n * A + e] = (dd < dis_q) ? 1.f / (dd + 1.f) : 0.f;
  }
}

// ---- the stochastic half: augmentation and inverse-importance sampling drawn on the device ---------------------------------
// Augmentation.augment_features / augment_adj (RAGraph_node/ragraph_utils/Augmentation.py:8-29), torch.multinomial
// (ToyGraphBase.py:98, RAGraph_edge/modules/RAGraph.py:213), adj[pick][:, pick] (ToyGraphBase.py:100).  Every draw is one
// lp_draw word (rng.h): a slot's fate depends on (seed, row, draw) only, never on how the work is split, and every rule is
// restated in numpy by tests/bank_rng_oracle.py.  No buffer here is proportional to the number of node PAIRS of a graph.

// the g with graph_ptr[g] <= i < graph_ptr[g + 1] (graph_ptr[0] <= i < graph_ptr[G]; empty graphs are stepped over)
__device__ __forceinline__ int64_t graph_of_node(const int64_t* __restrict__ graph_ptr, int64_t G, int64_t i) {
  int64_t lo = 0, hi = G;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (graph_ptr[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// One wave per row i of the batch; lane u looks at the slots (i, jb + u) of i's graph.  Slot (i, j) is kept iff
// u53(lp_draw(seed, i, j - lo)) < (p_i + p_j) * 0.5f (Augmentation.py:23-27, the diagonal included).  FILL = false: cnt[i] = the
// kept slots of the row; FILL = true: the same hashes again, the kept columns written in ascending order behind rowptr[i].
template <bool FILL>
__global__ void __launch_bounds__(256) edge_rewrite_kernel(const int64_t* __restrict__ seed_p, const float* __restrict__ prob,
                                                           const int64_t* __restrict__ graph_ptr, int64_t G, int64_t n,
                                                           int* __restrict__ cnt, int64_t* __restrict__ status,
                                                           const int64_t* __restrict__ rowptr, int32_t* __restrict__ col,
                                                           float* __restrict__ val, int64_t capacity) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (!FILL && blockIdx.x == 0 && threadIdx.x == 0) {
    cnt[n] = 0;      // (the scan runs over n + 1 counts: its last output is the total)
    status[1] = 0;   // (the overflow word, raised by widen_rowptr_kernel)
  }
  if (i >= n) return;
  const int64_t g = graph_of_node(graph_ptr, G, i);
  const int64_t lo = graph_ptr[g] > 0 ? graph_ptr[g] : 0;
  const int64_t hi = graph_ptr[g + 1] < n ? graph_ptr[g + 1] : n;
  const bool mine = lo <= i && i < hi;   // (false only for a graph_ptr that does not cover [0, n): such a row stays empty)
  const uint64_t rk = splitmix64((uint64_t)seed_p[0] ^ splitmix64((uint64_t)i));   // lp_draw's row part, once per row
  const float pi = prob[i];
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int64_t pos = FILL ? rowptr[i] : 0;
  int c = 0;
  for (int64_t jb = lo; mine && jb < hi; jb += 64) {   // (wave-uniform trip count: a ballot inside)
    const int64_t j = jb + lane;
    bool keep = false;
    if (j < hi) keep = lp_event(splitmix64(rk + (uint64_t)(j - lo)), __fmul_rn(__fadd_rn(pi, prob[j]), 0.5f));
    const unsigned long long m = __ballot(keep);
    if (FILL) {
      const int64_t at = pos + __popcll(m & below);
      if (keep && at >= 0 && at < capacity) {
        col[at] = (int32_t)j;
        val[at] = 1.f;
      }
      pos += __popcll(m);
    } else {
      c += __popcll(m);
    }
  }
  if (!FILL && lane == 0) cnt[i] = c;
}

// rowptr[k] = excl[k] for k <= n (excl: the int32 exclusive scan of n counts and a trailing zero), total[0] = excl[n].
// Every count is below 2^31, so the FIRST prefix that reaches 2^31 is still below 2^32: it shows as a negative int32 whatever
// wrapped after it -- overflow[0] = 1 then (the caller zeroes it first), and the caller reports an error.
__global__ void __launch_bounds__(256) widen_rowptr_kernel(const int* __restrict__ excl, int64_t n, int64_t* __restrict__ rowptr,
                                                           int64_t* __restrict__ total, int64_t* __restrict__ overflow) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k > n) return;
  const int v = excl[k];
  rowptr[k] = (int64_t)(uint32_t)v;
  if (v < 0 && overflow) overflow[0] = 1;
  if (k == n) total[0] = (int64_t)(uint32_t)v;
}

// ---- multinomial with replacement over segments ------------------------------------------------------------------------------
// Integer weights: w_i = (uint64)((double)min(p_i, 1) * 2^40), 0 for a negative or NaN p_i -- sums of them are exact, so the
// prefix a draw is compared with does not depend on the shape of the scan.  Level 1: the sums of tiles of 64 entries of the
// whole array (tile boundaries ignore the segments) and their exclusive prefix P; level 2: one wave per draw.
constexpr int MN_TILE = 64;
__device__ __forceinline__ uint64_t mn_weight(float p) {
  return p > 0.f ? (uint64_t)((double)fminf(p, 1.f) * 0x1p40) : 0ull;   // (NaN > 0 is false)
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// tsum[t] = the weights of tile t, t <= nt = ceil(n / 64) (the tile behind the last is empty: its prefix is the total)
__global__ void __launch_bounds__(256) mn_tile_sums_kernel(const float* __restrict__ prob, int64_t n, int64_t nt,
                                                           uint64_t* __restrict__ tsum) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t > nt) return;
  const int64_t i = t * MN_TILE + lane;
  const uint64_t s = wave_sum_u64(i < n ? mn_weight(prob[i]) : 0ull);
  if (lane == 0) tsum[t] = s;
}

// in place, one workgroup: P[t] = sum of tsum[0 .. t).  Thread u owns a contiguous run of entries.
__global__ void __launch_bounds__(256) mn_tile_scan_kernel(uint64_t* __restrict__ tsum, int64_t m) {
  __shared__ uint64_t sh[256];
  const int64_t per = (m + 255) / 256;
  const int64_t lo = (int64_t)threadIdx.x * per < m ? (int64_t)threadIdx.x * per : m;
  const int64_t hi = lo + per < m ? lo + per : m;
  uint64_t s = 0;
  for (int64_t k = lo; k < hi; ++k) s += tsum[k];
  sh[threadIdx.x] = s;
  __syncthreads();
  uint64_t run = 0;
  for (int u = 0; u < (int)threadIdx.x; ++u) run += sh[u];
  for (int64_t k = lo; k < hi; ++k) {
    const uint64_t v = tsum[k];
    tsum[k] = run;
    run += v;
  }
}

// One wave per draw (g, s).  F(x) = the weights of the entries below x = P[x / 64] + the head of x's tile.  W_g = F(hi) - F(lo),
// t = lp_below(lp_draw(seed, g, s), W_g); the answer is the smallest i in [lo, hi) with F(i + 1) > F(lo) + t: the last tile k
// with P[k] <= F(lo) + t holds it, and an inclusive wave scan over that tile finds it.  An entry of weight 0 has the prefix of
// its predecessor, so it is never the smallest; W_g = 0 gives -1.
__global__ void __launch_bounds__(256) mn_draw_kernel(const int64_t* __restrict__ seed_p, const float* __restrict__ prob,
                                                      const int64_t* __restrict__ seg_ptr, int64_t G, int S, int64_t n,
                                                      const uint64_t* __restrict__ P, int64_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t d = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= G * S) return;
  const int64_t g = d / S, s = d - g * S;
  int64_t lo = seg_ptr[g], hi = seg_ptr[g + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > n ? n : hi;
  auto below = [&](int64_t x) {   // F(x), 0 <= x <= n
    const int64_t i = (x >> 6) * MN_TILE + lane;
    return P[x >> 6] + wave_sum_u64(i < x ? mn_weight(prob[i]) : 0ull);
  };
  int64_t res = -1;
  if (lo < hi) {
    const uint64_t f_lo = below(lo);
    const uint64_t W = below(hi) - f_lo;
    if (W != 0) {
      const uint64_t target = f_lo + lp_below(lp_draw((uint64_t)seed_p[0], (uint64_t)g, (uint64_t)s), W);
      int64_t ka = lo >> 6, kb = (hi - 1) >> 6;   // P[ka] <= target; the answer's tile is the last k <= kb with P[k] <= target
      while (ka < kb) {
        const int64_t mid = (ka + kb + 1) >> 1;
        if (P[mid] <= target) ka = mid; else kb = mid - 1;
      }
      const int64_t i = ka * MN_TILE + lane;
      uint64_t incl = i < hi ? mn_weight(prob[i]) : 0ull;   // (entries below lo count: their prefixes are <= F(lo) <= target)
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint64_t up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
      }
      const unsigned long long m = __ballot(P[ka] + incl > target);
      if (m) res = ka * MN_TILE + (__ffsll((long long)m) - 1);
    }
  }
  if (lane == 0) out[d] = res;
}

// ---- adj[pick_g][:, pick_g] ----------------------------------------------------------------------------------------------------
// One lane per entry (g, a, b) of the dense [G, S, S]: the first slot of row pick[g, a] whose column is >= pick[g, b] (the
// columns of a row ascend), its value when the column is the one asked for, else 0.  A pick outside [0, n) (the -1 of an
// all-zero segment) gives a zero row and column.
__global__ void __launch_bounds__(256) csr_induced_blocks_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                 const float* __restrict__ val, int64_t n, int64_t nnz,
                                                                 const int64_t* __restrict__ pick, int64_t G, int S,
                                                                 float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= G * S * S) return;
  const int64_t ga = e / S;
  const int b = (int)(e - ga * S);
  const int64_t r = pick[ga], c = pick[ga - ga % S + b];
  float v = 0.f;
  if (r >= 0 && r < n && c >= 0 && c < n) {
    int64_t lo = rowptr[r], hi = rowptr[r + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > nnz ? nnz : hi;
    const int64_t end = hi;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)col[mid] < c) lo = mid + 1; else hi = mid;
    }
    if (lo < end && (int64_t)col[lo] == c) v = val[lo];
  }
  out[e] = v;
}

// ---- [G, S, S] dense blocks, S <= 64 -> block-diagonal CSR ------------------------------------------------------------------
// One wave per row (g, a); lane b holds entry (g, a, b).  An entry is kept iff it compares unequal to 0 (so -0 is dropped and a
// NaN kept, as torch.nonzero does).  FILL = false: the row's count; FILL = true: columns g * S + b ascending, the values as
// they are, behind excl[row].
template <bool FILL>
__global__ void __launch_bounds__(256) blocks_to_csr_kernel(const float* __restrict__ blocks, int64_t rows, int S,
                                                            int* __restrict__ cnt, const int* __restrict__ excl,
                                                            int32_t* __restrict__ col, float* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (!FILL && blockIdx.x == 0 && threadIdx.x == 0) cnt[rows] = 0;
  if (r >= rows) return;
  const float v = lane < S ? blocks[r * S + lane] : 0.f;
  const bool keep = lane < S && v != 0.f;
  const unsigned long long m = __ballot(keep);
  if (FILL) {
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    if (keep) {
      const int64_t at = (int64_t)excl[r] + __popcll(m & below);
      col[at] = (int32_t)(r - r % S + lane);
      val[at] = v;
    }
  } else if (lane == 0) {
    cnt[r] = __popcll(m);
  }
}

// ---- Augmentation.augment_features (Augmentation.py:8-22) ------------------------------------------------------------------
// One lane per pair of columns, as add_normal_noise_kernel (noise.hip) with J = 1.  Row i is kept iff
// u53(lp_draw(seed_drop, id_i, 0)) < p_i * rate; a kept row is x + std * z with the z of add_normal_noise for that id (the same
// bits); a dropped row is +0 in every column, and no normal is computed for it.
__global__ void __launch_bounds__(256) augment_features_kernel(const float* X, int64_t n, int D,
                                                               const float* __restrict__ prob, float rate, float std,
                                                               const int64_t* __restrict__ seed_drop,
                                                               const int64_t* __restrict__ seed_noise,
                                                               const int64_t* __restrict__ row_ids, int64_t row_base,
                                                               float* out) {
  const int64_t P = (D + 1) >> 1;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * P) return;
  const int64_t r = i / P;
  const int p = (int)(i - r * P);
  const uint64_t id = noise_row_id(row_ids, row_base, r);
  const int64_t o = r * D + 2 * p;
  const bool two = 2 * p + 1 < D;
  float y0 = 0.f, y1 = 0.f;
  if (lp_event(lp_draw((uint64_t)seed_drop[0], id, 0), __fmul_rn(prob[r], rate))) {
    float z0, z1;
    normal_pair((uint64_t)seed_noise[0], id, (uint64_t)p, z0, z1);
    y0 = __fadd_rn(X[o], __fmul_rn(std, z0));
    if (two) y1 = __fadd_rn(X[o + 1], __fmul_rn(std, z1));
  }
  out[o] = y0;
  if (two) out[o + 1] = y1;
}

}  // namespace ragraph

using namespace ragraph;

extern "C" size_t ragraph_pagerank_workspace_bytes(int64_t n, int64_t G) {
  return align_up((size_t)n * sizeof(float), 256) + align_up((size_t)G * sizeof(float), 256) +
         align_up((size_t)G * sizeof(int), 256);
}

extern "C" int ragraph_pagerank_f32(const int64_t* rowptrT, const int32_t* colT, const float* valT, const float* out_deg,
                                    const int64_t* graph_ptr, const int32_t* graph_of, int64_t G, int64_t n, float d, float eps,
                                    int max_iter, float* p, int* iters, void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(rowptrT && colT && valT && out_deg && graph_ptr && graph_of && p && iters && ws, RAGRAPH_EINVAL,
             "pagerank: null pointer");
  RG_REQUIRE(G >= 1 && n >= 1 && max_iter >= 1, RAGRAPH_EINVAL, "pagerank: bad G/n/max_iter");
  RG_REQUIRE(ws_bytes >= ragraph_pagerank_workspace_bytes(n, G), RAGRAPH_EWORKSPACE, "pagerank: workspace too small");
  hipStream_t st = as_stream(stream);
  char* w = static_cast<char*>(ws);
  float* new_p = reinterpret_cast<float*>(w);
  float* dangling = reinterpret_cast<float*>(w + align_up((size_t)n * sizeof(float), 256));
  int* done = reinterpret_cast<int*>(reinterpret_cast<char*>(dangling) + align_up((size_t)G * sizeof(float), 256));
  hipLaunchKernelGGL(pagerank_init_kernel, dim3((unsigned)G), dim3(PR_THREADS), 0, st, out_deg, graph_ptr, p, dangling, done,
                     iters);
  for (int it = 0; it < max_iter; ++it) {
    hipLaunchKernelGGL(pagerank_step_kernel, dim3((unsigned)cdiv(n, PR_THREADS)), dim3(PR_THREADS), 0, st, rowptrT, colT, valT,
                       out_deg, graph_ptr, graph_of, n, d, p, dangling, done, new_p);
    hipLaunchKernelGGL(pagerank_check_kernel, dim3((unsigned)G), dim3(PR_THREADS), 0, st, out_deg, graph_ptr, eps, p, new_p,
                       dangling, done, iters);
  }
  RG_CHECK_LAUNCH("pagerank");
  return RAGRAPH_OK;
}

extern "C" int ragraph_sample_prob_f32(const float* pagerank, const float* col_sum, const int64_t* graph_ptr, int64_t G,
                                       float alpha, float eps, float* prob, void* stream) {
  RG_REQUIRE(pagerank && col_sum && graph_ptr && prob, RAGRAPH_EINVAL, "sample_prob: null pointer");
  if (G <= 0) return RAGRAPH_OK;
  hipLaunchKernelGGL(sample_prob_kernel, dim3((unsigned)G), dim3(PR_THREADS), 0, as_stream(stream), pagerank, col_sum,
                     graph_ptr, alpha, eps, prob);
  RG_CHECK_LAUNCH("sample_prob");
  return RAGRAPH_OK;
}

extern "C" int ragraph_csr_row_sums_f32(const int64_t* rowptr, const float* val, int64_t n, float* out, void* stream) {
  RG_REQUIRE(rowptr && val && out, RAGRAPH_EINVAL, "csr_row_sums: null pointer");
  if (n <= 0) return RAGRAPH_OK;
  hipLaunchKernelGGL(csr_row_sums_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, as_stream(stream), rowptr, val, n, out);
  RG_CHECK_LAUNCH("csr_row_sums");
  return RAGRAPH_OK;
}

extern "C" int ragraph_position_codes_batch_f32(const float* adj, int64_t G, int n, const int64_t* anchors, int A, float dis_q,
                                                float* dist_out, float* codes, void* stream) {
  RG_REQUIRE(adj && anchors && codes, RAGRAPH_EINVAL, "position_codes_batch: null pointer");
  RG_REQUIRE(n >= 1 && n <= 64 && A >= 1, RAGRAPH_EUNSUPPORTED, "position_codes_batch: n=%d not in [1,64]", n);
  if (G <= 0) return RAGRAPH_OK;
  hipLaunchKernelGGL(fw_position_batch_kernel, dim3((unsigned)G), dim3(256), 0, as_stream(stream), adj, n, anchors, A, dis_q,
                     dist_out, codes);
  RG_CHECK_LAUNCH("position_codes_batch");
  return RAGRAPH_OK;
}

// ---- the stochastic half ---------------------------------------------------------------------------------------------------
static size_t counts_scan_bytes(int64_t rows) {   // rows + 1 int32 counts (scanned in place) + the scan's own scratch
  return align_up((size_t)(rows + 1) * sizeof(int), 256) + scan_temp_bytes(rows + 1);
}

extern "C" size_t ragraph_edge_rewrite_workspace_bytes(int64_t n) { return counts_scan_bytes(n > 0 ? n : 0); }

extern "C" int ragraph_edge_rewrite_csr(const int64_t* seed, const float* prob, const int64_t* graph_ptr, int64_t G, int64_t n,
                                        int64_t* rowptr, int64_t* status, int32_t* col, float* val, int64_t capacity, void* ws,
                                        size_t ws_bytes, void* stream) {
  RG_REQUIRE(seed, RAGRAPH_EINVAL, "edge_rewrite: null seed");
  RG_REQUIRE(prob && graph_ptr && rowptr, RAGRAPH_EINVAL, "edge_rewrite: null pointer");
  RG_REQUIRE(G >= 1 && n >= 1 && n <= (int64_t)INT_MAX - 1, RAGRAPH_EINVAL, "edge_rewrite: bad G=%lld / n=%lld", (long long)G,
             (long long)n);
  RG_REQUIRE((col == nullptr) == (val == nullptr), RAGRAPH_EINVAL, "edge_rewrite: col and val go together");
  hipStream_t st = as_stream(stream);
  const unsigned row_blocks = (unsigned)cdiv(n, 4);
  if (col) {   // the fill pass
    RG_REQUIRE(capacity >= 1, RAGRAPH_EINVAL, "edge_rewrite: capacity=%lld", (long long)capacity);
    hipLaunchKernelGGL(edge_rewrite_kernel<true>, dim3(row_blocks), dim3(256), 0, st, seed, prob, graph_ptr, G, n, (int*)nullptr,
                       (int64_t*)nullptr, (const int64_t*)rowptr, col, val, capacity);
    RG_CHECK_LAUNCH("edge_rewrite(fill)");
    return RAGRAPH_OK;
  }
  RG_REQUIRE(status && ws, RAGRAPH_EINVAL, "edge_rewrite: null pointer");
  RG_REQUIRE(ws_bytes >= ragraph_edge_rewrite_workspace_bytes(n), RAGRAPH_EWORKSPACE, "edge_rewrite: workspace too small");
  int* cnt = static_cast<int*>(ws);
  const size_t cnt_bytes = align_up((size_t)(n + 1) * sizeof(int), 256);
  hipLaunchKernelGGL(edge_rewrite_kernel<false>, dim3(row_blocks), dim3(256), 0, st, seed, prob, graph_ptr, G, n, cnt, status,
                     (const int64_t*)nullptr, (int32_t*)nullptr, (float*)nullptr, (int64_t)0);
  RG_CHECK_LAUNCH("edge_rewrite(count)");
  const int rc = scan_sum_i32(cnt, cnt, n + 1, false, static_cast<char*>(ws) + cnt_bytes, ws_bytes - cnt_bytes, st);
  if (rc != RAGRAPH_OK) return rc;
  hipLaunchKernelGGL(widen_rowptr_kernel, dim3((unsigned)cdiv(n + 1, 256)), dim3(256), 0, st, (const int*)cnt, n, rowptr, status,
                     status + 1);
  RG_CHECK_LAUNCH("edge_rewrite(rowptr)");
  return RAGRAPH_OK;
}

extern "C" size_t ragraph_multinomial_segments_workspace_bytes(int64_t n) {
  return align_up((size_t)(cdiv(n > 0 ? n : 0, MN_TILE) + 1) * sizeof(uint64_t), 256);
}

extern "C" int ragraph_multinomial_segments_i64(const int64_t* seed, const float* prob, int64_t n, const int64_t* seg_ptr,
                                                int64_t G, int S, int64_t* out, void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(seed, RAGRAPH_EINVAL, "multinomial_segments: null seed");
  RG_REQUIRE(prob && seg_ptr && out && ws, RAGRAPH_EINVAL, "multinomial_segments: null pointer");
  RG_REQUIRE(G >= 1 && S >= 1 && n >= 1, RAGRAPH_EINVAL, "multinomial_segments: bad G=%lld / S=%d / n=%lld", (long long)G, S,
             (long long)n);
  // every segment lies inside [0, n): n < 2^23 bounds each of them, and their weights (<= 2^40 each) sum below 2^63
  RG_REQUIRE(n < ((int64_t)1 << 23), RAGRAPH_EINVAL, "multinomial_segments: n=%lld, segments must be shorter than 2^23",
             (long long)n);
  RG_REQUIRE(G <= (((int64_t)1 << 33) - 4) / S, RAGRAPH_EINVAL, "multinomial_segments: G * S too large");
  RG_REQUIRE(ws_bytes >= ragraph_multinomial_segments_workspace_bytes(n), RAGRAPH_EWORKSPACE,
             "multinomial_segments: workspace too small");
  hipStream_t st = as_stream(stream);
  uint64_t* P = static_cast<uint64_t*>(ws);
  const int64_t nt = cdiv(n, MN_TILE);
  hipLaunchKernelGGL(mn_tile_sums_kernel, dim3((unsigned)cdiv(nt + 1, 4)), dim3(256), 0, st, prob, n, nt, P);
  hipLaunchKernelGGL(mn_tile_scan_kernel, dim3(1), dim3(256), 0, st, P, nt + 1);
  hipLaunchKernelGGL(mn_draw_kernel, dim3((unsigned)cdiv(G * S, 4)), dim3(256), 0, st, seed, prob, seg_ptr, G, S, n,
                     (const uint64_t*)P, out);
  RG_CHECK_LAUNCH("multinomial_segments");
  return RAGRAPH_OK;
}

extern "C" int ragraph_csr_induced_blocks_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n, int64_t nnz,
                                              const int64_t* pick, int64_t G, int S, float* out, void* stream) {
  RG_REQUIRE(rowptr && pick && out, RAGRAPH_EINVAL, "csr_induced_blocks: null pointer");
  RG_REQUIRE(nnz >= 0 && (nnz == 0 || (col && val)), RAGRAPH_EINVAL, "csr_induced_blocks: null pointer");
  RG_REQUIRE(G >= 1 && S >= 1 && n >= 1, RAGRAPH_EINVAL, "csr_induced_blocks: bad G=%lld / S=%d / n=%lld", (long long)G, S,
             (long long)n);
  RG_REQUIRE(G <= (((int64_t)1 << 39) - 256) / S / S, RAGRAPH_EINVAL, "csr_induced_blocks: G * S * S too large");
  hipLaunchKernelGGL(csr_induced_blocks_kernel, dim3((unsigned)cdiv(G * S * S, 256)), dim3(256), 0, as_stream(stream), rowptr,
                     col, val, n, nnz, pick, G, S, out);
  RG_CHECK_LAUNCH("csr_induced_blocks");
  return RAGRAPH_OK;
}

extern "C" size_t ragraph_blocks_to_csr_workspace_bytes(int64_t G, int S) {
  return counts_scan_bytes(G > 0 && S > 0 ? G * S : 0);
}

extern "C" int ragraph_blocks_to_csr_f32(const float* blocks, int64_t G, int S, int64_t* rowptr, int32_t* col, float* val,
                                         int64_t* nnz, void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(blocks && rowptr && col && val && nnz && ws, RAGRAPH_EINVAL, "blocks_to_csr: null pointer");
  RG_REQUIRE(G >= 1 && S >= 1 && S <= 64, RAGRAPH_EINVAL, "blocks_to_csr: bad G=%lld / S=%d (S <= 64)", (long long)G, S);
  RG_REQUIRE(G <= (int64_t)INT_MAX / S / S, RAGRAPH_EINVAL, "blocks_to_csr: G * S * S too large");
  RG_REQUIRE(ws_bytes >= ragraph_blocks_to_csr_workspace_bytes(G, S), RAGRAPH_EWORKSPACE, "blocks_to_csr: workspace too small");
  hipStream_t st = as_stream(stream);
  const int64_t rows = G * S;
  int* cnt = static_cast<int*>(ws);
  const size_t cnt_bytes = align_up((size_t)(rows + 1) * sizeof(int), 256);
  const unsigned row_blocks = (unsigned)cdiv(rows, 4);
  hipLaunchKernelGGL(blocks_to_csr_kernel<false>, dim3(row_blocks), dim3(256), 0, st, blocks, rows, S, cnt, (const int*)nullptr,
                     (int32_t*)nullptr, (float*)nullptr);
  RG_CHECK_LAUNCH("blocks_to_csr(count)");
  const int rc = scan_sum_i32(cnt, cnt, rows + 1, false, static_cast<char*>(ws) + cnt_bytes, ws_bytes - cnt_bytes, st);
  if (rc != RAGRAPH_OK) return rc;
  hipLaunchKernelGGL(widen_rowptr_kernel, dim3((unsigned)cdiv(rows + 1, 256)), dim3(256), 0, st, (const int*)cnt, rows, rowptr,
                     nnz, (int64_t*)nullptr);
  hipLaunchKernelGGL(blocks_to_csr_kernel<true>, dim3(row_blocks), dim3(256), 0, st, blocks, rows, S, (int*)nullptr,
                     (const int*)cnt, col, val);
  RG_CHECK_LAUNCH("blocks_to_csr(fill)");
  return RAGRAPH_OK;
}

extern "C" int ragraph_augment_features_f32(const float* X, int64_t n, int D, const float* prob, float rate, float std,
                                            const int64_t* seed_drop, const int64_t* seed_noise, const int64_t* row_ids,
                                            int64_t row_base, float* out, void* stream) {
  RG_REQUIRE(seed_drop && seed_noise, RAGRAPH_EINVAL, "augment_features: null seed");
  RG_REQUIRE(n >= 0 && D >= 1, RAGRAPH_EINVAL, "augment_features: bad shape (n=%lld, D=%d)", (long long)n, D);
  const int64_t P = ((int64_t)D + 1) >> 1;
  RG_REQUIRE(n <= (((int64_t)1 << 39) - 256) / P, RAGRAPH_EINVAL, "augment_features: n * D too large");
  if (n == 0) return RAGRAPH_OK;
  RG_REQUIRE(X && prob && out, RAGRAPH_EINVAL, "augment_features: null pointer");
  hipLaunchKernelGGL(augment_features_kernel, dim3((unsigned)cdiv(n * P, 256)), dim3(256), 0, as_stream(stream), X, n, D, prob,
                     rate, std, seed_drop, seed_noise, row_ids, row_base, out);
  RG_CHECK_LAUNCH("augment_features");
  return RAGRAPH_OK;
}
