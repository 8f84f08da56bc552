// Link-prediction pre-training (RAGraph_node/preprompt.py:80-126; RAGraph_graph/preprompt.py the same with 50 negatives):
//   * ragraph_lp_sample_i64: prompt_pretrain_sample over the CSR pattern of A, one wave per row.  A counter-based hash of
//     (seed, row, draw) -- the seed read from device memory -- draws the positive and, by Floyd's algorithm over ranks kept
//     in LDS, n_neg distinct ranks among the row's non-neighbours; a binary search over the sorted neighbour list maps
//     rank r to the r-th node that is not a neighbour.
//   * ragraph_lp_compare_loss_fwd_f32: compareloss as a sampled dense-dense product.  One pass normalises the rows of h
//     (torch's F.cosine_similarity: x / max(||x||, 1e-8)), one wave per row then reads its own row and its 1 + n_neg
//     partner rows, 16 lanes per partner, and writes L_i with the backward coefficients c = dL_i/dsim and c * sim; the
//     mean is one workgroup's fixed-order reduction.  No [n, 1 + n_neg, D] tensor exists.
//   * ragraph_lp_combine_f32: the backward's epilogue, s * (X / N_r - beta_r h_r / (N_r ||h_r||)), after the SpMMs of the
//     existing kernels (own and transposed sample pattern) have made X and beta.
// Both entries that take indices check them first (one 4-byte read-back) and return RAGRAPH_EINVAL before writing.
//
// Edge (link-prediction) flavour pre-training (RAGraph_edge/utils/dataloader.py:140-152, negative_sampling):
//   * ragraph_edge_hist_check_i64: the training-history CSR (item ids strictly ascending per user) is checked once, when it
//     is built: ids in range, order, and no user whose history covers every item (the reference's loop never ends there).
//   * ragraph_edge_neg_sample_i64: one lane per output slot.  The reference redraws np.random.randint until the item is not
//     in the user's history; the same law without a loop is a rank r uniform in [0, num_items - deg(u)) mapped to the r-th
//     item outside the history by the binary search of the LP sampler.  No read-back unless the caller asks for the user
//     ids to be checked.
#include "common.h"
#include "rng.h"

namespace ragraph {

constexpr int LP_NEG_MAX = 4096;          // negatives per row (ranks kept in LDS)
constexpr float LP_COS_EPS = 1e-8f;       // F.cosine_similarity's default eps

// (randomness: splitmix64 on (seed, row, draw) -- lp_draw / lp_below, rng.h)

// rank r -> the r-th id that is not in the strictly ascending list at(0) .. at(deg - 1): r + #{j : at(j) - j <= r}
// (at(j) - j never decreases, so a binary search counts them)
template <class At>
__device__ __forceinline__ int64_t lp_rank_to_id(At at, int64_t deg, int64_t r) {
  int64_t a = 0, b = deg;
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if (at(mid) - mid <= r) a = mid + 1; else b = mid;
  }
  return r + a;
}

// ---- sampler ----------------------------------------------------------------------------------------------------------
// Per row: columns in [0, n), strictly ascending; deg' = entries other than the diagonal; a row with neighbours needs
// n - deg' >= n_neg non-neighbours (the reference's broadcast error otherwise).  bad: 1 = ids, 2 = order, 4 = too dense.
__global__ void __launch_bounds__(256) lp_sample_check_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                              int64_t n, int64_t nnz, int n_neg, int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t e0 = rowptr[i], e1 = rowptr[i + 1];
  if (e0 < 0 || e1 < e0 || e1 > nnz) {
    atomicOr(bad, 1);
    return;
  }
  int flags = 0;
  int64_t deg = 0;
  int64_t prev = -1;
  for (int64_t e = e0; e < e1; ++e) {
    const int64_t c = col[e];
    if (c < 0 || c >= n) {
      flags |= 1;
      break;
    }
    if (c <= prev) flags |= 2;
    prev = c;
    deg += c != i;
  }
  if (!flags && deg > 0 && n - deg < n_neg) flags |= 4;
  if (flags) atomicOr(bad, flags);
}

// The j-th neighbour of the row without its diagonal entry (at raw position pd, or none: pd = deg').
__device__ __forceinline__ int64_t lp_neighbour(const int32_t* __restrict__ c, int64_t pd, int64_t j) {
  return c[j < pd ? j : j + 1];
}

__global__ void __launch_bounds__(64) lp_sample_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                       int64_t n, int n_neg, const int64_t* __restrict__ seed_p,
                                                       int64_t* __restrict__ out) {
  __shared__ uint32_t chosen[LP_NEG_MAX];
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  const uint64_t seed = (uint64_t)seed_p[0];
  const int32_t* c = col + rowptr[i];
  const int64_t raw = rowptr[i + 1] - rowptr[i];
  // the diagonal entry (process_tu_dataset's A_hat carries one): its raw position, by binary search
  int64_t lo = 0, hi = raw;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (c[mid] < i) lo = mid + 1; else hi = mid;
  }
  const bool has_diag = lo < raw && c[lo] == i;
  const int64_t deg = raw - (has_diag ? 1 : 0);
  const int64_t pd = has_diag ? lo : deg;
  int64_t* o = out + i * (int64_t)(1 + n_neg);
  if (lane == 0) {  // column 0: a uniformly random neighbour, or i itself (preprompt.py:119-122)
    o[0] = deg == 0 ? i : lp_neighbour(c, pd, (int64_t)lp_below(lp_draw(seed, (uint64_t)i, 0), (uint64_t)deg));
  }
  // Floyd: for j = M - k .. M - 1, draw r in [0, j]; take r unless already taken, then j.  M = n - deg' ranks.
  const uint64_t M = (uint64_t)(n - deg);
  for (int s = 0; s < n_neg; ++s) {
    const uint64_t j = M - (uint64_t)n_neg + (uint64_t)s;
    const uint32_t r = (uint32_t)lp_below(lp_draw(seed, (uint64_t)i, 1 + (uint64_t)s), j + 1);
    bool hit = false;
    for (int q = lane; q < s; q += 64) hit |= chosen[q] == r;
    const bool any = __ballot(hit) != 0;
    if (lane == 0) chosen[s] = any ? (uint32_t)j : r;
    __syncthreads();
  }
  for (int s = lane; s < n_neg; s += 64) {
    o[1 + s] = lp_rank_to_id([=](int64_t j) { return lp_neighbour(c, pd, j); }, deg, (int64_t)chosen[s]);
  }
}

// ---- edge flavour: negatives outside the user's training history -----------------------------------------------------
// Per user: rowptr runs from 0 to nnz without decreasing, items in [0, num_items) strictly ascending, deg < num_items.
// bad: 1 = ids / rowptr, 2 = order, 4 = a history covers every item.
__global__ void __launch_bounds__(256) edge_hist_check_kernel(const int64_t* __restrict__ rowptr,
                                                              const int64_t* __restrict__ items, int64_t num_users,
                                                              int64_t num_items, int64_t nnz, int* __restrict__ bad) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= num_users) return;
  const int64_t e0 = rowptr[u], e1 = rowptr[u + 1];
  if (e0 < 0 || e1 < e0 || e1 > nnz || (u == 0 && e0 != 0) || (u == num_users - 1 && e1 != nnz)) {
    atomicOr(bad, 1);
    return;
  }
  int flags = 0;
  int64_t prev = -1;
  for (int64_t e = e0; e < e1; ++e) {
    const int64_t v = items[e];
    if (v < 0 || v >= num_items) {
      flags |= 1;
      break;
    }
    if (v <= prev) flags |= 2;
    prev = v;
  }
  if (!flags && e1 - e0 >= num_items) flags |= 4;
  if (flags) atomicOr(bad, flags);
}

// Slot s = b * n_negs + j (triple-major, the reference's list order): r = lp_below(lp_draw(seed, s, 0), num_items - deg),
// then the r-th item not in H(users[b]).
__global__ void __launch_bounds__(256) edge_neg_sample_kernel(const int64_t* __restrict__ rowptr,
                                                              const int64_t* __restrict__ items, int64_t num_items,
                                                              const int64_t* __restrict__ users, int64_t total, int n_negs,
                                                              const int64_t* __restrict__ seed_p, int64_t* __restrict__ out) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= total) return;
  const uint64_t seed = (uint64_t)seed_p[0];
  const int64_t u = users[s / n_negs];
  const int64_t e0 = rowptr[u];
  const int64_t deg = rowptr[u + 1] - e0;
  const int64_t* h = items + e0;
  const int64_t r = (int64_t)lp_below(lp_draw(seed, (uint64_t)s, 0), (uint64_t)(num_items - deg));
  out[s] = lp_rank_to_id([=](int64_t j) { return h[j]; }, deg, r);
}

// ---- compare loss -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lp_index_check_kernel(const int64_t* __restrict__ t, int64_t total, int64_t n,
                                                             int* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    const int64_t v = t[e];
    if (v < 0 || v >= n) {
      atomicOr(bad, 1);
      return;
    }
  }
}

// One wave per row: ||h_i|| (the fixed tree of the row norms), hhat_i = h_i / max(||h_i||, eps) (an IEEE division per
// element, as ATen's x / x_norm).
__global__ void __launch_bounds__(256) lp_normalize_kernel(const float* __restrict__ h, int64_t n, int D,
                                                           float* __restrict__ hhat, float* __restrict__ nrm) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;
  const float* x = h + i * (int64_t)D;
  float p = 0.f;
  for (int d = lane; d < D; d += 64) p = fmaf(x[d], x[d], p);
  const float nn = sqrtf(wave_sum_fixed_tree(p));
  const float den = fmaxf(nn, LP_COS_EPS);
  float* y = hhat + i * (int64_t)D;
  for (int d = lane; d < D; d += 64) y[d] = x[d] / den;
  if (lane == 0) nrm[i] = nn;
}

__device__ __forceinline__ float sum16(float p) {
  p += __shfl_xor(p, 8);
  p += __shfl_xor(p, 4);
  p += __shfl_xor(p, 2);
  p += __shfl_xor(p, 1);
  return p;
}

// One wave (one workgroup) per row i; lanes 16g .. 16g + 15 take partner s = s0 + g.
template <bool VEC4>
__global__ void __launch_bounds__(64) lp_loss_kernel(const float* __restrict__ hhat, const int64_t* __restrict__ t, int64_t n,
                                                     int D, int S, float temperature, float* __restrict__ L,
                                                     float* __restrict__ coef, float* __restrict__ csim) {
  __shared__ float sims[LP_NEG_MAX + 1];
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x, g = lane >> 4, gl = lane & 15;
  const float* hi = hhat + i * (int64_t)D;
  const int64_t* ti = t + i * (int64_t)S;
  for (int s0 = 0; s0 < S; s0 += 4) {
    const int s = s0 + g;
    float p = 0.f;
    if (s < S) {
      const float* hj = hhat + ti[s] * (int64_t)D;
      if (VEC4) {
        for (int d = gl * 4; d < D; d += 64) {
          const float4 a = *reinterpret_cast<const float4*>(hi + d);
          const float4 b = *reinterpret_cast<const float4*>(hj + d);
          p = fmaf(a.x, b.x, p);
          p = fmaf(a.y, b.y, p);
          p = fmaf(a.z, b.z, p);
          p = fmaf(a.w, b.w, p);
        }
      } else {
        for (int d = gl; d < D; d += 16) p = fmaf(hi[d], hj[d], p);
      }
    }
    p = sum16(p);
    if (s < S && gl == 0) sims[s] = p;
  }
  __syncthreads();
  // exp(sim) / T (preprompt.py:93-94); denominator over s >= 1 in a fixed order (lane-strided chains, then the fixed tree)
  float part = 0.f;
  for (int s = 1 + lane; s < S; s += 64) part += expf(sims[s]) / temperature;
  const float den = wave_sum_fixed_tree(part);
  const float e0 = expf(sims[0]) / temperature;
  float* ci = coef + i * (int64_t)S;
  float* ki = csim + i * (int64_t)S;
  for (int s = lane; s < S; s += 64) {
    const float sim = sims[s];
    const float cs = s == 0 ? -1.f : (expf(sim) / temperature) / den;   // dL_i/dsim: -1, then the softmax weight of e
    ci[s] = cs;
    ki[s] = cs * sim;
  }
  if (lane == 0) L[i] = -logf(e0 / den);                               // :101
}

// mean of L: 256 lane-strided chains in index order, then a fixed LDS tree; / n last (res.mean())
__global__ void __launch_bounds__(256) lp_mean_kernel(const float* __restrict__ L, int64_t n, float* __restrict__ loss) {
  __shared__ float part[256];
  float a = 0.f;
  for (int64_t j = threadIdx.x; j < n; j += 256) a += L[j];
  part[threadIdx.x] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = part[0] / (float)n;
}

// grad_r = s * (X_r / N_r - beta_r * h_r / (N_r ||h_r||)), N_r = max(||h_r||, eps), s = go[0] / n_rows.  The second term is
// 0 where ||h_r|| = 0 (ATen's norm backward masks a zero norm).
__global__ void __launch_bounds__(256) lp_combine_kernel(const float* __restrict__ X, const float* __restrict__ h,
                                                         const float* __restrict__ nrm, const float* __restrict__ beta,
                                                         const float* __restrict__ go, float inv_rows, int64_t n, int D,
                                                         float* __restrict__ out) {
  const int64_t total = n * (int64_t)D;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t r = e / D;
  const float nn = nrm[r];
  const float N = fmaxf(nn, LP_COS_EPS);
  const float k = nn > 0.f ? beta[r] / (N * nn) : 0.f;
  const float s = go[0] * inv_rows;
  out[e] = s * (X[e] / N - k * h[e]);
}

static int lp_read_flag(const int* bad, hipStream_t st, int* out, const char* what) {
  if (hipMemcpyAsync(out, bad, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    set_error("%s: read-back of the check failed", what);
    return RAGRAPH_EDEVICE;
  }
  return RAGRAPH_OK;
}

}  // namespace ragraph

using namespace ragraph;

extern "C" size_t ragraph_lp_workspace_bytes(void) { return 256; }

extern "C" int ragraph_lp_sample_i64(const int64_t* rowptr, const int32_t* col, int64_t n, int64_t nnz, int n_neg,
                                     const int64_t* seed, int64_t* out, void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(rowptr && seed && out && ws, RAGRAPH_EINVAL, "lp_sample: null pointer");
  RG_REQUIRE(nnz == 0 || col, RAGRAPH_EINVAL, "lp_sample: null col");
  RG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && nnz >= 0, RAGRAPH_EINVAL, "lp_sample: n=%lld nnz=%lld", (long long)n,
             (long long)nnz);
  RG_REQUIRE(n_neg >= 0 && n_neg <= LP_NEG_MAX && n_neg <= n, RAGRAPH_EINVAL, "lp_sample: n_neg=%d not in [0, min(n, %d)]",
             n_neg, LP_NEG_MAX);
  RG_REQUIRE(ws_bytes >= 256, RAGRAPH_EWORKSPACE, "lp_sample: workspace too small");
  hipStream_t st = as_stream(stream);
  int* bad = reinterpret_cast<int*>(ws);
  if (hipMemsetAsync(bad, 0, sizeof(int), st) != hipSuccess) {
    set_error("lp_sample: memset failed");
    return RAGRAPH_EDEVICE;
  }
  hipLaunchKernelGGL(lp_sample_check_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, rowptr, col, n, nnz, n_neg, bad);
  RG_CHECK_LAUNCH("lp_sample(check)");
  int bad_h = 0;
  const int rc = lp_read_flag(bad, st, &bad_h, "lp_sample");
  if (rc != RAGRAPH_OK) return rc;
  RG_REQUIRE(!(bad_h & 1), RAGRAPH_EINVAL, "lp_sample: rowptr / col is not a CSR pattern over %lld nodes", (long long)n);
  RG_REQUIRE(!(bad_h & 2), RAGRAPH_EINVAL, "lp_sample: the columns of a row are not strictly ascending");
  RG_REQUIRE(!(bad_h & 4), RAGRAPH_EINVAL, "lp_sample: a row with neighbours has fewer than n_neg=%d non-neighbours", n_neg);
  hipLaunchKernelGGL(lp_sample_kernel, dim3((unsigned)n), dim3(64), 0, st, rowptr, col, n, n_neg, seed, out);
  RG_CHECK_LAUNCH("lp_sample");
  return RAGRAPH_OK;
}

extern "C" int ragraph_edge_hist_check_i64(const int64_t* rowptr, const int64_t* items, int64_t num_users, int64_t num_items,
                                           int64_t nnz, void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(rowptr && ws, RAGRAPH_EINVAL, "edge_hist_check: null pointer");
  RG_REQUIRE(nnz == 0 || items, RAGRAPH_EINVAL, "edge_hist_check: null items");
  RG_REQUIRE(num_users >= 1 && num_items >= 1 && nnz >= 0, RAGRAPH_EINVAL, "edge_hist_check: num_users=%lld num_items=%lld nnz=%lld",
             (long long)num_users, (long long)num_items, (long long)nnz);
  RG_REQUIRE(ws_bytes >= 256, RAGRAPH_EWORKSPACE, "edge_hist_check: workspace too small");
  hipStream_t st = as_stream(stream);
  int* bad = reinterpret_cast<int*>(ws);
  if (hipMemsetAsync(bad, 0, sizeof(int), st) != hipSuccess) {
    set_error("edge_hist_check: memset failed");
    return RAGRAPH_EDEVICE;
  }
  hipLaunchKernelGGL(edge_hist_check_kernel, dim3((unsigned)cdiv(num_users, 256)), dim3(256), 0, st, rowptr, items, num_users,
                     num_items, nnz, bad);
  RG_CHECK_LAUNCH("edge_hist_check");
  int bad_h = 0;
  const int rc = lp_read_flag(bad, st, &bad_h, "edge_hist_check");
  if (rc != RAGRAPH_OK) return rc;
  RG_REQUIRE(!(bad_h & 1), RAGRAPH_EINVAL, "edge_hist_check: rowptr / items is not a CSR over %lld users and %lld items",
             (long long)num_users, (long long)num_items);
  RG_REQUIRE(!(bad_h & 2), RAGRAPH_EINVAL, "edge_hist_check: the items of a history are not strictly ascending");
  RG_REQUIRE(!(bad_h & 4), RAGRAPH_EINVAL, "edge_hist_check: a user's history covers every item (%lld): no negative exists",
             (long long)num_items);
  return RAGRAPH_OK;
}

extern "C" int ragraph_edge_neg_sample_i64(const int64_t* rowptr, const int64_t* items, int64_t num_users, int64_t num_items,
                                           const int64_t* users, int64_t B, int n_negs, int check_users, const int64_t* seed,
                                           int64_t* out, void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(rowptr && seed, RAGRAPH_EINVAL, "edge_neg_sample: null pointer");
  RG_REQUIRE(num_users >= 1 && num_items >= 1 && B >= 0 && n_negs >= 1, RAGRAPH_EINVAL,
             "edge_neg_sample: num_users=%lld num_items=%lld B=%lld n_negs=%d", (long long)num_users, (long long)num_items,
             (long long)B, n_negs);
  RG_REQUIRE(B <= ((int64_t)1 << 38) / n_negs, RAGRAPH_EUNSUPPORTED, "edge_neg_sample: B * n_negs = %lld * %d slots",
             (long long)B, n_negs);
  if (B == 0) return RAGRAPH_OK;
  RG_REQUIRE(users && out, RAGRAPH_EINVAL, "edge_neg_sample: null users / out");
  hipStream_t st = as_stream(stream);
  if (check_users) {
    RG_REQUIRE(ws && ws_bytes >= 256, RAGRAPH_EWORKSPACE, "edge_neg_sample: workspace too small");
    int* bad = reinterpret_cast<int*>(ws);
    if (hipMemsetAsync(bad, 0, sizeof(int), st) != hipSuccess) {
      set_error("edge_neg_sample: memset failed");
      return RAGRAPH_EDEVICE;
    }
    const int64_t cb = cdiv(B, 256) < 4096 ? cdiv(B, 256) : 4096;
    hipLaunchKernelGGL(lp_index_check_kernel, dim3((unsigned)cb), dim3(256), 0, st, users, B, num_users, bad);
    RG_CHECK_LAUNCH("edge_neg_sample(check)");
    int bad_h = 0;
    const int rc = lp_read_flag(bad, st, &bad_h, "edge_neg_sample");
    if (rc != RAGRAPH_OK) return rc;
    RG_REQUIRE(!bad_h, RAGRAPH_EINVAL, "edge_neg_sample: a user id is outside [0, %lld)", (long long)num_users);
  }
  const int64_t total = B * (int64_t)n_negs;
  hipLaunchKernelGGL(edge_neg_sample_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, rowptr, items, num_items,
                     users, total, n_negs, seed, out);
  RG_CHECK_LAUNCH("edge_neg_sample");
  return RAGRAPH_OK;
}

extern "C" int ragraph_lp_compare_loss_fwd_f32(const float* h, int64_t n, int D, const int64_t* t, int S, float temperature,
                                               float* loss, float* L, float* coef, float* csim, float* hhat, float* nrm,
                                               void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(h && t && loss && L && coef && csim && hhat && nrm && ws, RAGRAPH_EINVAL, "lp_compare_loss: null pointer");
  RG_REQUIRE(n >= 1 && D >= 1 && S >= 2 && S <= LP_NEG_MAX + 1, RAGRAPH_EINVAL,
             "lp_compare_loss: n=%lld D=%d S=%d (need n >= 1, D >= 1, 2 <= S <= %d)", (long long)n, D, S, LP_NEG_MAX + 1);
  RG_REQUIRE(n <= INT_MAX, RAGRAPH_EUNSUPPORTED, "lp_compare_loss: n=%lld rows", (long long)n);
  RG_REQUIRE(temperature > 0.f, RAGRAPH_EINVAL, "lp_compare_loss: temperature must be > 0");
  RG_REQUIRE(ws_bytes >= 256, RAGRAPH_EWORKSPACE, "lp_compare_loss: workspace too small");
  hipStream_t st = as_stream(stream);
  int* bad = reinterpret_cast<int*>(ws);
  if (hipMemsetAsync(bad, 0, sizeof(int), st) != hipSuccess) {
    set_error("lp_compare_loss: memset failed");
    return RAGRAPH_EDEVICE;
  }
  const int64_t total = n * (int64_t)S;
  const int64_t cb = cdiv(total, 256) < 4096 ? cdiv(total, 256) : 4096;
  hipLaunchKernelGGL(lp_index_check_kernel, dim3((unsigned)cb), dim3(256), 0, st, t, total, n, bad);
  RG_CHECK_LAUNCH("lp_compare_loss(check)");
  int bad_h = 0;
  const int rc = lp_read_flag(bad, st, &bad_h, "lp_compare_loss");
  if (rc != RAGRAPH_OK) return rc;
  RG_REQUIRE(!bad_h, RAGRAPH_EINVAL, "lp_compare_loss: a sample id is outside [0, %lld)", (long long)n);
  hipLaunchKernelGGL(lp_normalize_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, st, h, n, D, hhat, nrm);
  RG_CHECK_LAUNCH("lp_compare_loss(normalize)");
  if (D % 4 == 0 && aligned16(hhat)) {
    hipLaunchKernelGGL(lp_loss_kernel<true>, dim3((unsigned)n), dim3(64), 0, st, hhat, t, n, D, S, temperature, L, coef, csim);
  } else {
    hipLaunchKernelGGL(lp_loss_kernel<false>, dim3((unsigned)n), dim3(64), 0, st, hhat, t, n, D, S, temperature, L, coef, csim);
  }
  RG_CHECK_LAUNCH("lp_compare_loss(rows)");
  hipLaunchKernelGGL(lp_mean_kernel, dim3(1), dim3(256), 0, st, L, n, loss);
  RG_CHECK_LAUNCH("lp_compare_loss(mean)");
  return RAGRAPH_OK;
}

extern "C" int ragraph_lp_combine_f32(const float* X, const float* h, const float* nrm, const float* beta, const float* go,
                                      float inv_rows, int64_t n, int D, float* out, void* stream) {
  RG_REQUIRE(X && h && nrm && beta && go && out, RAGRAPH_EINVAL, "lp_combine: null pointer");
  RG_REQUIRE(n >= 1 && D >= 1, RAGRAPH_EINVAL, "lp_combine: n=%lld D=%d", (long long)n, D);
  hipLaunchKernelGGL(lp_combine_kernel, dim3((unsigned)cdiv(n * (int64_t)D, 256)), dim3(256), 0, as_stream(stream),
                     X, h, nrm, beta, go, inv_rows, n, D, out);
  RG_CHECK_LAUNCH("lp_combine");
  return RAGRAPH_OK;
}
