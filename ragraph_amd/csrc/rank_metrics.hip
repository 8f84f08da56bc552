// Ranking metrics of the edge flavour's evaluation on the device: RAGraph_edge/utils/metrics.py:12-46 (recall, ndcg,
// precision), :60-80 (eval_batch) and :131-133 (result += batch_result / n_users).  Three launches, no atomics:
//   1. one thread per user: hits of its ranked list, then per k its recall, ndcg and hit count (fp64);
//   2. one thread per (batch, metric, k): the batch's users summed in user order (precision: / k after the sum);
//   3. one thread per (metric, k): batch_sum / n_users accumulated batch by batch.
// The only host read-back is the caller's 3 x nks doubles.
#include "common.h"

namespace ragraph {

constexpr int RANK_MAX_KS = 16;

struct RankKs {
  int k[RANK_MAX_KS];
};

__global__ void __launch_bounds__(256) rank_user_kernel(const int64_t* __restrict__ idx, int64_t U, int kmax,
                                                        const int64_t* __restrict__ grp, const int64_t* __restrict__ gt,
                                                        RankKs ks, int nks, double* __restrict__ per_user) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= U) return;
  const int64_t g0 = grp[u], g1 = grp[u + 1];
  const int64_t glen = g1 - g0;
  double* o = per_user + u * 3 * nks;
  for (int t = 0; t < nks; ++t) {
    const int k = ks.k[t];
    double hits = 0.0, dcg = 0.0, idcg = 0.0;
    for (int i = 0; i < k; ++i) {
      const int64_t it = idx[u * kmax + i];
      bool hit = false;
      for (int64_t e = g0; e < g1 && !hit; ++e) hit = gt[e] == it;  // `x in ground_true` (metrics.py:56)
      const double disc = 1.0 / log2((double)(i + 2));
      if (hit) {
        hits += 1.0;
        dcg += disc;
      }
      if (i < glen) idcg += disc;
    }
    if (idcg == 0.0) idcg = 1.0;                     // metrics.py:42
    o[t] = hits / (double)glen;                      // metrics.py:13-16 (recall_n = raw length)
    o[nks + t] = dcg / idcg;                         // metrics.py:30-46
    o[2 * nks + t] = hits;                           // metrics.py:18-22 (summed, then / k)
  }
}

__global__ void __launch_bounds__(256) rank_batch_kernel(const double* __restrict__ per_user, int64_t U, int64_t batch,
                                                         int64_t nbatch, RankKs ks, int nks, double* __restrict__ bsum) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int cols = 3 * nks;
  if (i >= nbatch * cols) return;
  const int64_t b = i / cols;
  const int c = (int)(i % cols);
  const int64_t u1 = (b + 1) * batch < U ? (b + 1) * batch : U;
  double s = 0.0;
  for (int64_t u = b * batch; u < u1; ++u) s += per_user[u * cols + c];
  if (c >= 2 * nks) s = s / (double)ks.k[c - 2 * nks];
  bsum[i] = s;
}

__global__ void __launch_bounds__(64) rank_total_kernel(const double* __restrict__ bsum, int64_t U, int64_t nbatch,
                                                        int cols, double* __restrict__ out) {
  const int c = threadIdx.x;
  if (c >= cols) return;
  double acc = 0.0;
  for (int64_t b = 0; b < nbatch; ++b) acc += bsum[b * cols + c] / (double)U;
  // out is [metric][k]: column c = metric * nks + t already
  out[c] = acc;
}

}  // namespace ragraph

using namespace ragraph;

extern "C" size_t ragraph_rank_metrics_workspace_bytes(int64_t U, int nks, int64_t batch) {
  if (U < 1 || nks < 1 || nks > RANK_MAX_KS || batch < 1) return 0;
  const int64_t nbatch = cdiv(U, batch);
  return align_up((size_t)U * 3 * nks * sizeof(double), 256) + align_up((size_t)nbatch * 3 * nks * sizeof(double), 256);
}

extern "C" int ragraph_rank_metrics_f64(const int64_t* idx, int64_t U, int kmax, const int64_t* gt_rowptr,
                                        const int64_t* gt_items, const int* ks, int nks, int64_t batch, double* out,
                                        void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(idx && gt_rowptr && ks && out && ws, RAGRAPH_EINVAL, "rank_metrics: null pointer");
  RG_REQUIRE(U >= 1 && kmax >= 1 && batch >= 1, RAGRAPH_EINVAL, "rank_metrics: U=%lld kmax=%d batch=%lld", (long long)U,
             kmax, (long long)batch);
  RG_REQUIRE(nks >= 1 && nks <= RANK_MAX_KS, RAGRAPH_EINVAL, "rank_metrics: nks=%d not in [1, %d]", nks, RANK_MAX_KS);
  RankKs kk;
  for (int t = 0; t < RANK_MAX_KS; ++t) kk.k[t] = 0;
  for (int t = 0; t < nks; ++t) {
    RG_REQUIRE(ks[t] >= 1 && ks[t] <= kmax, RAGRAPH_EINVAL, "rank_metrics: k=%d not in [1, %d]", ks[t], kmax);
    kk.k[t] = ks[t];
  }
  RG_REQUIRE(ws_bytes >= ragraph_rank_metrics_workspace_bytes(U, nks, batch), RAGRAPH_EWORKSPACE,
             "rank_metrics: workspace too small");
  hipStream_t st = as_stream(stream);
  const int64_t nbatch = cdiv(U, batch);
  double* per_user = reinterpret_cast<double*>(ws);
  double* bsum = reinterpret_cast<double*>(static_cast<char*>(ws) + align_up((size_t)U * 3 * nks * sizeof(double), 256));
  hipLaunchKernelGGL(rank_user_kernel, dim3((unsigned)cdiv(U, 256)), dim3(256), 0, st, idx, U, kmax, gt_rowptr, gt_items,
                     kk, nks, per_user);
  RG_CHECK_LAUNCH("rank_metrics(users)");
  hipLaunchKernelGGL(rank_batch_kernel, dim3((unsigned)cdiv(nbatch * 3 * nks, 256)), dim3(256), 0, st, per_user, U, batch,
                     nbatch, kk, nks, bsum);
  RG_CHECK_LAUNCH("rank_metrics(batches)");
  hipLaunchKernelGGL(rank_total_kernel, dim3(1), dim3(64), 0, st, bsum, U, nbatch, 3 * nks, out);
  RG_CHECK_LAUNCH("rank_metrics(total)");
  return RAGRAPH_OK;
}
