// Structure-aware retrieval through the filter (ragraph_topk_mix_rerank_f32, ragraph_topk_rows_scatter_f32):
// RAGraph_node_fewshot/ragraph_utils/ToyGraphBase.py:47-65 from a canonical SEMANTIC candidate list.
//
// Given the canonical semantic top-k' of every query (scores = the fp32 fmaf chains of the contract: the bits of s_sem) the
// kernel computes, for each listed key, what the exact mixed call computes for it -- s_struct, the A-step fmaf chain from +0
// over the two normalised code rows, and fl(fl(s_struct * w_struct) + fl(s_sem * w_sem)) --, and selects the canonical top-k
// (score descending, index ascending) of those k' mixed scores.
// Proof.  A key outside the list has s_sem <= s_last, the list's k'-th score.  For w_sem > 0 rounding is monotone, so its
// mixed score is at most  bound = fl(fl(s_last * w_sem) + slack),  slack = mix_slack_of(w_struct) >= |fl(s_struct * w_struct)|
// (mix_slack.h: the value the fused mixed kernels prune with).  A row whose k-th best mixed score is STRICTLY greater than
// bound cannot be entered or tied by an outside key: its list is the exact call's, bit for bit, and its flag is 0.  Every other
// row -- also one with a non-finite score (every comparison with a NaN is false) or an index outside the bank -- has its flag
// set to 1 and is counted; the caller recomputes such rows with the exact call.  Nothing approximate is returned as proven.
//
// One wave per query, four queries per workgroup.  Lane l owns the candidates l and l + 64 (k' <= 128): it reads the key's A
// codes (4 A bytes of a table that is 6 % of the bank: L2 hits), runs the chain with the columns beyond A as zeros (a step
// fmaf(0, 0, acc) = acc: acc is never -0, the chain starts from +0) and the three-op mix.  The rank of a candidate is the
// number of candidates that beat it, counted against the k' candidates broadcast one by one from their lanes (readlane, a
// wave-uniform loop: no LDS, no sort); the candidate of rank r < k is stored to slot r, the one of rank k - 1 is compared with
// the bound.  No scratch, no LDS, no branch on data except around the final stores.  The count is one vector atomic add per
// unproven row; it decides no result (the flags say which rows are recomputed, the count only whether any is).
#include "common.h"
#include "mix_slack.h"
#include "topk_order.h"

namespace ragraph {

constexpr int RERANK_WAVES = 4;
constexpr int RERANK_MAX_A = 16;
constexpr int RERANK_MAX_LIST = 128;

struct RerankParams {
  const float* sem = nullptr;     // [B, kp] canonical semantic scores
  const int64_t* idx = nullptr;   // [B, kp]
  const float* Pq = nullptr;      // [B, A] normalised query codes
  const float* Pn = nullptr;      // [N, A] normalised bank codes
  int64_t B = 0, N = 0, idx_base = 0;
  int kp = 0, k = 0, A = 0;
  float w_struct = 0.f, w_sem = 0.f, slack = 0.f;
  float* out_s = nullptr;         // [B, k]
  int64_t* out_i = nullptr;
  int* unproven = nullptr;        // [B]
  int* count = nullptr;
};

__device__ __forceinline__ float lane_f32(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

__global__ void __launch_bounds__(RERANK_WAVES * 64) topk_mix_rerank_kernel(RerankParams p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * RERANK_WAVES + wave;
  if (row >= p.B) return;   // (wave-uniform)
  const float* __restrict__ sem = p.sem + row * p.kp;
  const int64_t* __restrict__ ix = p.idx + row * p.kp;
  const float* __restrict__ pq = p.Pq + row * p.A;

  // the lane's two candidates (an entry beyond the list re-reads the last one and is marked absent)
  const int e0 = min(lane, p.kp - 1), e1 = min(lane + 64, p.kp - 1);
  const bool have0 = lane < p.kp, have1 = lane + 64 < p.kp;
  const float s0 = sem[e0], s1 = sem[e1];
  const int64_t id0 = ix[e0], id1 = ix[e1];
  // (unsigned: a padding entry's INT64_MAX, or any index below idx_base, lands beyond N: never read, the row is unproven)
  const uint64_t u0 = (uint64_t)id0 - (uint64_t)p.idx_base, u1 = (uint64_t)id1 - (uint64_t)p.idx_base;
  const bool in0 = u0 < (uint64_t)p.N, in1 = u1 < (uint64_t)p.N;
  const int r0 = in0 ? (int)u0 : RG_IDX_NONE, r1 = in1 ? (int)u1 : RG_IDX_NONE;   // (N < 2^31 - 1: checked by the entry)
  const float* __restrict__ pn0 = p.Pn + (in0 ? (int64_t)u0 : 0) * p.A;
  const float* __restrict__ pn1 = p.Pn + (in1 ? (int64_t)u1 : 0) * p.A;

  float c0[RERANK_MAX_A], c1[RERANK_MAX_A], cq[RERANK_MAX_A];
#pragma unroll
  for (int a = 0; a < RERANK_MAX_A; ++a) {   // (A is wave-uniform: every load issued before the first is used)
    const bool on = a < p.A;
    c0[a] = on ? pn0[a] : 0.f;
    c1[a] = on ? pn1[a] : 0.f;
    cq[a] = on ? pq[a] : 0.f;
  }
  float t0 = 0.f, t1 = 0.f;
#pragma unroll
  for (int a = 0; a < RERANK_MAX_A; ++a) {
    t0 = fmaf(c0[a], cq[a], t0);
    t1 = fmaf(c1[a], cq[a], t1);
  }
  const float m0 = __fadd_rn(__fmul_rn(t0, p.w_struct), __fmul_rn(s0, p.w_sem));
  const float m1 = __fadd_rn(__fmul_rn(t1, p.w_struct), __fmul_rn(s1, p.w_sem));

  // rank by counting: how many of the k' candidates beat mine (canonical order; indices of a list are unique)
  int rank0 = 0, rank1 = 0;
  const int n_lo = min(p.kp, 64);
  for (int j = 0; j < n_lo; ++j) {
    const float sj = lane_f32(m0, j);
    const int ij = __builtin_amdgcn_readlane(r0, j);
    rank0 += cand_better(sj, ij, m0, r0) ? 1 : 0;
    rank1 += cand_better(sj, ij, m1, r1) ? 1 : 0;
  }
  for (int j = 64; j < p.kp; ++j) {
    const float sj = lane_f32(m1, j - 64);
    const int ij = __builtin_amdgcn_readlane(r1, j - 64);
    rank0 += cand_better(sj, ij, m0, r0) ? 1 : 0;
    rank1 += cand_better(sj, ij, m1, r1) ? 1 : 0;
  }

  // the proof: k-th best mixed score > bound, every score finite, every index inside the bank
  const float s_last = lane_f32(p.kp > 64 ? s1 : s0, (p.kp - 1) & 63);
  const float bound = __fadd_rn(__fmul_rn(s_last, p.w_sem), p.slack);
  const bool kth_above = (have0 && rank0 == p.k - 1 && m0 > bound) || (have1 && rank1 == p.k - 1 && m1 > bound);
  const bool bad = (have0 && !(in0 && fabsf(m0) <= 3.4028234e38f)) || (have1 && !(in1 && fabsf(m1) <= 3.4028234e38f));
  const bool proven = __ballot(kth_above) != 0ull && __ballot(bad) == 0ull;

  float* os = p.out_s + row * p.k;
  int64_t* oi = p.out_i + row * p.k;
  if (have0 && rank0 < p.k) {
    os[rank0] = m0;
    oi[rank0] = id0;
  }
  if (have1 && rank1 < p.k) {
    os[rank1] = m1;
    oi[rank1] = id1;
  }
  if (lane == 0) {
    p.unproven[row] = proven ? 0 : 1;
    if (!proven) __hip_atomic_fetch_add(p.count, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// out rows pos[m] <- rows m of (s, idx): the repaired rows of a call written back over its lists
__global__ void __launch_bounds__(256) topk_rows_scatter_kernel(const float* __restrict__ s, const int64_t* __restrict__ idx,
                                                                const int64_t* __restrict__ pos, int64_t M, int k, int64_t B,
                                                                float* __restrict__ out_s, int64_t* __restrict__ out_i) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= M * k) return;
  const int64_t m = t / k;
  const int j = (int)(t - m * k);
  const uint64_t r = (uint64_t)pos[m];
  if (r < (uint64_t)B) {   // (a position outside the lists writes nothing)
    out_s[(int64_t)r * k + j] = s[t];
    out_i[(int64_t)r * k + j] = idx[t];
  }
}

}  // namespace ragraph

using namespace ragraph;

extern "C" size_t ragraph_topk_mix_rerank_workspace_bytes(int64_t B, int A) {
  if (B < 1 || A < 1 || A > RERANK_MAX_A) return 0;
  return align_up((size_t)B * A * sizeof(float), 256);   // the normalised query codes
}

extern "C" int ragraph_topk_mix_rerank_f32(const float* sem_scores, const int64_t* sem_idx, int64_t B, int k_list,
                                           const float* Pq, const float* Pn, int64_t N, int A, float w_struct, float w_sem,
                                           int k, int64_t idx_base, float* out_scores, int64_t* out_idx, int* unproven,
                                           int* unproven_count, void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(sem_scores && sem_idx && Pq && Pn && out_scores && out_idx && unproven && unproven_count && ws, RAGRAPH_EINVAL,
             "topk_mix_rerank: null pointer");
  RG_REQUIRE(B >= 1 && B < ((int64_t)1 << 31) && N >= 1, RAGRAPH_EINVAL, "topk_mix_rerank: B=%lld N=%lld out of range",
             (long long)B, (long long)N);
  RG_REQUIRE(A >= 1 && A <= RERANK_MAX_A, RAGRAPH_EINVAL, "topk_mix_rerank: A=%d not in [1,%d]", A, RERANK_MAX_A);
  RG_REQUIRE(k_list >= 2 && k_list <= RERANK_MAX_LIST, RAGRAPH_EINVAL, "topk_mix_rerank: list length k'=%d outside 2..%d", k_list,
             RERANK_MAX_LIST);
  RG_REQUIRE(k >= 1 && k < k_list, RAGRAPH_EINVAL, "topk_mix_rerank: k=%d outside 1..k'-1=%d", k, k_list - 1);
  RG_REQUIRE(fabsf(w_struct) <= 3.0e38f, RAGRAPH_EINVAL, "topk_mix_rerank: w_struct is not finite");
  RG_REQUIRE(w_sem > 0.f && w_sem <= 3.0e38f, RAGRAPH_EINVAL,
             "topk_mix_rerank: w_sem=%g must be positive and finite (the bound needs a rising semantic term)", (double)w_sem);
  RG_REQUIRE(idx_base >= 0, RAGRAPH_EINVAL, "topk_mix_rerank: idx_base=%lld is negative", (long long)idx_base);
  RG_REQUIRE(N < (int64_t)INT_MAX, RAGRAPH_EUNSUPPORTED, "topk_mix_rerank: bank rows must fit int32");
  RG_REQUIRE((const void*)out_scores != (const void*)sem_scores && (const void*)out_idx != (const void*)sem_idx, RAGRAPH_EINVAL,
             "topk_mix_rerank: out must not alias the lists");
  const size_t need = ragraph_topk_mix_rerank_workspace_bytes(B, A);
  RG_REQUIRE(ws_bytes >= need, RAGRAPH_EWORKSPACE, "topk_mix_rerank: workspace %zu < %zu", ws_bytes, need);
  hipStream_t st = as_stream(stream);
  float* Pqn = static_cast<float*>(ws);
  const int rc = ragraph_normalize_rows_f32(Pq, B, A, Pqn, stream);   // (as ragraph_topk_cosine_mix_f32 normalises them)
  if (rc != RAGRAPH_OK) return rc;
  if (hipMemsetAsync(unproven_count, 0, sizeof(int), st) != hipSuccess) {
    set_error("topk_mix_rerank: clearing the count failed");
    return RAGRAPH_EDEVICE;
  }
  RerankParams p;
  p.sem = sem_scores;
  p.idx = sem_idx;
  p.Pq = Pqn;
  p.Pn = Pn;
  p.B = B;
  p.N = N;
  p.idx_base = idx_base;
  p.kp = k_list;
  p.k = k;
  p.A = A;
  p.w_struct = w_struct;
  p.w_sem = w_sem;
  p.slack = mix_slack_of(w_struct);
  p.out_s = out_scores;
  p.out_i = out_idx;
  p.unproven = unproven;
  p.count = unproven_count;
  hipLaunchKernelGGL(topk_mix_rerank_kernel, dim3((unsigned)cdiv(B, RERANK_WAVES)), dim3(RERANK_WAVES * 64), 0, st, p);
  RG_CHECK_LAUNCH("topk_mix_rerank");
  return RAGRAPH_OK;
}

extern "C" int ragraph_topk_rows_scatter_f32(const float* scores, const int64_t* idx, const int64_t* pos, int64_t M, int k,
                                             int64_t B, float* out_scores, int64_t* out_idx, void* stream) {
  RG_REQUIRE(out_scores && out_idx && ((scores && idx && pos) || M == 0), RAGRAPH_EINVAL, "topk_rows_scatter: null pointer");
  RG_REQUIRE(M >= 0 && B >= 1 && k >= 1 && M < ((int64_t)1 << 31) && k <= RERANK_MAX_LIST, RAGRAPH_EINVAL,
             "topk_rows_scatter: M=%lld B=%lld k=%d out of range", (long long)M, (long long)B, k);
  if (M == 0) return RAGRAPH_OK;
  hipLaunchKernelGGL(topk_rows_scatter_kernel, dim3((unsigned)cdiv(M * k, 256)), dim3(256), 0, as_stream(stream), scores, idx,
                     pos, M, k, B, out_scores, out_idx);
  RG_CHECK_LAUNCH("topk_rows_scatter");
  return RAGRAPH_OK;
}
