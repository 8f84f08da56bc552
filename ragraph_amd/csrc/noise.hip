// Noisy fine-tuning with the noise drawn on the device, keyed by the query's row id (finetune-noise.py of every flavour):
//   * ragraph_noise_rows_i64: the noise_retrieve_num random bank rows per query (RAGraph_node/ragraph_utils/ToyGraphBase.py:
//     73-79, RAGraph_node_fewshot/ragraph_utils/ToyGraphBase.py:70-76, RAGraph_edge/modules/RAGraph.py:316-318), one lane per
//     slot: out[b, j] = lp_below(lp_draw(seed, row_id(b), j), N).
//   * ragraph_gather_reduce_noisy_f32: sum / mean over the top-k rows AND those noise rows (RAGraph_node/RAGraph.py:48-49,
//     RAGraph_edge/modules/RAGraph.py:314-321) without an index matrix for the noise: gather_reduce_kernel (rowops.hip) over a
//     list of k + m entries whose last m ids the lanes compute instead of loading.
//   * ragraph_add_normal_noise_f32: the Gaussian noise on the gathered embeddings of the graph flavours
//     (RAGraph_graph/ragraph_utils/ToyGraphBase.py:131-134, RAGraph_graph_fewshot/ragraph_utils/ToyGraphBase.py:135-138):
//     out = X + std * z, z by Box-Muller on one lp_draw word per pair of columns.
// The reference draws all of these from torch's CPU generator; the streams here are other streams of the same laws.  A value
// depends on (seed[0], row id, draw) only: a row gets the same noise whichever rows are computed beside it, no draw is made
// for a row nobody asked for, and nothing passes through the host (seed[0] is read from device memory), so a step that uses
// these entries can be captured in a HIP graph.
#include "common.h"
#include "rng.h"

namespace ragraph {

// ---- noise rows: one lane per slot ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) noise_rows_kernel(const int64_t* __restrict__ seed_p, const int64_t* __restrict__ row_ids,
                                                         int64_t row_base, int64_t B, int m, uint64_t N,
                                                         int64_t* __restrict__ out, int64_t out_stride) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= B * m) return;
  const int64_t b = s / m;
  const int64_t j = s - b * m;
  out[b * out_stride + j] = (int64_t)lp_below(lp_draw((uint64_t)seed_p[0], noise_row_id(row_ids, row_base, b), (uint64_t)j), N);
}

// ---- gather-reduce over k listed rows and m noise rows ------------------------------------------------------------------
// gather_reduce_kernel's shape (rowops.hip): the wave holds a block of 64 entries of the row's list in
// its lanes BEFORE any row load goes out -- lane u the entry jb + u: loaded from idx while jb + u < k, hashed from
// (seed, row id, jb + u - k) behind that -- and hands them out through v_readlane, so the loads of 8 entries go out back to
// back.  Same adds in the same order as gather_reduce_kernel over cat(idx, noise rows): the same bits.
template <bool VEC4>
__global__ void __launch_bounds__(256) gather_reduce_noisy_kernel(const float* __restrict__ V, int D, const float* __restrict__ L,
                                                                  int C, int64_t N, const int64_t* __restrict__ idx, int64_t B,
                                                                  int k, int64_t base, float v_scale,
                                                                  const int64_t* __restrict__ seed_p,
                                                                  const int64_t* __restrict__ row_ids, int64_t row_base, int m,
                                                                  uint64_t noise_n, float* __restrict__ sumV,
                                                                  float* __restrict__ meanL, const float* __restrict__ mixA,
                                                                  float wa, float wb) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t* ib = idx + b * k;
  const int kt = k + m;
  const uint64_t seed = (uint64_t)seed_p[0];
  const uint64_t rid = noise_row_id(row_ids, row_base, b);
  auto row_of = [&](int64_t mine, int u) {   // entry u of the block whose rows the lanes hold (u wave-uniform); -1: not mine
    return ((int64_t)__builtin_amdgcn_readlane((int)(mine >> 32), u) << 32) | (unsigned)__builtin_amdgcn_readlane((int)mine, u);
  };
  auto load_block = [&](int jb) {            // lane u: row of entry jb + u inside this shard, or -1
    int64_t r = -1;
    const int j = jb + lane;
    if (j < kt) {
      r = (j < k ? ib[j] : (int64_t)lp_below(lp_draw(seed, rid, (uint64_t)(j - k)), noise_n)) - base;
      if (r < 0 || r >= N) r = -1;
    }
    return r;
  };
  if (VEC4) {
    const int D4 = D >> 2;
    for (int c = lane; c < ((D4 + 63) / 64) * 64; c += 64) {   // (uniform trip count: readlanes inside)
      const bool colok = c < D4;
      const int cc = colok ? c : 0;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int jb = 0; jb < kt && N > 0; jb += 64) {   // (an empty shard has no row 0 to read)
        const int64_t mine = load_block(jb);
        const int nb = kt - jb < 64 ? kt - jb : 64;
        for (int j0 = 0; j0 < nb; j0 += 8) {
          float4 v[8];
          bool ok[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int64_t r = j0 + u < nb ? row_of(mine, j0 + u) : -1;
            ok[u] = r >= 0;
            v[u] = reinterpret_cast<const float4*>(V + (ok[u] ? r : 0) * D)[cc];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (j0 + u < nb) {
              const float4 x = ok[u] ? v[u] : make_float4(0.f, 0.f, 0.f, 0.f);
              acc.x = __fadd_rn(acc.x, x.x); acc.y = __fadd_rn(acc.y, x.y);
              acc.z = __fadd_rn(acc.z, x.z); acc.w = __fadd_rn(acc.w, x.w);
            }
          }
        }
      }
      if (v_scale != 1.f) {
        acc.x = __fmul_rn(acc.x, v_scale); acc.y = __fmul_rn(acc.y, v_scale);
        acc.z = __fmul_rn(acc.z, v_scale); acc.w = __fmul_rn(acc.w, v_scale);
      }
      if (mixA && colok) {
        const float4 a = reinterpret_cast<const float4*>(mixA + b * D)[c];
        acc.x = __fadd_rn(__fmul_rn(a.x, wa), __fmul_rn(acc.x, wb)); acc.y = __fadd_rn(__fmul_rn(a.y, wa), __fmul_rn(acc.y, wb));
        acc.z = __fadd_rn(__fmul_rn(a.z, wa), __fmul_rn(acc.z, wb)); acc.w = __fadd_rn(__fmul_rn(a.w, wa), __fmul_rn(acc.w, wb));
      }
      if (colok) reinterpret_cast<float4*>(sumV + b * D)[c] = acc;
    }
  } else {
    for (int e = lane; e < D; e += 64) {
      float acc = 0.f;
      for (int jx = 0; jx < kt; ++jx) {
        const int64_t r = (jx < k ? ib[jx] : (int64_t)lp_below(lp_draw(seed, rid, (uint64_t)(jx - k)), noise_n)) - base;
        if (r >= 0 && r < N) acc = __fadd_rn(acc, V[r * D + e]);
      }
      acc = (v_scale == 1.f) ? acc : __fmul_rn(acc, v_scale);
      sumV[b * D + e] = mixA ? __fadd_rn(__fmul_rn(mixA[b * D + e], wa), __fmul_rn(acc, wb)) : acc;
    }
  }
  if (L && meanL) {
    for (int c = lane; c < ((C + 63) / 64) * 64; c += 64) {
      const bool colok = c < C;
      float acc = 0.f;
      for (int jb = 0; jb < kt; jb += 64) {
        const int64_t mine = load_block(jb);
        const int nb = kt - jb < 64 ? kt - jb : 64;
        for (int jx = 0; jx < nb; ++jx) {
          const int64_t r = row_of(mine, jx);
          if (r >= 0 && colok) acc = __fadd_rn(acc, L[r * C + c]);
        }
      }
      if (colok) meanL[b * C + c] = acc / (float)kt;
    }
  }
}

// ---- Gaussian noise on gathered embeddings ----------------------------------------------------------------------------------
// One lane per pair of columns of X [B, J, D]: pair p of row (b, j) is draw j * ceil(D / 2) + p of row id(b).  out may be X.
__global__ void __launch_bounds__(256) add_normal_noise_kernel(const float* X, int64_t B, int64_t J, int D, float std,
                                                               const int64_t* __restrict__ seed_p,
                                                               const int64_t* __restrict__ row_ids, int64_t row_base, float* out) {
  const int64_t P = (D + 1) >> 1;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * J * P) return;
  const int64_t b = i / (J * P);
  const int64_t jp = i - b * (J * P);          // j * P + p: the draw
  const int64_t j = jp / P;
  const int p = (int)(jp - j * P);
  float z0, z1;
  normal_pair((uint64_t)seed_p[0], noise_row_id(row_ids, row_base, b), (uint64_t)jp, z0, z1);
  const int64_t o = (b * J + j) * D + 2 * p;
  const bool two = 2 * p + 1 < D;
  const float x0 = X ? X[o] : 0.f;
  const float x1 = (X && two) ? X[o + 1] : 0.f;
  out[o] = __fadd_rn(x0, __fmul_rn(std, z0));
  if (two) out[o + 1] = __fadd_rn(x1, __fmul_rn(std, z1));
}

}  // namespace ragraph

using namespace ragraph;

extern "C" int ragraph_noise_rows_i64(const int64_t* seed, const int64_t* row_ids, int64_t row_base, int64_t B, int m,
                                      int64_t N, int64_t* out, int64_t out_stride, void* stream) {
  RG_REQUIRE(seed, RAGRAPH_EINVAL, "noise_rows: null seed");
  RG_REQUIRE(N >= 1 && m >= 1 && B >= 0, RAGRAPH_EINVAL, "noise_rows: bad shape (B=%lld, m=%d, N=%lld)", (long long)B, m,
             (long long)N);
  RG_REQUIRE(out_stride >= m, RAGRAPH_EINVAL, "noise_rows: out_stride=%lld < m=%d", (long long)out_stride, m);
  RG_REQUIRE(B <= (INT64_MAX >> 8) / m, RAGRAPH_EINVAL, "noise_rows: B * m too large");
  if (B == 0) return RAGRAPH_OK;
  RG_REQUIRE(out, RAGRAPH_EINVAL, "noise_rows: null pointer");
  const int64_t blocks = cdiv(B * m, 256);
  RG_REQUIRE(blocks <= 0x7FFFFFFFll, RAGRAPH_EINVAL, "noise_rows: B * m too large");
  hipLaunchKernelGGL(noise_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), seed, row_ids, row_base, B, m,
                     (uint64_t)N, out, out_stride);
  RG_CHECK_LAUNCH("noise_rows");
  return RAGRAPH_OK;
}

extern "C" int ragraph_gather_reduce_noisy_f32(const float* V, int D, const float* L, int C, int64_t N, const int64_t* idx,
                                               int64_t B, int k, int64_t idx_base, float v_scale, const int64_t* seed,
                                               const int64_t* row_ids, int64_t row_base, int m, int64_t noise_n, const float* A,
                                               float wa, float wb, float* out, float* mean_L, void* stream) {
  RG_REQUIRE(seed, RAGRAPH_EINVAL, "gather_reduce_noisy: null seed");
  RG_REQUIRE(V && idx && out, RAGRAPH_EINVAL, "gather_reduce_noisy: null pointer");
  RG_REQUIRE(D >= 1 && k >= 1 && B >= 0 && N >= 0, RAGRAPH_EINVAL, "gather_reduce_noisy: bad shape");
  RG_REQUIRE(m >= 1 && m <= INT_MAX - k && noise_n >= 1, RAGRAPH_EINVAL, "gather_reduce_noisy: m=%d, noise_n=%lld", m,
             (long long)noise_n);
  RG_REQUIRE((L == nullptr) == (mean_L == nullptr), RAGRAPH_EINVAL, "gather_reduce_noisy: L and mean_L go together");
  RG_REQUIRE(!L || C >= 1, RAGRAPH_EINVAL, "gather_reduce_noisy: C=%d", C);
  RG_REQUIRE(!A || A != out, RAGRAPH_EINVAL, "gather_reduce_noisy: out must not alias A");
  if (B == 0) return RAGRAPH_OK;
  const bool vec = (D % 4 == 0) && aligned16(V) && aligned16(out) && (!A || aligned16(A));
  if (vec)
    hipLaunchKernelGGL(gather_reduce_noisy_kernel<true>, dim3((unsigned)cdiv(B, 4)), dim3(256), 0, as_stream(stream), V, D, L, C,
                       N, idx, B, k, idx_base, v_scale, seed, row_ids, row_base, m, (uint64_t)noise_n, out, mean_L, A, wa, wb);
  else
    hipLaunchKernelGGL(gather_reduce_noisy_kernel<false>, dim3((unsigned)cdiv(B, 4)), dim3(256), 0, as_stream(stream), V, D, L, C,
                       N, idx, B, k, idx_base, v_scale, seed, row_ids, row_base, m, (uint64_t)noise_n, out, mean_L, A, wa, wb);
  RG_CHECK_LAUNCH("gather_reduce_noisy");
  return RAGRAPH_OK;
}

extern "C" int ragraph_add_normal_noise_f32(const float* X, int64_t B, int64_t J, int D, float std, const int64_t* seed,
                                            const int64_t* row_ids, int64_t row_base, float* out, void* stream) {
  RG_REQUIRE(seed, RAGRAPH_EINVAL, "add_normal_noise: null seed");
  RG_REQUIRE(B >= 0 && J >= 1 && D >= 1, RAGRAPH_EINVAL, "add_normal_noise: bad shape (B=%lld, J=%lld, D=%d)", (long long)B,
             (long long)J, D);
  const int64_t P = ((int64_t)D + 1) >> 1;
  RG_REQUIRE(J <= (INT64_MAX >> 8) / P && (B == 0 || J * P <= (INT64_MAX >> 8) / B), RAGRAPH_EINVAL,
             "add_normal_noise: B * J * D too large");
  if (B == 0) return RAGRAPH_OK;
  RG_REQUIRE(out, RAGRAPH_EINVAL, "add_normal_noise: null pointer");
  const int64_t blocks = cdiv(B * J * P, 256);
  RG_REQUIRE(blocks <= 0x7FFFFFFFll, RAGRAPH_EINVAL, "add_normal_noise: B * J * D too large");
  hipLaunchKernelGGL(add_normal_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), X, B, J, D, std, seed,
                     row_ids, row_base, out);
  RG_CHECK_LAUNCH("add_normal_noise");
  return RAGRAPH_OK;
}
