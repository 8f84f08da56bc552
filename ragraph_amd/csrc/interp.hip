// The interpolative update of the edge flavour's staged fine-tuning (RAGraph_edge/finetune_rag.py:63-86):
//   F.normalize(torch.sum(torch.stack(tables) * w[:, None, None], dim=0), dim=1)
// in one pass: S tables read once, one table written, nothing allocated.  HBM-bound, (S + 1) * n * D * 4 bytes.
//
// The tables' pointers and the weights travel in the kernel's arguments (InterpArgs, by value): no pointer table on the
// device, no copy, no synchronisation.  S is a template parameter, so a lane's S loads of a chunk go out back to back
// before the first multiply needs one.
//
// Mix (never contracted): acc = T_0 * w_0; acc = acc + T_s * w_s for s = 1..S-1 -- the bits of ragraph_axpby_f32(T_0, w_0,
// T_1, w_1) followed by ragraph_axpby_f32(acc, 1, T_s, w_s).  Norm: the tree of ragraph_normalize_rows_f32 (float4 chunk c of a
// row belongs to lane c mod 64, squares by fmaf in element order, butterfly 32..1) on the mixed row.
//   rows of <= 16 chunks (D <= 64): a 16-lane group owns a row, one chunk per lane, four rows per wave.  Lanes 16..63 of the
//       documented tree would hold +0 partials and p + 0 = p, so the levels 8, 4, 2, 1 inside the group give its bits.
//   rows of <= 256 chunks (D <= 1024): one wave per row, a lane keeps the mix of its (up to four) chunks in registers.
//   longer rows: one wave per row mixes twice -- once for the norm, once for the quotient -- and keeps nothing.
#include "common.h"

namespace ragraph {

struct InterpArgs {
  const float* t[RAGRAPH_INTERP_MAX_TABLES];
  float w[RAGRAPH_INTERP_MAX_TABLES];
};

// the mix of chunk c of a row (elements 4c .. 4c+3; elements at or beyond D come back as +0)
template <int S, bool VEC4>
__device__ __forceinline__ float4 interp_mix_chunk(const InterpArgs& a, int64_t base, int c, int D) {
  float4 v[S];
  if (VEC4) {
#pragma unroll
    for (int s = 0; s < S; ++s) v[s] = reinterpret_cast<const float4*>(a.t[s] + base)[c];
  } else {
    const int e = 4 * c;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const float* x = a.t[s] + base;
      v[s].x = x[e];   // (c < nchunk: e < D)
      v[s].y = e + 1 < D ? x[e + 1] : 0.f;
      v[s].z = e + 2 < D ? x[e + 2] : 0.f;
      v[s].w = e + 3 < D ? x[e + 3] : 0.f;
    }
  }
  float4 m;
  m.x = __fmul_rn(v[0].x, a.w[0]); m.y = __fmul_rn(v[0].y, a.w[0]);
  m.z = __fmul_rn(v[0].z, a.w[0]); m.w = __fmul_rn(v[0].w, a.w[0]);
#pragma unroll
  for (int s = 1; s < S; ++s) {
    m.x = __fadd_rn(m.x, __fmul_rn(v[s].x, a.w[s])); m.y = __fadd_rn(m.y, __fmul_rn(v[s].y, a.w[s]));
    m.z = __fadd_rn(m.z, __fmul_rn(v[s].z, a.w[s])); m.w = __fadd_rn(m.w, __fmul_rn(v[s].w, a.w[s]));
  }
  if (!VEC4) {   // a padding element takes no part in the norm, whatever 0 * w is
    const int e = 4 * c;
    if (e + 1 >= D) m.y = 0.f;
    if (e + 2 >= D) m.z = 0.f;
    if (e + 3 >= D) m.w = 0.f;
  }
  return m;
}

__device__ __forceinline__ float interp_squares(float4 m, float p) {
  p = fmaf(m.x, m.x, p);
  p = fmaf(m.y, m.y, p);
  p = fmaf(m.z, m.z, p);
  p = fmaf(m.w, m.w, p);
  return p;
}

template <bool VEC4>
__device__ __forceinline__ void interp_store_chunk(float* __restrict__ o, int c, int D, float4 m, float d) {
  m.x = m.x / d; m.y = m.y / d; m.z = m.z / d; m.w = m.w / d;
  if (VEC4) {
    reinterpret_cast<float4*>(o)[c] = m;
  } else {
    const int e = 4 * c;
    o[e] = m.x;
    if (e + 1 < D) o[e + 1] = m.y;
    if (e + 2 < D) o[e + 2] = m.z;
    if (e + 3 < D) o[e + 3] = m.w;
  }
}

// rows of at most 16 chunks: sixteen rows per workgroup, a 16-lane group (one DPP row) each
template <int S, bool VEC4>
__global__ void __launch_bounds__(256) interp_group_kernel(InterpArgs a, int64_t n, int D, float* __restrict__ out) {
  const int c = threadIdx.x & 15;
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (row >= n) return;   // (a whole group leaves: the exchanges below stay inside a group)
  const int nchunk = (D + 3) >> 2;
  const bool mine = c < nchunk;
  float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
  if (mine) m = interp_mix_chunk<S, VEC4>(a, row * D, c, D);
  float p = interp_squares(m, 0.f);
  p = __fadd_rn(p, dpp_f32<DPP_ROW_ROR8>(0.f, p));   // the levels 8, 4, 2, 1 of wave_sum_fixed_tree
  p = __fadd_rn(p, dpp_f32<DPP_ROW_ROR4>(0.f, p));
  p = __fadd_rn(p, dpp_f32<DPP_QUAD_XOR2>(0.f, p));
  p = __fadd_rn(p, dpp_f32<DPP_QUAD_XOR1>(0.f, p));
  const float d = fmaxf(sqrtf(p), 1e-12f);
  if (mine) interp_store_chunk<VEC4>(out + row * D, c, D, m, d);
}

// one wave per row.  KEEP: the lane holds the mix of its chunks lane, lane + 64, lane + 128, lane + 192 (nchunk <= 256);
// otherwise the row is mixed a second time for the quotient.
template <int S, bool VEC4, bool KEEP>
__global__ void __launch_bounds__(256) interp_wave_kernel(InterpArgs a, int64_t n, int D, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int nchunk = (D + 3) >> 2;
  const int64_t base = row * D;
  float p = 0.f;
  if (KEEP) {
    float4 m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = lane + 64 * j;
      m[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < nchunk) m[j] = interp_mix_chunk<S, VEC4>(a, base, c, D);
      p = interp_squares(m[j], p);   // (a chunk beyond the row adds +0: p is never -0)
    }
    p = wave_sum_fixed_tree(p);
    const float d = fmaxf(sqrtf(p), 1e-12f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = lane + 64 * j;
      if (c < nchunk) interp_store_chunk<VEC4>(out + base, c, D, m[j], d);
    }
  } else {
    for (int c = lane; c < nchunk; c += 64) p = interp_squares(interp_mix_chunk<S, VEC4>(a, base, c, D), p);
    p = wave_sum_fixed_tree(p);
    const float d = fmaxf(sqrtf(p), 1e-12f);
    for (int c = lane; c < nchunk; c += 64) interp_store_chunk<VEC4>(out + base, c, D, interp_mix_chunk<S, VEC4>(a, base, c, D), d);
  }
}

template <int S>
static void interp_launch(const InterpArgs& a, int64_t n, int D, bool vec, float* out, hipStream_t st) {
  const int nchunk = (D + 3) >> 2;
  if (nchunk <= 16) {
    const dim3 grid((unsigned)cdiv(n, 16));
    if (vec) hipLaunchKernelGGL((interp_group_kernel<S, true>), grid, dim3(256), 0, st, a, n, D, out);
    else hipLaunchKernelGGL((interp_group_kernel<S, false>), grid, dim3(256), 0, st, a, n, D, out);
    return;
  }
  const dim3 grid((unsigned)cdiv(n, 4));
  if (nchunk <= 256) {
    if (vec) hipLaunchKernelGGL((interp_wave_kernel<S, true, true>), grid, dim3(256), 0, st, a, n, D, out);
    else hipLaunchKernelGGL((interp_wave_kernel<S, false, true>), grid, dim3(256), 0, st, a, n, D, out);
  } else {
    if (vec) hipLaunchKernelGGL((interp_wave_kernel<S, true, false>), grid, dim3(256), 0, st, a, n, D, out);
    else hipLaunchKernelGGL((interp_wave_kernel<S, false, false>), grid, dim3(256), 0, st, a, n, D, out);
  }
}

}  // namespace ragraph

using namespace ragraph;

extern "C" int ragraph_interp_normalize_f32(const float* const* tables, const float* weights, int S, int64_t n, int D,
                                            float* out, void* stream) {
  RG_REQUIRE(tables && weights && out, RAGRAPH_EINVAL, "interp_normalize: null pointer");
  RG_REQUIRE(S >= 1 && S <= RAGRAPH_INTERP_MAX_TABLES, RAGRAPH_EINVAL, "interp_normalize: S=%d not in [1,%d]", S,
             RAGRAPH_INTERP_MAX_TABLES);
  RG_REQUIRE(n >= 0 && D >= 1, RAGRAPH_EINVAL, "interp_normalize: n=%lld D=%d", (long long)n, D);
  InterpArgs a;
  bool vec = (D % 4 == 0) && aligned16(out);
  for (int s = 0; s < RAGRAPH_INTERP_MAX_TABLES; ++s) {
    a.t[s] = s < S ? tables[s] : nullptr;
    a.w[s] = s < S ? weights[s] : 0.f;
    if (s >= S) continue;
    RG_REQUIRE(a.t[s], RAGRAPH_EINVAL, "interp_normalize: table %d is a null pointer", s);
    RG_REQUIRE(a.t[s] != out, RAGRAPH_EINVAL, "interp_normalize: out must not alias table %d", s);
    vec = vec && aligned16(a.t[s]);
  }
  if (n == 0) return RAGRAPH_OK;
  RG_REQUIRE(cdiv(n, 4) <= (int64_t)INT_MAX, RAGRAPH_EUNSUPPORTED, "interp_normalize: n=%lld rows in one call", (long long)n);
  hipStream_t st = as_stream(stream);
  switch (S) {
    case 1: interp_launch<1>(a, n, D, vec, out, st); break;
    case 2: interp_launch<2>(a, n, D, vec, out, st); break;
    case 3: interp_launch<3>(a, n, D, vec, out, st); break;
    case 4: interp_launch<4>(a, n, D, vec, out, st); break;
    case 5: interp_launch<5>(a, n, D, vec, out, st); break;
    case 6: interp_launch<6>(a, n, D, vec, out, st); break;
    case 7: interp_launch<7>(a, n, D, vec, out, st); break;
    default: interp_launch<8>(a, n, D, vec, out, st); break;
  }
  RG_CHECK_LAUNCH("interp_normalize");
  return RAGRAPH_OK;
}
