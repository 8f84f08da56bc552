// Counter-based randomness shared by the samplers (pretrain.hip), the noise sources (noise.hip) and the stochastic half of bank
// construction (bank.hip): a splitmix64 hash of (seed, row, draw).  No state: a value depends on its three keys only, so any lane can produce any draw.
#pragma once
#include "common.h"

namespace ragraph {

// ---- randomness: splitmix64 on (seed, row, draw) ----------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t lp_draw(uint64_t seed, uint64_t row, uint64_t draw) {
  return splitmix64(splitmix64(seed ^ splitmix64(row)) + draw);
}
// uniform in [0, m) (the high half of the 128-bit product; bias < m / 2^64)
__device__ __forceinline__ uint64_t lp_below(uint64_t h, uint64_t m) { return __umul64hi(h, m); }

// uniform in [0, 1) with 53 bits: exact in a double.  An event of probability t (a float) happens iff u53(w) < (double)t -- a
// 24-bit uniform cannot represent probabilities near 2e-9 (the edge flavour's node drop)
__device__ __forceinline__ double u53(uint64_t w) { return (double)(w >> 11) * 0x1p-53; }
__device__ __forceinline__ bool lp_event(uint64_t w, float t) { return u53(w) < (double)t; }

// the id that keys a row's draws: the caller's row_ids[b], or row_base + b without them
__device__ __forceinline__ uint64_t noise_row_id(const int64_t* __restrict__ row_ids, int64_t row_base, int64_t b) {
  return (uint64_t)(row_ids ? row_ids[b] : row_base + b);
}

// ---- Gaussian draws ----------------------------------------------------------------------------------------------------
// The two standard normals of draw `draw` of a row: Box-Muller on the two 24-bit halves of the word's high 48 bits.
// u1 = (h + 1) / 2^24 lies in (0, 1], so r <= sqrt(48 ln 2) ~ 5.77; u2 = l / 2^24 in [0, 1).  Every product is explicit.
__device__ __forceinline__ void normal_pair(uint64_t seed, uint64_t row, uint64_t draw, float& z0, float& z1) {
  const uint64_t w = lp_draw(seed, row, draw);
  const float u1 = __fmul_rn((float)((uint32_t)(w >> 40) + 1u), 0x1p-24f);
  const float u2 = __fmul_rn((float)((uint32_t)(w >> 16) & 0xFFFFFFu), 0x1p-24f);
  const float r = sqrtf(__fmul_rn(-2.f, logf(u1)));
  float s, c;
  sincospif(__fmul_rn(2.f, u2), &s, &c);
  z0 = __fmul_rn(r, c);
  z1 = __fmul_rn(r, s);
}

}  // namespace ragraph
