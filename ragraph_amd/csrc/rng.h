// Counter-based randomness shared by the samplers (pretrain.hip) and the noise sources (noise.hip): a splitmix64 hash of
// (seed, row, draw).  No state: a value depends on its three keys only, so any lane can produce any draw.
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

}  // namespace ragraph
