// The slack of the structure-aware bound, shared by the fused mixed kernels (topk_cosine.hip) and the rerank of filtered
// candidate lists (topk_mix_rerank.hip): one value, so a proof made by either is a proof for both.
#pragma once
#include <math.h>

namespace ragraph {

// >= |fl(s_struct * w_struct)| for every pair of unit-or-zero code rows:
// |s_struct| <= |a||b| (1 + A 2^-23) for rows normalised to within a few ulp of 1: 2^-10 covers it many times over
static inline float mix_slack_of(float w_struct) {
  return nextafterf((float)(fabs((double)w_struct) * (1.0 + 1.0 / 1024)), __builtin_huge_valf());
}

}  // namespace ragraph
