// Ordered top-k for 64 < k <= RAGRAPH_TOPK_ORDERED_MAX (csrc/topk_large.hip), shared with the cosine slab path.
#pragma once
#include "common.h"

namespace ragraph {

// Workspace of large_select over B rows of n elements (0 when every row fits one workgroup).
size_t large_select_ws_bytes(int64_t B, int64_t n, int64_t k);

// The canonical top-k (score descending, index ascending; NaN never selected) of every row of either a float matrix S
// [B, ld] (C == nullptr; the index of element e is idx_off + e) or a matrix of packed candidates C [B, ld]
// ((~order_key << 32) | index, ascending = canonical; ~0 = none).  The result goes either to
//   out_s / out_i [B, k] (out_i != nullptr): scores read from score_src[b * score_ld + index] when score_src is set (the
//   input's exact bits), decoded from the key otherwise; indices + idx_base; missing entries (-inf, INT64_MAX), or to
//   cand_out + b * cand_ld [k] as packed candidates, missing entries ~0.
int large_select(const float* S, const unsigned long long* C, int64_t B, int64_t n, int64_t ld, int64_t k,
                 unsigned idx_off, const float* score_src, int64_t score_ld, int64_t idx_base, unsigned long long* cand_out,
                 int64_t cand_ld, float* out_s, int64_t* out_i, void* ws, hipStream_t st);

}  // namespace ragraph
