// Graph ingestion on the device: edge lists -> the hot path's input formats.
//
//   csr_sym_normalized   D^-1/2 (A + I) D^-1/2 as CSR                  RAGraph_node/ragraph_utils/utility.py:19-26 (normalize_adj),
//                                                                       :45-66 (coo_matrix of ones -> dense: duplicate edges SUM;
//                                                                       + eye; torch.FloatTensor)
//   binorm_edges         bipartite D^-1/2 A D^-1/2 as a sorted edge list RAGraph_edge/modules/base_model.py:34-52 (_make_binorm_adj:
//                                                                       binarised, symmetric, .tocoo() order), edge times of
//                                                                       utils/dataloader.py:94,108-113 (the LAST time of a
//                                                                       repeated (user, item) pair wins: dict assignment)
//
// The reference builds both on the host (a numpy row_stack loop that densifies the block-diagonal adjacency -- quadratic
// in the batch's node count and the reason a 100k-node graph cannot be ingested at all -- and Python loops over every
// edge).  Here: 64-bit keys, the library's own stable radix sort and prefix sums (csrc/sortscan.hip), run-length heads, a prefix
// sum, and kernels that count multiplicities, accumulate integer degrees (exact whatever the atomic order) and emit the
// normalised values in double precision cast to fp32 last -- as scipy (float64) followed by torch.FloatTensor does.
#include "sortscan.h"

namespace ragraph {

__global__ void __launch_bounds__(256) sym_keys_kernel(const int64_t* __restrict__ row, const int64_t* __restrict__ col,
                                                       int64_t E, int64_t n, uint64_t* __restrict__ keys) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < E) keys[e] = (uint64_t)col[e] * (uint64_t)n + (uint64_t)row[e];  // normalize_adj returns (A D)^T D: transposed pattern
  else if (e < E + n) keys[e] = (uint64_t)(e - E) * (uint64_t)n + (uint64_t)(e - E);  // + sp.eye(n)
}

// head[s] = 1 where a run of equal keys starts (LAST = 0) or ends (LAST = 1)
template <bool LAST>
__global__ void __launch_bounds__(256) run_flags_kernel(const uint64_t* __restrict__ keys, int64_t M, int* __restrict__ flag) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= M) return;
  if (LAST) flag[s] = (s == M - 1 || keys[s] != keys[s + 1]) ? 1 : 0;
  else flag[s] = (s == 0 || keys[s] != keys[s - 1]) ? 1 : 0;
}

// pos[u] = sorted position of the u-th flagged element; count = number of flagged elements; pos[count] = M
__global__ void __launch_bounds__(256) run_positions_kernel(const int* __restrict__ flag, const int* __restrict__ slot, int64_t M,
                                                            int64_t* __restrict__ pos, int64_t* __restrict__ count) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= M) return;
  if (flag[s]) pos[slot[s]] = s;
  if (s == M - 1) {
    const int64_t c = (int64_t)slot[s] + flag[s];
    *count = c;
    pos[c] = M;
  }
}

// unique (out_row = original col, out_col = original row) entries with multiplicities; integer degrees of the ORIGINAL rows
__global__ void __launch_bounds__(256) sym_entries_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ pos,
                                                          const int64_t* __restrict__ nnz, int64_t n,
                                                          int64_t* __restrict__ rowptr, int32_t* __restrict__ out_col,
                                                          unsigned* __restrict__ cnt, unsigned* __restrict__ deg) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nn = *nnz;
  if (u == 0) rowptr[n] = nn;
  if (u >= nn) return;
  const uint64_t key = keys[pos[u]];
  const int64_t orow = (int64_t)(key / (uint64_t)n), r = (int64_t)(key % (uint64_t)n);
  const unsigned c = (unsigned)(pos[u + 1] - pos[u]);
  out_col[u] = (int32_t)r;
  cnt[u] = c;
  atomicAdd(deg + r, c);  // row sum of A + I over the original row r (integers: exact in any order)
  if (u == 0 || (int64_t)(keys[pos[u - 1]] / (uint64_t)n) != orow) rowptr[orow] = u;  // every row holds its self loop
}

__global__ void __launch_bounds__(256) sym_values_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ pos,
                                                         const int64_t* __restrict__ nnz, int64_t n,
                                                         const unsigned* __restrict__ cnt, const unsigned* __restrict__ deg,
                                                         float* __restrict__ val) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= *nnz) return;
  const uint64_t key = keys[pos[u]];
  const int64_t c = (int64_t)(key / (uint64_t)n), r = (int64_t)(key % (uint64_t)n);
  const double dr = deg[r] ? pow((double)deg[r], -0.5) : 0.0, dc = deg[c] ? pow((double)deg[c], -0.5) : 0.0;
  val[u] = (float)(((double)cnt[u] * dr) * dc);  // (A[r][c] * d_r) * d_c in float64, cast last
}

// ---- bipartite ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pair_keys_kernel(const int64_t* __restrict__ u, const int64_t* __restrict__ it, int64_t E,
                                                        int64_t num_items, uint64_t* __restrict__ keys, int64_t* __restrict__ idx) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  keys[e] = (uint64_t)u[e] * (uint64_t)num_items + (uint64_t)it[e];
  idx[e] = e;
}

// unique (user, item) pairs: the time of the LAST occurrence; both directed edges' keys (dst * n + src) and degrees
__global__ void __launch_bounds__(256) pair_edges_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ idx,
                                                         const int64_t* __restrict__ pos /* last positions */,
                                                         const int64_t* __restrict__ npairs, const int64_t* __restrict__ step,
                                                         int64_t num_users, int64_t num_items, uint64_t* __restrict__ ekeys,
                                                         int64_t* __restrict__ etime, unsigned* __restrict__ deg) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t np_ = *npairs;
  if (p >= np_) return;
  const int64_t s = pos[p];
  const uint64_t key = keys[s];
  const int64_t uu = (int64_t)(key / (uint64_t)num_items), ii = (int64_t)(key % (uint64_t)num_items) + num_users;
  const uint64_t n = (uint64_t)(num_users + num_items);
  const int64_t t = step[idx[s]];
  ekeys[p] = (uint64_t)ii * n + (uint64_t)uu;        // edge uu -> ii, ordered by (dst, src)
  ekeys[np_ + p] = (uint64_t)uu * n + (uint64_t)ii;  // edge ii -> uu
  etime[p] = t;
  etime[np_ + p] = t;
  atomicAdd(deg + uu, 1u);
  atomicAdd(deg + ii, 1u);
}

__global__ void __launch_bounds__(256) pair_emit_kernel(const uint64_t* __restrict__ ekeys_sorted, const int64_t* __restrict__ etime_sorted,
                                                        const int64_t* __restrict__ npairs, int64_t n,
                                                        const unsigned* __restrict__ deg, int64_t* __restrict__ edges,
                                                        float* __restrict__ norm, int64_t* __restrict__ times,
                                                        int64_t* __restrict__ nedges) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ne = 2 * *npairs;
  if (e == 0) *nedges = ne;
  if (e >= ne) return;
  const uint64_t key = ekeys_sorted[e];
  const int64_t dst = (int64_t)(key / (uint64_t)n), src = (int64_t)(key % (uint64_t)n);
  edges[2 * e] = src;
  edges[2 * e + 1] = dst;
  const double ds = deg[src] ? pow((double)deg[src], -0.5) : 0.0, dd = deg[dst] ? pow((double)deg[dst], -0.5) : 0.0;
  norm[e] = (float)(ds * dd);  // mat.data.astype(np.float32) of the float64 product
  times[e] = etime_sorted[e];
}

// ---- COO -> CSR (stable) ------------------------------------------------------------------------------------------
// key = row (sort_cols = 0: the given edge order survives inside a row -- the order scatter_add_ accumulates in,
// RAGraph_edge/modules/utils.py:17-32) or row * n + col (columns ascending inside a row); the value is the edge's position.
__global__ void __launch_bounds__(256) coo_keys_kernel(const int64_t* __restrict__ row, const int64_t* __restrict__ col, int64_t E,
                                                       int64_t n, int sort_cols, uint64_t* __restrict__ keys,
                                                       int64_t* __restrict__ idx) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  keys[e] = sort_cols ? (uint64_t)row[e] * (uint64_t)n + (uint64_t)col[e] : (uint64_t)row[e];
  idx[e] = e;
}

// rowptr[r] = the first sorted slot whose row is >= r: slot s writes the rows in (row(s - 1), row(s)] -- its own row and
// the empty rows before it --, the last slot also the rows behind it.  O(E + n) stores, no histogram and no prefix sum.
// out_col (optional): the columns in CSR order.
__global__ void __launch_bounds__(256) coo_rowptr_kernel(const uint64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                         const int64_t* __restrict__ col, int64_t E, int64_t n, int sort_cols,
                                                         int64_t* __restrict__ rowptr, int32_t* __restrict__ out_col) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= E) return;
  const uint64_t un = (uint64_t)n;
  const int64_t r = (int64_t)(sort_cols ? keys[s] / un : keys[s]);
  const int64_t rp = s == 0 ? -1 : (int64_t)(sort_cols ? keys[s - 1] / un : keys[s - 1]);
  for (int64_t x = rp + 1; x <= r; ++x) rowptr[x] = s;
  if (s == E - 1)
    for (int64_t x = r + 1; x <= n; ++x) rowptr[x] = E;
  if (out_col) out_col[s] = (int32_t)(sort_cols ? (int64_t)(keys[s] % un) : col[perm[s]]);
}

__global__ void __launch_bounds__(256) fill_i64_kernel(int64_t* __restrict__ p, int64_t n, int64_t v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

// rows[e] = the row whose range [rowptr[r], rowptr[r + 1]) holds e (binary search: the last r with rowptr[r] <= e)
__global__ void __launch_bounds__(256) csr_row_ids_kernel(const int64_t* __restrict__ rowptr, int64_t n, int64_t nnz,
                                                          int64_t* __restrict__ rows) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  int64_t lo = 0, hi = n;   // invariant: rowptr[lo] <= e < rowptr[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (rowptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  rows[e] = lo;
}

// ---- positions of the set elements of a byte mask (boolean indexing without another library's select) --------------
__global__ void __launch_bounds__(256) mask_flags_kernel(const unsigned char* __restrict__ mask, int64_t E, int* __restrict__ flag) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < E) flag[e] = mask[e] ? 1 : 0;
}

__global__ void __launch_bounds__(256) mask_positions_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ slot,
                                                             int64_t E, int64_t* __restrict__ pos, int64_t* __restrict__ count) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  if (mask[e]) pos[slot[e]] = e;
  if (e == E - 1) *count = (int64_t)slot[e] + (mask[e] ? 1 : 0);
}

static int key_bits(uint64_t max_key) {
  int b = 1;
  while (b < 64 && (max_key >> b) != 0) ++b;
  return b;
}

struct IngestWs {
  uint64_t *keys_a, *keys_b;
  int64_t *vals_a, *vals_b, *pos, *count;
  int *flag, *slot;
  unsigned *cnt, *deg;
  void* temp;
  size_t temp_bytes;
};

static size_t ingest_carve(char* w, int64_t M, int64_t n, IngestWs* out) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = w ? w + off : nullptr;
    off += align_up(bytes, 256);
    return p;
  };
  IngestWs f;
  f.keys_a = reinterpret_cast<uint64_t*>(take((size_t)M * 8));
  f.keys_b = reinterpret_cast<uint64_t*>(take((size_t)M * 8));
  f.vals_a = reinterpret_cast<int64_t*>(take((size_t)M * 8));
  f.vals_b = reinterpret_cast<int64_t*>(take((size_t)M * 8));
  f.pos = reinterpret_cast<int64_t*>(take((size_t)(M + 1) * 8));
  f.count = reinterpret_cast<int64_t*>(take(8));
  f.flag = reinterpret_cast<int*>(take((size_t)M * 4));
  f.slot = reinterpret_cast<int*>(take((size_t)M * 4));
  f.cnt = reinterpret_cast<unsigned*>(take((size_t)M * 4));
  f.deg = reinterpret_cast<unsigned*>(take((size_t)n * 4));
  const size_t t1 = radix_sort_temp_bytes(M, 8), t3 = scan_temp_bytes(M);
  f.temp_bytes = t1 > t3 ? t1 : t3;
  f.temp = take(f.temp_bytes + 256);
  if (out) *out = f;
  return off;
}

}  // namespace ragraph

using namespace ragraph;

extern "C" size_t ragraph_ingest_workspace_bytes(int64_t max_keys, int64_t n) {
  if (max_keys < 1 || max_keys >= (int64_t)INT_MAX || n < 1) return 0;
  return ingest_carve(nullptr, max_keys, n, nullptr);
}

#define RG_HIPCUB(call, what)                                                  \
  do {                                                                         \
    hipError_t e__ = (call);                                                   \
    if (e__ != hipSuccess) {                                                   \
      set_error("%s: %s", (what), hipGetErrorString(e__));                     \
      return RAGRAPH_EDEVICE;                                                  \
    }                                                                          \
  } while (0)

extern "C" int ragraph_csr_sym_normalized_f32(const int64_t* row, const int64_t* col, int64_t E, int64_t n, int64_t* rowptr,
                                              int32_t* out_col, float* out_val, int64_t* nnz, void* ws, size_t ws_bytes,
                                              void* stream) {
  RG_REQUIRE((row && col) || E == 0, RAGRAPH_EINVAL, "csr_sym_normalized: null edge list");
  RG_REQUIRE(rowptr && out_col && out_val && nnz && ws, RAGRAPH_EINVAL, "csr_sym_normalized: null pointer");
  RG_REQUIRE(E >= 0 && n >= 1 && n < ((int64_t)1 << 31), RAGRAPH_EINVAL, "csr_sym_normalized: bad E/n");
  const int64_t M = E + n;
  RG_REQUIRE(M < (int64_t)INT_MAX, RAGRAPH_EUNSUPPORTED, "csr_sym_normalized: E + n must fit int32");
  RG_REQUIRE(ws_bytes >= ragraph_ingest_workspace_bytes(M, n), RAGRAPH_EWORKSPACE, "csr_sym_normalized: workspace too small");
  hipStream_t st = as_stream(stream);
  IngestWs f;
  ingest_carve(static_cast<char*>(ws), M, n, &f);
  const unsigned g = (unsigned)cdiv(M, 256);
  RG_HIPCUB(hipMemsetAsync(f.deg, 0, (size_t)n * 4, st), "csr_sym_normalized(memset)");
  hipLaunchKernelGGL(sym_keys_kernel, dim3(g), dim3(256), 0, st, row, col, E, n, f.keys_a);
  int rc = radix_sort_u64(f.keys_a, f.keys_b, nullptr, nullptr, 0, M, key_bits((uint64_t)n * (uint64_t)n), f.temp, f.temp_bytes, st);
  if (rc != RAGRAPH_OK) return rc;
  hipLaunchKernelGGL(run_flags_kernel<false>, dim3(g), dim3(256), 0, st, f.keys_b, M, f.flag);
  rc = scan_sum_i32(f.flag, f.slot, M, false, f.temp, f.temp_bytes, st);
  if (rc != RAGRAPH_OK) return rc;
  hipLaunchKernelGGL(run_positions_kernel, dim3(g), dim3(256), 0, st, f.flag, f.slot, M, f.pos, nnz);
  hipLaunchKernelGGL(sym_entries_kernel, dim3(g), dim3(256), 0, st, f.keys_b, f.pos, nnz, n, rowptr, out_col, f.cnt, f.deg);
  hipLaunchKernelGGL(sym_values_kernel, dim3(g), dim3(256), 0, st, f.keys_b, f.pos, nnz, n, f.cnt, f.deg, out_val);
  RG_CHECK_LAUNCH("csr_sym_normalized");
  return RAGRAPH_OK;
}

extern "C" int ragraph_binorm_edges_f32(const int64_t* users, const int64_t* items, const int64_t* step, int64_t E,
                                        int64_t num_users, int64_t num_items, int64_t* edges, float* norm, int64_t* times,
                                        int64_t* nedges, void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(users && items && step && edges && norm && times && nedges && ws, RAGRAPH_EINVAL, "binorm_edges: null pointer");
  RG_REQUIRE(E >= 1 && num_users >= 1 && num_items >= 1, RAGRAPH_EINVAL, "binorm_edges: bad sizes");
  const int64_t n = num_users + num_items, M = 2 * E;
  RG_REQUIRE(M < (int64_t)INT_MAX && n < ((int64_t)1 << 31), RAGRAPH_EUNSUPPORTED, "binorm_edges: 2E and n must fit int32");
  RG_REQUIRE(ws_bytes >= ragraph_ingest_workspace_bytes(M, n), RAGRAPH_EWORKSPACE, "binorm_edges: workspace too small");
  hipStream_t st = as_stream(stream);
  IngestWs f;
  ingest_carve(static_cast<char*>(ws), M, n, &f);
  const unsigned gE = (unsigned)cdiv(E, 256), gM = (unsigned)cdiv(M, 256);
  RG_HIPCUB(hipMemsetAsync(f.deg, 0, (size_t)n * 4, st), "binorm_edges(memset)");
  hipLaunchKernelGGL(pair_keys_kernel, dim3(gE), dim3(256), 0, st, users, items, E, num_items, f.keys_a, f.vals_a);
  // (the radix sort is stable: among equal (user, item) pairs the original order survives, so a run's last element is the
  // pair's last occurrence)
  int rc = radix_sort_u64(f.keys_a, f.keys_b, f.vals_a, f.vals_b, 8, E, key_bits((uint64_t)num_users * (uint64_t)num_items), f.temp,
                          f.temp_bytes, st);
  if (rc != RAGRAPH_OK) return rc;
  hipLaunchKernelGGL(run_flags_kernel<true>, dim3(gE), dim3(256), 0, st, f.keys_b, E, f.flag);
  rc = scan_sum_i32(f.flag, f.slot, E, false, f.temp, f.temp_bytes, st);
  if (rc != RAGRAPH_OK) return rc;
  hipLaunchKernelGGL(run_positions_kernel, dim3(gE), dim3(256), 0, st, f.flag, f.slot, E, f.pos, f.count);
  // directed edges keyed by (dst, src); keys_a / vals_a are free again
  RG_HIPCUB(hipMemsetAsync(f.keys_a, 0xFF, (size_t)M * 8, st), "binorm_edges(memset keys)");  // unused tail sorts last
  hipLaunchKernelGGL(pair_edges_kernel, dim3(gE), dim3(256), 0, st, f.keys_b, f.vals_b, f.pos, f.count, step, num_users, num_items,
                     f.keys_a, f.vals_a, f.deg);
  // (vals_a beyond 2 * npairs is garbage paired with 0xFF.. keys: sorted behind every real edge)
  rc = radix_sort_u64(f.keys_a, f.keys_b, f.vals_a, f.vals_b, 8, M, 64, f.temp, f.temp_bytes, st);
  if (rc != RAGRAPH_OK) return rc;
  hipLaunchKernelGGL(pair_emit_kernel, dim3(gM), dim3(256), 0, st, f.keys_b, f.vals_b, f.count, n, f.deg, edges, norm, times,
                     nedges);
  RG_CHECK_LAUNCH("binorm_edges");
  return RAGRAPH_OK;
}

// COO -> CSR, stable (what torch.sort(stable) + bincount + cumsum did on the per-step paths until round 5: the edge flavour's
// destination-sorted CSR of every re-drawn edge set, modules/RAGraph.py:337-343 + utils.py:40-53; the transposed pattern of a
// training SpMM; the hit lists of a gather's backward).  perm[s] = the input position of CSR slot s.
extern "C" size_t ragraph_coo_to_csr_workspace_bytes(int64_t E, int64_t n) {
  if (E < 0 || E >= (int64_t)INT_MAX || n < 1) return 0;
  return ingest_carve(nullptr, E > 0 ? E : 1, 1, nullptr);
}

extern "C" int ragraph_coo_to_csr_i64(const int64_t* row, const int64_t* col, int64_t E, int64_t n, int sort_cols, int64_t* rowptr,
                                      int64_t* perm, int32_t* out_col, void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(rowptr && ws && (E == 0 || (row && col && perm)), RAGRAPH_EINVAL, "coo_to_csr: null pointer");
  RG_REQUIRE(E >= 0 && E < (int64_t)INT_MAX && n >= 1 && n < ((int64_t)1 << 31), RAGRAPH_EINVAL, "coo_to_csr: bad E/n");
  RG_REQUIRE(ws_bytes >= ragraph_coo_to_csr_workspace_bytes(E, n), RAGRAPH_EWORKSPACE, "coo_to_csr: workspace too small");
  hipStream_t st = as_stream(stream);
  if (E == 0) {
    hipLaunchKernelGGL(fill_i64_kernel, dim3((unsigned)cdiv(n + 1, 256)), dim3(256), 0, st, rowptr, n + 1, (int64_t)0);
    RG_CHECK_LAUNCH("coo_to_csr");
    return RAGRAPH_OK;
  }
  IngestWs f;
  ingest_carve(static_cast<char*>(ws), E, 1, &f);
  const unsigned g = (unsigned)cdiv(E, 256);
  hipLaunchKernelGGL(coo_keys_kernel, dim3(g), dim3(256), 0, st, row, col, E, n, sort_cols, f.keys_a, f.vals_a);
  const uint64_t max_key = sort_cols ? (uint64_t)n * (uint64_t)n - 1 : (uint64_t)(n - 1);
  const int rc = radix_sort_u64(f.keys_a, f.keys_b, f.vals_a, perm, 8, E, key_bits(max_key), f.temp, f.temp_bytes, st);
  if (rc != RAGRAPH_OK) return rc;
  hipLaunchKernelGGL(coo_rowptr_kernel, dim3(g), dim3(256), 0, st, f.keys_b, perm, col, E, n, sort_cols, rowptr, out_col);
  RG_CHECK_LAUNCH("coo_to_csr");
  return RAGRAPH_OK;
}

extern "C" int ragraph_csr_row_ids_i64(const int64_t* rowptr, int64_t n, int64_t nnz, int64_t* rows, void* stream) {
  RG_REQUIRE(rowptr && (rows || nnz == 0), RAGRAPH_EINVAL, "csr_row_ids: null pointer");
  RG_REQUIRE(n >= 1 && nnz >= 0, RAGRAPH_EINVAL, "csr_row_ids: bad n/nnz");
  if (nnz == 0) return RAGRAPH_OK;
  hipLaunchKernelGGL(csr_row_ids_kernel, dim3((unsigned)cdiv(nnz, 256)), dim3(256), 0, as_stream(stream), rowptr, n, nnz, rows);
  RG_CHECK_LAUNCH("csr_row_ids");
  return RAGRAPH_OK;
}

// pos[j] = the position of the j-th non-zero byte of mask, ascending; *count = how many (the edge dropout of a training step,
// modules/utils.py:40-53: edges[mask] through the library's own prefix sums).  ws: ragraph_mask_positions_workspace_bytes(E).
extern "C" size_t ragraph_mask_positions_workspace_bytes(int64_t E) {
  if (E < 0 || E >= (int64_t)INT_MAX) return 0;
  const int64_t M = E > 0 ? E : 1;
  return 2 * align_up((size_t)M * 4, 256) + scan_temp_bytes(M) + 256;
}

extern "C" int ragraph_mask_positions_i64(const unsigned char* mask, int64_t E, int64_t* pos, int64_t* count, void* ws,
                                          size_t ws_bytes, void* stream) {
  RG_REQUIRE(count && ws && (E == 0 || (mask && pos)), RAGRAPH_EINVAL, "mask_positions: null pointer");
  RG_REQUIRE(E >= 0 && E < (int64_t)INT_MAX, RAGRAPH_EINVAL, "mask_positions: bad E");
  RG_REQUIRE(ws_bytes >= ragraph_mask_positions_workspace_bytes(E), RAGRAPH_EWORKSPACE, "mask_positions: workspace too small");
  hipStream_t st = as_stream(stream);
  if (E == 0) {
    hipLaunchKernelGGL(fill_i64_kernel, dim3(1), dim3(256), 0, st, count, (int64_t)1, (int64_t)0);
    RG_CHECK_LAUNCH("mask_positions");
    return RAGRAPH_OK;
  }
  char* w = static_cast<char*>(ws);
  int* flag = reinterpret_cast<int*>(w);
  int* slot = reinterpret_cast<int*>(w + align_up((size_t)E * 4, 256));
  void* temp = w + 2 * align_up((size_t)E * 4, 256);
  const unsigned g = (unsigned)cdiv(E, 256);
  hipLaunchKernelGGL(mask_flags_kernel, dim3(g), dim3(256), 0, st, mask, E, flag);
  const int rc = scan_sum_i32(flag, slot, E, false, temp, scan_temp_bytes(E) + 256, st);
  if (rc != RAGRAPH_OK) return rc;
  hipLaunchKernelGGL(mask_positions_kernel, dim3(g), dim3(256), 0, st, mask, slot, E, pos, count);
  RG_CHECK_LAUNCH("mask_positions");
  return RAGRAPH_OK;
}

// ---- the edges of a row subset (the backward of ragraph_spmm_csr_rows_f32) --------------------------------------------
// off[r] = the summed lengths of rows[0 .. r) (off[R] = the total; a row outside [0, n) is empty), on the library's own
// prefix sums; then edge e of the subset = (col, r, val) of the (e - off[r])-th edge of row rows[r]: ascending r, CSR order.
namespace ragraph {

__global__ void __launch_bounds__(256) rows_deg_kernel(const int64_t* __restrict__ rowptr, int64_t n,
                                                       const int64_t* __restrict__ rows, int64_t R, int* __restrict__ deg) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > R) return;
  int d = 0;
  if (r < R) {
    const int64_t row = rows[r];
    if (row >= 0 && row < n) d = (int)(rowptr[row + 1] - rowptr[row]);
  }
  deg[r] = d;   // (deg[R] = 0: the exclusive scan of R + 1 terms ends in the total)
}

// int32 prefix sums -> int64; a total of 2^31 or more shows as a sum that went down: off[R] = -1 then
__global__ void __launch_bounds__(256) rows_off_kernel(const int* __restrict__ sum, int64_t R, int64_t* __restrict__ off,
                                                       int* __restrict__ bad) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > R) return;
  if (sum[r] < 0 || (r > 0 && sum[r] < sum[r - 1])) *bad = 1;
  if (r < R) off[r] = sum[r];
}

__global__ void rows_total_kernel(const int* __restrict__ sum, int64_t R, const int* __restrict__ bad, int64_t* __restrict__ off) {
  off[R] = *bad ? -1 : (int64_t)sum[R];
}

__global__ void __launch_bounds__(256) rows_edges_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const float* __restrict__ val, const int64_t* __restrict__ rows,
                                                         int64_t R, const int64_t* __restrict__ off, int64_t E,
                                                         int64_t* __restrict__ out_col, int64_t* __restrict__ out_r,
                                                         float* __restrict__ out_val) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  int64_t lo = 0, hi = R;   // invariant: off[lo] <= e < off[hi]  (the last r with off[r] <= e: the non-empty one)
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= e) lo = mid;
    else hi = mid;
  }
  const int64_t src = rowptr[rows[lo]] + (e - off[lo]);
  out_col[e] = col[src];
  out_r[e] = lo;
  out_val[e] = val[src];
}

}  // namespace ragraph

extern "C" size_t ragraph_csr_rows_offsets_workspace_bytes(int64_t R) {
  if (R < 0 || R + 1 >= (int64_t)INT_MAX) return 0;
  return 256 + 2 * align_up((size_t)(R + 1) * 4, 256) + scan_temp_bytes(R + 1) + 256;
}

extern "C" int ragraph_csr_rows_offsets_i64(const int64_t* rowptr, int64_t n, const int64_t* rows, int64_t R, int64_t* off,
                                            void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(rowptr && off && ws && (rows || R == 0), RAGRAPH_EINVAL, "csr_rows_offsets: null pointer");
  RG_REQUIRE(n >= 0 && R >= 0 && R + 1 < (int64_t)INT_MAX, RAGRAPH_EINVAL, "csr_rows_offsets: bad n/R");
  RG_REQUIRE(ws_bytes >= ragraph_csr_rows_offsets_workspace_bytes(R), RAGRAPH_EWORKSPACE, "csr_rows_offsets: workspace too small");
  hipStream_t st = as_stream(stream);
  char* w = static_cast<char*>(ws);
  int* bad = reinterpret_cast<int*>(w);
  int* deg = reinterpret_cast<int*>(w + 256);
  int* sum = reinterpret_cast<int*>(w + 256 + align_up((size_t)(R + 1) * 4, 256));
  void* temp = w + 256 + 2 * align_up((size_t)(R + 1) * 4, 256);
  RG_HIPCUB(hipMemsetAsync(bad, 0, sizeof(int), st), "csr_rows_offsets(memset)");
  const unsigned g = (unsigned)cdiv(R + 1, 256);
  hipLaunchKernelGGL(rows_deg_kernel, dim3(g), dim3(256), 0, st, rowptr, n, rows, R, deg);
  const int rc = scan_sum_i32(deg, sum, R + 1, false, temp, scan_temp_bytes(R + 1) + 256, st);
  if (rc != RAGRAPH_OK) return rc;
  hipLaunchKernelGGL(rows_off_kernel, dim3(g), dim3(256), 0, st, sum, R, off, bad);
  hipLaunchKernelGGL(rows_total_kernel, dim3(1), dim3(1), 0, st, sum, R, bad, off);
  RG_CHECK_LAUNCH("csr_rows_offsets");
  return RAGRAPH_OK;
}

extern "C" int ragraph_csr_rows_edges_f32(const int64_t* rowptr, const int32_t* col, const float* val, const int64_t* rows,
                                          int64_t R, const int64_t* off, int64_t E, int64_t* out_col, int64_t* out_r,
                                          float* out_val, void* stream) {
  RG_REQUIRE(E >= 0 && R >= 0, RAGRAPH_EINVAL, "csr_rows_edges: bad R/E");
  if (E == 0) return RAGRAPH_OK;
  RG_REQUIRE(rowptr && col && val && rows && off && out_col && out_r && out_val && R >= 1, RAGRAPH_EINVAL,
             "csr_rows_edges: null pointer");
  hipLaunchKernelGGL(rows_edges_kernel, dim3((unsigned)cdiv(E, 256)), dim3(256), 0, as_stream(stream), rowptr, col, val, rows,
                     R, off, E, out_col, out_r, out_val);
  RG_CHECK_LAUNCH("csr_rows_edges");
  return RAGRAPH_OK;
}

// ---- dense [rows, cols] -> CSR (the reference's adjacency and bag-of-words forms, RAGraph_node/layers/gcn.py:26-40) ------------
// One wave per row, four rows per workgroup.  The lanes walk the row in chunks: one ballot per chunk position gives every kept
// entry its rank inside the chunk (v_mbcnt over the lanes below) and the chunk's total (s_bcnt1), which the wave carries as a
// running offset -- columns ascend inside a row without any sort.  An entry is kept iff its bits are not those of +0 or -0
// (torch.nonzero's rule: NaN, infinities and denormals stay, whatever the denormal mode of the comparison), and moves as an
// integer word, so a NaN keeps its payload.  FILL = false: cnt[r] = the row's count (cnt[rows] = 0: the exclusive scan of rows + 1
// terms ends in the total); FILL = true: the same walk behind excl[r], storing only slots below `capacity`; a row without entries
// is not read again.  WALK: D2C_ONE (cols <= 64: one chunk, no loop -- PROTEINS-sized graphs), D2C_SCALAR (64 columns per chunk,
// any alignment), D2C_VEC4 (256 columns per chunk, one 128-bit load per lane: every row starts on 16 bytes).
namespace ragraph {

enum { D2C_ONE = 0, D2C_SCALAR = 1, D2C_VEC4 = 2 };

__device__ __forceinline__ int lanes_below(unsigned long long m) {   // set bits of m below this lane
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ bool d2c_keep(uint32_t bits) { return (bits << 1) != 0u; }

template <bool FILL, int WALK>
__global__ void __launch_bounds__(256) dense_to_csr_kernel(const uint32_t* __restrict__ a, int64_t rows, int64_t cols, int64_t lda,
                                                           int* __restrict__ cnt, const int* __restrict__ excl, int64_t capacity,
                                                           int32_t* __restrict__ col, uint32_t* __restrict__ val) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (!FILL && blockIdx.x == 0 && threadIdx.x == 0) cnt[rows] = 0;
  if (r >= rows) return;
  int64_t at = 0;
  if (FILL) {
    at = excl[r];
    if ((int64_t)excl[r + 1] == at || at >= capacity) return;   // (wave-uniform: an empty row, or one wholly behind the capacity)
  }
  const uint32_t* __restrict__ row = a + r * lda;
  int total = 0;
  auto put = [&](int64_t s, int64_t c, uint32_t bits) {
    if (s < capacity) {
      col[s] = (int32_t)c;
      val[s] = bits;
    }
  };
  if (WALK == D2C_ONE) {
    const uint32_t v = lane < cols ? row[lane] : 0u;
    const bool keep = d2c_keep(v);
    const unsigned long long m = __ballot(keep);
    if (FILL) {
      if (keep) put(at + lanes_below(m), lane, v);
    } else {
      total = __popcll(m);
    }
  } else if (WALK == D2C_SCALAR) {
    for (int64_t cb = 0; cb < cols; cb += 64) {   // (wave-uniform trip count: a ballot inside)
      const int64_t c = cb + lane;
      const uint32_t v = c < cols ? row[c] : 0u;
      const bool keep = d2c_keep(v);
      const unsigned long long m = __ballot(keep);
      if (FILL && keep) put(at + lanes_below(m), c, v);
      const int n = __popcll(m);
      at += n;
      total += n;
    }
  } else {
    auto load4 = [&](int64_t c) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (c + 3 < cols) {
        v = *reinterpret_cast<const uint4*>(row + c);
      } else {                                    // (the one lane that holds the row's end, and the lanes behind it)
        if (c < cols) v.x = row[c];
        if (c + 1 < cols) v.y = row[c + 1];
        if (c + 2 < cols) v.z = row[c + 2];
      }
      return v;
    };
    auto chunk = [&](int64_t c, const uint4 v) {
      const bool k0 = d2c_keep(v.x), k1 = d2c_keep(v.y), k2 = d2c_keep(v.z), k3 = d2c_keep(v.w);
      const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1), m2 = __ballot(k2), m3 = __ballot(k3);
      if (FILL) {   // a lane's four columns are adjacent: the entries of the lanes below come first, then its own in order
        int64_t s = at + lanes_below(m0) + lanes_below(m1) + lanes_below(m2) + lanes_below(m3);
        if (k0) put(s, c, v.x);
        s += k0;
        if (k1) put(s, c + 1, v.y);
        s += k1;
        if (k2) put(s, c + 2, v.z);
        s += k2;
        if (k3) put(s, c + 3, v.w);
      }
      const int n = __popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3);
      at += n;
      total += n;
    };
    // two chunks per trip, both loads in flight before the first ballot (a chunk wholly behind the row's end is all zeros)
    for (int64_t cb = 0; cb < cols; cb += 512) {
      const int64_t c0 = cb + 4 * lane, c1 = c0 + 256;
      const uint4 v0 = load4(c0), v1 = load4(c1);
      chunk(c0, v0);
      chunk(c1, v1);
    }
  }
  if (!FILL && lane == 0) cnt[r] = total;
}

// int32 prefix sums -> rowptr int64 [rows + 1]; status[0] = the total, status[1] = 1 iff it exceeds the capacity
__global__ void __launch_bounds__(256) dense_rowptr_kernel(const int* __restrict__ excl, int64_t rows, int64_t capacity,
                                                           int64_t* __restrict__ rowptr, int64_t* __restrict__ status) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k > rows) return;
  const int64_t v = (int64_t)excl[k];
  rowptr[k] = v;
  if (k == rows) {
    status[0] = v;
    status[1] = v > capacity ? 1 : 0;
  }
}

template <bool FILL>
static void dense_to_csr_launch(int walk, unsigned blocks, hipStream_t st, const uint32_t* a, int64_t rows, int64_t cols,
                                int64_t lda, int* cnt, int64_t capacity, int32_t* col, uint32_t* val) {
  const int* excl = FILL ? cnt : nullptr;
  int* out = FILL ? nullptr : cnt;
  if (walk == D2C_ONE)
    hipLaunchKernelGGL((dense_to_csr_kernel<FILL, D2C_ONE>), dim3(blocks), dim3(256), 0, st, a, rows, cols, lda, out, excl, capacity,
                       col, val);
  else if (walk == D2C_SCALAR)
    hipLaunchKernelGGL((dense_to_csr_kernel<FILL, D2C_SCALAR>), dim3(blocks), dim3(256), 0, st, a, rows, cols, lda, out, excl,
                       capacity, col, val);
  else
    hipLaunchKernelGGL((dense_to_csr_kernel<FILL, D2C_VEC4>), dim3(blocks), dim3(256), 0, st, a, rows, cols, lda, out, excl,
                       capacity, col, val);
}

}  // namespace ragraph

extern "C" size_t ragraph_dense_to_csr_workspace_bytes(int64_t rows, int64_t cols) {
  if (rows < 0 || cols < 0 || rows >= (int64_t)INT_MAX || (cols > 0 && rows > ((int64_t)INT_MAX) / cols)) return 0;
  return align_up((size_t)(rows + 1) * sizeof(int), 256) + scan_temp_bytes(rows + 1);
}

extern "C" int ragraph_dense_to_csr_f32(const float* a, int64_t rows, int64_t cols, int64_t lda, int64_t capacity, int64_t* rowptr,
                                        int32_t* col, float* val, int64_t* status, void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(rows >= 0 && cols >= 0 && rows < (int64_t)INT_MAX, RAGRAPH_EINVAL, "dense_to_csr: bad shape (%lld x %lld)",
             (long long)rows, (long long)cols);
  RG_REQUIRE(cols == 0 || rows <= ((int64_t)INT_MAX) / cols, RAGRAPH_EINVAL,
             "dense_to_csr: %lld x %lld entries (rows * cols must be below 2^31)", (long long)rows, (long long)cols);
  RG_REQUIRE(lda >= cols, RAGRAPH_EINVAL, "dense_to_csr: lda=%lld < cols=%lld", (long long)lda, (long long)cols);
  RG_REQUIRE(capacity >= 0, RAGRAPH_EINVAL, "dense_to_csr: capacity=%lld", (long long)capacity);
  RG_REQUIRE(rowptr && status && ws && (a || rows == 0 || cols == 0), RAGRAPH_EINVAL, "dense_to_csr: null pointer");
  RG_REQUIRE((col == nullptr) == (val == nullptr), RAGRAPH_EINVAL, "dense_to_csr: col and val go together");
  RG_REQUIRE(col || capacity == 0, RAGRAPH_EINVAL, "dense_to_csr: capacity=%lld without col / val", (long long)capacity);
  RG_REQUIRE(ws_bytes >= ragraph_dense_to_csr_workspace_bytes(rows, cols), RAGRAPH_EWORKSPACE,
             "dense_to_csr: workspace too small");
  hipStream_t st = as_stream(stream);
  if (rows == 0 || cols == 0) {
    hipLaunchKernelGGL(fill_i64_kernel, dim3((unsigned)cdiv(rows + 1, 256)), dim3(256), 0, st, rowptr, rows + 1, (int64_t)0);
    hipLaunchKernelGGL(fill_i64_kernel, dim3(1), dim3(256), 0, st, status, (int64_t)2, (int64_t)0);
    RG_CHECK_LAUNCH("dense_to_csr(empty)");
    return RAGRAPH_OK;
  }
  int* cnt = static_cast<int*>(ws);
  const size_t cnt_bytes = align_up((size_t)(rows + 1) * sizeof(int), 256);
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(a);
  const int walk = cols <= 64 ? D2C_ONE : (aligned16(a) && lda % 4 == 0) ? D2C_VEC4 : D2C_SCALAR;
  const unsigned row_blocks = (unsigned)cdiv(rows, 4);
  dense_to_csr_launch<false>(walk, row_blocks, st, bits, rows, cols, lda, cnt, capacity, nullptr, nullptr);
  RG_CHECK_LAUNCH("dense_to_csr(count)");
  const int rc = scan_sum_i32(cnt, cnt, rows + 1, false, static_cast<char*>(ws) + cnt_bytes, ws_bytes - cnt_bytes, st);
  if (rc != RAGRAPH_OK) return rc;
  hipLaunchKernelGGL(dense_rowptr_kernel, dim3((unsigned)cdiv(rows + 1, 256)), dim3(256), 0, st, (const int*)cnt, rows, capacity,
                     rowptr, status);
  RG_CHECK_LAUNCH("dense_to_csr(rowptr)");
  if (capacity > 0) {
    dense_to_csr_launch<true>(walk, row_blocks, st, bits, rows, cols, lda, cnt, capacity, col, reinterpret_cast<uint32_t*>(val));
    RG_CHECK_LAUNCH("dense_to_csr(fill)");
  }
  return RAGRAPH_OK;
}
