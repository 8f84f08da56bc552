// Position codes of a LARGE query graph: distances from every node to the A anchors, relaxed on the
// CSR with the distance vectors in global memory and the rows spread over the whole chip.  anchor_dist_kernel (rows.hip)
// keeps one anchor's vector in LDS -- n <= 40000, A workgroups; this path takes any n < 2^31.
//
// Contract (the same as anchor_dist_kernel and oracle_position_codes_csr, bit for bit): d[u] = min(d[u], val[u,v] + d[v]) over
// the out-edges with val != 0 and v != u, to the fixpoint.  min is exact and every candidate is ONE fp32 add, so lanes, waves
// and workgroups may split a row's edges and reduce in any order without touching a bit; a value read too early is an older
// upper bound and only delays convergence.
//
// Shape:
//   * pull style, single writer: the 16-lane group (or, for a long row, the workgroup) that owns row u is the only writer of
//     d[u, :] and of dirty[u].  No float atomics.
//   * all anchors ride together: the state is [n, 16] floats (64 B per node, lane c of a group = anchor column c), so one
//     neighbour gather serves up to 16 anchors; A > 16 runs ceil(A / 16) such chunks side by side (blockIdx.y).
//   * dirty bytes, two buffers alternating by round: row u writes dirty_cur[u] = "some column of u fell this round" and reads
//     d[v, :] only where dirty_prev[v] is set.  By induction over the rounds d_r[u] <= val[u,v] + d_{r-1}[v] holds for EVERY edge
//     (a neighbour that did not change in round r-1 was already accounted for in an earlier round; initially every row but the
//     anchors' is +inf), so a round that changes nothing has reached the fixpoint.
//   * rounds are kernel boundaries: nothing rests on one workgroup seeing another's stores inside a launch.  "No row changed
//     in a whole launch" is a word the round's workgroups set with an agent-scope atomic store and the NEXT launch reads; three
//     words rotate (round j reads word j % 3, sets word (j + 1) % 3, clears word (j + 2) % 3), so no launch clears a word
//     another workgroup of the same launch reads or sets.  A round whose predecessor changed nothing returns at once.
//   * the round number lives in the workspace (ctl->base, advanced by the finishing kernel of every call), so a call with
//     resume = 1 continues with the right dirty buffer and word whatever the number of rounds of the calls before it.
#include "common.h"

namespace ragraph {

constexpr int PC_COLS = 16;                                   // anchor columns per chunk = lanes per row group
constexpr int PC_LONG = RAGRAPH_POSITION_CODES_LONG_ROW;      // a row with MORE edges than this goes to a whole workgroup
constexpr int PC_THREADS = 1024;
constexpr int PC_GROUPS = PC_THREADS / PC_COLS;               // row groups per workgroup
constexpr int PC_GATHER = 4;                                  // neighbour rows a group gathers before it folds them
constexpr int PC_LONG_UNROLL = 8;                             // 16-edge pieces a group of a long row's workgroup keeps in flight
constexpr int PC_MAX_ROW_BLOCKS = 8192;                       // grid-stride beyond (bounds the stores to the changed word)
constexpr int PC_LONG_BLOCKS = 64;                            // workgroups that share the long rows of one chunk

struct PcControl {      // first 256 bytes of the workspace
  unsigned changed[3];  // changed[(j + 1) % 3] != 0: round j lowered some distance
  unsigned base;        // rounds run by the calls before this one (since resume = 0)
  unsigned long_count;  // rows with more than PC_LONG edges, listed in long_rows
};

struct PcLayout {
  size_t d, dirty, long_rows, total;
  int chunks;
};
static inline PcLayout pc_layout(int64_t n, int A) {
  PcLayout l;
  l.chunks = (int)cdiv(A, PC_COLS);
  l.d = 256;
  l.dirty = l.d + align_up((size_t)l.chunks * (size_t)n * PC_COLS * sizeof(float), 256);
  l.long_rows = l.dirty + align_up((size_t)l.chunks * 2 * (size_t)n, 256);
  l.total = l.long_rows + align_up((size_t)n * sizeof(int32_t), 256);
  return l;
}

// The 16-bit slice of a wave ballot that belongs to this lane's row group.
__device__ __forceinline__ unsigned group_ballot(bool p) {
  const unsigned long long b = __ballot(p);
  return (unsigned)(b >> (threadIdx.x & 48)) & 0xFFFFu;
}

// state: 0 at an anchor's own node, +inf elsewhere; dirty_prev = the anchors' rows; the list of long rows.
__global__ void __launch_bounds__(PC_THREADS) pc_init_kernel(const int64_t* __restrict__ rowptr, int64_t n,
                                                             const int64_t* __restrict__ anchors, int A,
                                                             PcControl* __restrict__ ctl, float* __restrict__ d,
                                                             unsigned char* __restrict__ dirty,
                                                             int32_t* __restrict__ long_rows) {
  const int c = threadIdx.x & (PC_COLS - 1);
  const int chunk = blockIdx.y;
  const int a = chunk * PC_COLS + c;
  const int64_t mine = a < A ? anchors[a] : -1;
  float* dc = d + (size_t)chunk * (size_t)n * PC_COLS;
  unsigned char* dirty0 = dirty + (size_t)chunk * 2 * (size_t)n;
  const int64_t stride = (int64_t)gridDim.x * PC_GROUPS;
  for (int64_t u = (int64_t)blockIdx.x * PC_GROUPS + (threadIdx.x >> 4); u < n; u += stride) {
    const bool here = mine == u;
    dc[(size_t)u * PC_COLS + c] = here ? 0.f : __builtin_huge_valf();
    const unsigned any = group_ballot(here);
    if (c == 0) {
      dirty0[u] = any != 0;
      if (chunk == 0 && rowptr[u + 1] - rowptr[u] > PC_LONG) long_rows[atomicAdd(&ctl->long_count, 1u)] = (int32_t)u;
    }
  }
  if (blockIdx.x == 0 && chunk == 0 && threadIdx.x == 0) ctl->changed[0] = 1;   // round 0 has a predecessor that "changed"
}

// One round.  Workgroups [0, row_blocks) deal the rows over their 16-lane groups (long rows skipped); the PC_LONG_BLOCKS
// workgroups behind them take the long rows, one workgroup per row at a time.
__global__ void __launch_bounds__(PC_THREADS) pc_round_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                              const float* __restrict__ val, int64_t n, PcControl* ctl,
                                                              float* d, unsigned char* dirty, const int32_t* __restrict__ long_rows,
                                                              unsigned round_in_call, int row_blocks, int use_dirty) {
  __shared__ float part[PC_GROUPS][PC_COLS];
  const unsigned j = ctl->base + round_in_call;
  const int chunk = blockIdx.y;
  if (blockIdx.x == 0 && chunk == 0 && threadIdx.x == 0) ctl->changed[(j + 2) % 3] = 0;   // nobody reads or sets it in this launch
  if (ctl->changed[j % 3] == 0) return;   // the predecessor changed nothing: the fixpoint is reached (word (j+1)%3 stays 0)
  const int c = threadIdx.x & (PC_COLS - 1);
  const int grp = threadIdx.x >> 4;
  float* dc = d + (size_t)chunk * (size_t)n * PC_COLS;
  const unsigned char* dirty_prev = dirty + ((size_t)chunk * 2 + (j & 1)) * (size_t)n;
  unsigned char* dirty_cur = dirty + ((size_t)chunk * 2 + ((j & 1) ^ 1)) * (size_t)n;
  int changed = 0;

  // The edges [e0, e0 + 16) of row u, lane c the edge e0 + c: loaded, marked live (a real edge to a neighbour that changed in
  // the round before), then the live ones folded, PC_GATHER at a time: 16 lanes = 16 columns of d[v, :].
  struct Piece {
    int v;
    float w;
    bool live;
  };
  auto load_piece = [&](int64_t u, int64_t e0, int64_t e1) {
    Piece p = {0, 0.f, false};
    const int64_t e = e0 + c;
    if (e < e1) {
      p.v = col[e];
      p.w = val[e];
      p.live = p.w != 0.f && (int64_t)p.v != u;
    }
    return p;
  };
  auto mark_piece = [&](Piece& p) {
    if (use_dirty && p.live) p.live = dirty_prev[p.v] != 0;
  };
  auto fold_piece = [&](const Piece& p, float best) {
    unsigned m = group_ballot(p.live);
    while (m) {   // PC_GATHER neighbour rows in flight: the gathers are the latency of a round in which most neighbours changed
      float ww[PC_GATHER], dv[PC_GATHER];
#pragma unroll
      for (int q = 0; q < PC_GATHER; ++q) {
        ww[q] = 0.f;
        dv[q] = __builtin_huge_valf();   // (no edge left: w + inf = inf loses every min)
        if (m) {
          const int k = __builtin_ctz(m);
          m &= m - 1;
          ww[q] = __shfl(p.w, k, PC_COLS);
          dv[q] = dc[(size_t)__shfl(p.v, k, PC_COLS) * PC_COLS + c];
        }
      }
#pragma unroll
      for (int q = 0; q < PC_GATHER; ++q) best = fminf(best, __fadd_rn(ww[q], dv[q]));
    }
    return best;
  };

  if ((int)blockIdx.x < row_blocks) {
    const int64_t stride = (int64_t)row_blocks * PC_GROUPS;
    for (int64_t u = (int64_t)blockIdx.x * PC_GROUPS + grp; u < n; u += stride) {
      const int64_t rs = rowptr[u], re = rowptr[u + 1];
      if (re - rs > PC_LONG) continue;
      const float cur = dc[(size_t)u * PC_COLS + c];
      float best = cur;
      for (int64_t e0 = rs; e0 < re; e0 += PC_COLS) {
        Piece p = load_piece(u, e0, re);
        mark_piece(p);
        best = fold_piece(p, best);
      }
      const bool fell = best < cur;
      if (fell) dc[(size_t)u * PC_COLS + c] = best;
      const unsigned any = group_ballot(fell);
      if (c == 0) dirty_cur[u] = any != 0;
      changed |= fell;
    }
  } else {
    const unsigned count = ctl->long_count;
    for (unsigned i = blockIdx.x - row_blocks; i < count; i += PC_LONG_BLOCKS) {
      const int64_t u = long_rows[i];
      const int64_t rs = rowptr[u], re = rowptr[u + 1];
      const float cur = dc[(size_t)u * PC_COLS + c];
      float best = cur;
      // the col / val loads of PC_LONG_UNROLL pieces go out together, then their dirty bytes: a hub row is a latency chain
      for (int64_t e0 = rs + grp * PC_COLS; e0 < re; e0 += (int64_t)PC_THREADS * PC_LONG_UNROLL) {
        Piece p[PC_LONG_UNROLL];
#pragma unroll
        for (int q = 0; q < PC_LONG_UNROLL; ++q) p[q] = load_piece(u, e0 + (int64_t)q * PC_THREADS, re);
#pragma unroll
        for (int q = 0; q < PC_LONG_UNROLL; ++q) mark_piece(p[q]);
#pragma unroll
        for (int q = 0; q < PC_LONG_UNROLL; ++q) best = fold_piece(p[q], best);
      }
      part[grp][c] = best;
      __syncthreads();
      if (grp == 0) {
#pragma unroll
        for (int g = 1; g < PC_GROUPS; ++g) best = fminf(best, part[g][c]);
        const bool fell = best < cur;
        if (fell) dc[(size_t)u * PC_COLS + c] = best;
        const unsigned any = group_ballot(fell);
        if (c == 0) dirty_cur[u] = any != 0;
        changed |= fell;
      }
      __syncthreads();
    }
  }
  if (__syncthreads_or(changed) && threadIdx.x == 0)
    __hip_atomic_store(&ctl->changed[(j + 1) % 3], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// codes, dist and the converged word from the state; advances the round number for a call with resume = 1.
__global__ void __launch_bounds__(PC_THREADS) pc_finish_kernel(const float* __restrict__ d, int64_t n, int A, float dis_q,
                                                               float* __restrict__ codes, float* __restrict__ dist,
                                                               PcControl* __restrict__ ctl, unsigned rounds,
                                                               int32_t* __restrict__ converged) {
  const int64_t total = n * (int64_t)A;
  const int64_t stride = (int64_t)gridDim.x * PC_THREADS;
  for (int64_t e = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x; e < total; e += stride) {
    const int64_t u = e / A;
    const int a = (int)(e - u * A);
    const float x = d[((size_t)(a / PC_COLS) * (size_t)n + (size_t)u) * PC_COLS + (a % PC_COLS)];
    if (dist) dist[e] = x;
    codes[e] = position_code_of(x, dis_q);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned j = ctl->base + rounds;          // the word the last round of this call set (or left clear)
    if (converged) *converged = ctl->changed[j % 3] == 0;
    ctl->base = j;
  }
}

// RAGRAPH_POSITION_CODES_DIRTY=0 (read per call): every neighbour is read in every round -- the A/B of the dirty bytes
// (tools/position_codes_probe.py).  Same bits either way.
static bool pc_use_dirty() {
  const char* e = getenv("RAGRAPH_POSITION_CODES_DIRTY");
  return !(e && e[0] == '0');
}

}  // namespace ragraph

using namespace ragraph;

extern "C" size_t ragraph_position_codes_csr_global_workspace_bytes(int64_t n, int A) {
  if (n < 1 || A < 1 || n >= ((int64_t)1 << 31)) return 0;
  return pc_layout(n, A).total;
}

extern "C" int ragraph_position_codes_csr_global_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n,
                                                     const int64_t* anchors, int A, float dis_q, float* codes, float* dist,
                                                     int rounds, int resume, int32_t* converged, void* ws, size_t ws_bytes,
                                                     void* stream) {
  RG_REQUIRE(rowptr && anchors && codes && ws, RAGRAPH_EINVAL, "position_codes_csr_global: null pointer");
  RG_REQUIRE(n >= 1 && A >= 1, RAGRAPH_EINVAL, "position_codes_csr_global: bad shape");
  RG_REQUIRE(n < ((int64_t)1 << 31), RAGRAPH_EUNSUPPORTED, "position_codes_csr_global: n=%lld: node ids are int32", (long long)n);
  RG_REQUIRE(rounds >= 1, RAGRAPH_EINVAL, "position_codes_csr_global: rounds=%d", rounds);
  const PcLayout l = pc_layout(n, A);
  RG_REQUIRE(ws_bytes >= l.total, RAGRAPH_EWORKSPACE, "position_codes_csr_global: workspace too small");
  RG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 63u) == 0, RAGRAPH_EINVAL, "position_codes_csr_global: workspace not 64-byte aligned");
  char* w = static_cast<char*>(ws);
  PcControl* ctl = reinterpret_cast<PcControl*>(w);
  float* d = reinterpret_cast<float*>(w + l.d);
  unsigned char* dirty = reinterpret_cast<unsigned char*>(w + l.dirty);
  int32_t* long_rows = reinterpret_cast<int32_t*>(w + l.long_rows);
  hipStream_t st = as_stream(stream);
  const int row_blocks = (int)(cdiv(n, PC_GROUPS) < PC_MAX_ROW_BLOCKS ? cdiv(n, PC_GROUPS) : PC_MAX_ROW_BLOCKS);
  if (!resume) {
    if (hipError_t e = hipMemsetAsync(ctl, 0, sizeof(PcControl), st); e != hipSuccess) {
      set_error("position_codes_csr_global: memset failed: %s", hipGetErrorString(e));
      return RAGRAPH_EDEVICE;
    }
    hipLaunchKernelGGL(pc_init_kernel, dim3((unsigned)row_blocks, (unsigned)l.chunks), dim3(PC_THREADS), 0, st, rowptr, n, anchors,
                       A, ctl, d, dirty, long_rows);
  }
  const int use_dirty = pc_use_dirty() ? 1 : 0;
  for (int r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(pc_round_kernel, dim3((unsigned)(row_blocks + PC_LONG_BLOCKS), (unsigned)l.chunks), dim3(PC_THREADS), 0, st,
                       rowptr, col, val, n, ctl, d, dirty, long_rows, (unsigned)r, row_blocks, use_dirty);
  const int64_t fin = cdiv(n * (int64_t)A, PC_THREADS);
  hipLaunchKernelGGL(pc_finish_kernel, dim3((unsigned)(fin < 65536 ? fin : 65536)), dim3(PC_THREADS), 0, st, d, n, A, dis_q, codes,
                     dist, ctl, (unsigned)rounds, converged);
  RG_CHECK_LAUNCH("position_codes_csr_global");
  return RAGRAPH_OK;
}
