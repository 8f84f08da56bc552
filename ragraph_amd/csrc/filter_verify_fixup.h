// Behind the last level: the verdict on a speculative first bound (single bank; merged rows of a sharded bank) and the sliced exact scans of the listed queries.
// Part of csrc/topk_filter.hip (textually included there, inside its namespace / after its helpers): split out in round 6 so
// that the ring, the candidate path and the launch plumbing can be read -- and changed -- apart.  No include guard on purpose:
// these are not stand-alone headers.

// A call that filtered with a SPECULATIVE first bound (ragraph_topk_cosine_filtered_set_prior: theta = the prior for every
// query, no bound pass) is exact for a query iff its final k-th best candidate scores at least the prior: a level filtered
// with theta_l = max(prior, the running exact k-th best) <= the final k-th best, so every key that scores at least the
// final k-th best passed its level.  A query whose k-th best is below the prior (or that found fewer than k candidates) is
// listed for the exact scan of the fixup launch behind this one, like a query whose list overflowed.  The same pass
// records the smallest / largest final k-th best of the call (stats[18] / [19]): the next call's prior comes from them.
// (Zero queries -- flag 2 -- are answered without a scan and not judged; queries already listed by the final level
// -- flag 1 / an overflowed list -- carry -inf or stale rows: listed twice would be scanned twice, so they are skipped by
// their flag.)
// Under a TIGHT bound t (below; delta > 0 then, 0 otherwise) the same read of the k-th best scores also counts the LOW TAIL of
// their distribution: the judged queries (flag 0, proven against the prior) whose final k-th best is below t + m delta for
// m = 1, 2, 4, 8 go to stats[25 .. 28], and stats[24] holds delta's bits (0: not reported).  With stats[22] -- the count below
// t itself: a query's k-th best found is below t iff its final one is -- that is five points of the cumulative count, from
// which the owner of the bank places the next call's t at a soft-miss COUNT (ragraph_amd/kernels_index.py).  The edges are
// formed in fp32 as t + m delta (m delta is exact: a power of two).
// FILTER_VERIFY_ROWS queries per thread: the launch is bound by its atomics on the one line of statistics words, not by the
// 400 KB it reads (100 000 queries, 12 us with three words per 256 queries; the four tail words took that to 26 us), so a
// workgroup judges 1024 queries and the words see a quarter of the workgroups.
constexpr int FILTER_TAIL_EDGES = 4;
constexpr int FILTER_VERIFY_ROWS = 4;
__global__ void __launch_bounds__(256) filter_verify_prior_kernel(const float* __restrict__ out_s, int64_t B, int k, float prior,
                                                                  int speculative, const unsigned char* __restrict__ flag,
                                                                  int* __restrict__ overflow, int* __restrict__ overflow_list,
                                                                  int* __restrict__ stats, float tight, float delta) {
  int lo = INT_MAX, hi = INT_MIN, failed = 0;
  const bool tail = delta > 0.f;   // (launch-uniform)
  int below[FILTER_TAIL_EDGES] = {0, 0, 0, 0};
#pragma unroll
  for (int r = 0; r < FILTER_VERIFY_ROWS; ++r) {
    const int64_t q = ((int64_t)blockIdx.x * FILTER_VERIFY_ROWS + r) * 256 + threadIdx.x;
    float judged = __builtin_huge_valf();   // the k-th best of a query the tail counts (+inf: below no edge)
    if (q < B && flag[q] != 2) {
      const float kth = out_s[q * k + k - 1];
      if (speculative && flag[q] == 0 && !(kth >= prior)) {
        overflow_list[atomicAdd(overflow, 1)] = (int)q;
        failed += 1;
      } else if (kth > RG_NEG_INF) {
        lo = min(lo, f2ord(kth));
        hi = max(hi, f2ord(kth));
        if (flag[q] == 0) judged = kth;
      }
    }
    if (tail) {
#pragma unroll
      for (int e = 0; e < FILTER_TAIL_EDGES; ++e) below[e] += __popcll(__ballot(judged < tight + (float)(1 << e) * delta));
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    lo = min(lo, __shfl_xor(lo, off));
    hi = max(hi, __shfl_xor(hi, off));
    failed += __shfl_xor(failed, off);
  }
  // one set of atomics per WORKGROUP (a returning atomic on one address costs ~11 ns chip-wide: 1600 waves of a 100 000-query
  // call at three each were 38 us of a launch that reads 400 KB)
  __shared__ int red[3 + FILTER_TAIL_EDGES][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][w] = lo;
    red[1][w] = hi;
    red[2][w] = failed;
#pragma unroll
    for (int e = 0; e < FILTER_TAIL_EDGES; ++e) red[3 + e][w] = below[e];
  }
  __syncthreads();
  if (threadIdx.x == 0 && stats) {
    lo = min(min(red[0][0], red[0][1]), min(red[0][2], red[0][3]));
    hi = max(max(red[1][0], red[1][1]), max(red[1][2], red[1][3]));
    failed = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    if (lo != INT_MAX) atomicMin(stats + 18, lo);
    if (hi != INT_MIN) atomicMax(stats + 19, hi);
    if (failed) atomicAdd(stats + 17, failed);
    if (tail) {
      if (blockIdx.x == 0) stats[24] = __float_as_int(delta);
#pragma unroll
      for (int e = 0; e < FILTER_TAIL_EDGES; ++e) {
        const int n = red[3 + e][0] + red[3 + e][1] + red[3 + e][2] + red[3 + e][3];
        if (n) atomicAdd(stats + 25 + e, n);
      }
    }
  }
}

// ---- a TIGHT speculative bound t on top of the prior p (filter_schedule.h: FilterCall::tight) -------------------------------
// The levels filtered with theta = max(t, the running exact k-th best).  Behind their rescoring:
//   * a query whose k-th best found is >= t is PROVEN: every key that scores at least that passed.  theta[q] = +inf -- it
//     passes nothing in the repair.
//   * any other unflagged query is a SOFT miss.  Its k-th best found (exact score of a real key), floored by p, is a lower
//     bound of its final k-th best as good as p itself: theta[q] = max(p, k-th best found), or p when it found fewer than k.
//     Its row number goes to list[] (the first FILTER_REPAIR_Q of them; stats[22] counts them all), and its running result is
//     RESET to the empty row: the repair relists every key it needs, including those already found, so no key is merged
//     twice (a winner listed twice breaks the selection: docs/HISTORY.md, round 3).
//   * flagged queries (2: zero query, 1: overflowed list) are left to the final rescoring and the fixup launch as ever.
// Then the repair, enqueued unconditionally and gated by stats[22] on the device (FilterGate), no host read-back:
//   1 .. 256 soft misses: filter_repair_gather_kernel copies their raw rows into a compact batch of 256 (zero rows beyond the
//     count -- zero queries, answered without work); filter_prep_kernel prepares it; ONE pass of the direct kernel over [0, N)
//     with the per-query theta and its rescoring; filter_repair_scatter_kernel writes the rows back (local indices) or hands
//     a row whose repair list overflowed to the exact scan (flag 1).
//   more: one more ring level over [0, N) for all B queries with theta[] -- proven queries pass nothing -- the bounded worst case.
// Behind either, the call's FINAL rescoring launch (merge with the running rows, + idx_base, overflow lists), then the
// verdict against p (filter_verify_prior_kernel: a repaired query whose final k-th best is below p was repaired from a bound
// that was too high -- a hard miss, scanned) and the fixup launch, unchanged.
// Statistics words: [21] = 1 a tight bound was in force, [22] soft misses, [23] the repair that ran (0 none, 1 the 256-query
// call, 2 the all-queries level), [24] delta = (t - p) / 16 as float bits and [25 .. 28] the judged queries whose final k-th
// best is below t + delta, + 2 delta, + 4 delta, + 8 delta (filter_verify_prior_kernel above).
// The FINAL rescoring of such a call finds an empty list for every query the all-queries level did not serve -- all of them
// unless it ran -- and such a query's merge would rewrite the row it read: with idx_base == 0 its wave returns on the count and
// the flag alone (filter_rescore.h: SKIP).
__global__ void __launch_bounds__(256) filter_tight_verdict_kernel(float* __restrict__ out_s, int64_t* __restrict__ out_i, int64_t B,
                                                                   int k, float tight, float prior,
                                                                   const unsigned char* __restrict__ flag, float* __restrict__ theta,
                                                                   int* __restrict__ list, int* __restrict__ stats) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if (q == 0) stats[21] = 1;
  bool soft = false;
  float kth = RG_NEG_INF;
  if (q < B) {
    kth = out_s[q * k + k - 1];
    soft = flag[q] == 0 && !(kth >= tight);
    theta[q] = soft ? fmaxf(prior, kth) : __builtin_huge_valf();
  }
  // one atomic per wave that saw any (a flood of soft misses would serialise on the one counter otherwise)
  const unsigned long long m = __ballot(soft);
  if (m == 0ull) return;  // (wave-uniform)
  int base = 0;
  if (lane == 0) base = atomicAdd(stats + 22, __popcll(m));
  base = __shfl(base, 0);
  if (!soft) return;
  const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
  if (pos < FILTER_REPAIR_Q) list[pos] = (int)q;
  for (int j = 0; j < k; ++j) {
    out_s[q * k + j] = RG_NEG_INF;
    out_i[q * k + j] = INT64_MAX;
  }
}

// One wave per row of the compact batch.  (Always writes all 256 rows: zero rows when there is nothing for the 256-query
// repair to do, so the launches behind it read defined memory whatever the count.)
template <int D>
__global__ void __launch_bounds__(64) filter_repair_gather_kernel(const float* __restrict__ Q, const float* __restrict__ theta,
                                                                  const int* __restrict__ list, float* __restrict__ Q2,
                                                                  float* __restrict__ theta2, int* __restrict__ stats) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const int n = stats[22];
  if (row == 0 && lane == 0) stats[23] = n == 0 ? 0 : (n <= FILTER_REPAIR_Q ? 1 : 2);
  const bool live = n <= FILTER_REPAIR_Q && row < n;
  const int64_t q = live ? list[row] : 0;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live && lane < D / 4) v = reinterpret_cast<const float4*>(Q + q * D)[lane];
  if (lane < D / 4) reinterpret_cast<float4*>(Q2 + (int64_t)row * D)[lane] = v;
  if (lane == 0) theta2[row] = live ? theta[q] : 0.f;
}

// LW = 128 (lists of 65 .. 128 keys): a lane copies two entries of the row.
template <int LW = 64>
__global__ void __launch_bounds__(64) filter_repair_scatter_kernel(const int* __restrict__ list, const float* __restrict__ s2,
                                                                   const int64_t* __restrict__ i2,
                                                                   const unsigned char* __restrict__ flag2, int k,
                                                                   float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                                   unsigned char* __restrict__ flag, const int* __restrict__ stats) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const int n = stats[22];
  if (n < 1 || n > FILTER_REPAIR_Q || row >= n) return;
  const int64_t q = list[row];
  if (flag2[row] != 0) {  // its repair list overflowed: the final rescoring lists the row for the exact scan
    if (lane == 0) flag[q] = 1;
    return;
  }
  if (lane < k) {
    out_s[q * k + lane] = s2[(int64_t)row * k + lane];
    out_i[q * k + lane] = i2[(int64_t)row * k + lane];
  }
  if constexpr (LW > 64) {
    if (lane + 64 < k) {
      out_s[q * k + lane + 64] = s2[(int64_t)row * k + lane + 64];
      out_i[q * k + lane + 64] = i2[(int64_t)row * k + lane + 64];
    }
  }
}

// Sharded banks under a speculative first bound: the verdict of the rows' OWNER, behind the merge of the shards' lists.  One
// workgroup walks the R merged rows: a row is proven iff its k-th best reaches the prior (an all-zero query -- every score +0 --
// is answered by index order and needs no proof); out[0] = rows that missed, out[1] = -(smallest proven k-th best), out[2] =
// the largest, out[3] = this shard's candidates per query over its levels (the call's statistics words; -1 without them),
// out[4] = its overflowed lists: five numbers that ONE all_reduce MAX turns into the group's (ragraph_amd/sharded.py).
__global__ void __launch_bounds__(256) verify_merged_prior_kernel(const float* __restrict__ s, int64_t R, int k, float prior,
                                                                  int speculative, const int* __restrict__ words,
                                                                  const int* __restrict__ overflow, float* __restrict__ out) {
  __shared__ float red[3][4];
  float miss = 0.f, neg_lo = RG_NEG_INF, hi = RG_NEG_INF;
  for (int64_t q = threadIdx.x; q < R; q += 256) {
    const float top = s[q * k], kth = s[q * k + k - 1];
    const bool zero = top == 0.f && kth == 0.f;
    const bool ok = zero || !speculative || kth >= prior;
    if (!ok) miss += 1.f;
    else if (!zero && kth > RG_NEG_INF) {
      neg_lo = fmaxf(neg_lo, -kth);
      hi = fmaxf(hi, kth);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    miss += __shfl_xor(miss, off);
    neg_lo = fmaxf(neg_lo, __shfl_xor(neg_lo, off));
    hi = fmaxf(hi, __shfl_xor(hi, off));
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][w] = miss;
    red[1][w] = neg_lo;
    red[2][w] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    out[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    out[2] = fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3]));
    float cand = -1.f;
    if (words && words[0] == FILTER_STATS_MAGIC) {
      cand = 0.f;
      for (int l = 0; l < 3; ++l)
        if (words[5 + l] > 0) cand += (float)words[2 + l] / (float)words[5 + l];
    }
    out[3] = cand;
    out[4] = overflow ? (float)*overflow : 0.f;
  }
}

// Large batches (the one-wave-per-query rescoring kernels): the final level has listed the overflowed queries, and this
// launch -- a fixed grid that finds an empty list on ordinary banks and returns -- runs exact_scan_query for each.
// (Below 2048 queries the workgroup-per-query rescoring kernels call it themselves and this launch is not made.)
// The exact scan of the queries the final level could not serve, in ONE launch behind it (calls of 65 queries and more;
// smaller ones scan inside their rescoring launch).  Few overflowed queries -- the usual case when there are any: a
// tight cluster next to a handful of queries -- would leave the chip idle behind one workgroup per query (25 ms per
// scan of 1M x 256 keys; 94 ms when the query's own rescoring wave did it), so a query's scan is cut into up to
// FILTER_FIX_SLICES key slices (as many as keep ~256 workgroups busy), each workgroup leaves its slice's k winners in
// part_s / part_i, and the query's last slice to finish (a ticket) merges them: 1.6 ms for one query.  Many overflowed
// queries take one workgroup each as before.  A ZERO query is answered without a scan.
// LW = 64 (the wide entry, 33 <= k <= 64): a slice leaves up to 64 winners, so the scans are cut into HALF as many slices
// (FILTER_FIX_SLICES * 32 / LW = 8) rather than carrying 16 x 64 = sixteen slots per lane of the merging wave: SL k <= 512
// and the part_s / part_i buffers keep their size, the merge keeps its eight slots, and a path that ordinary banks never take
// (it exists for adversarial clusters) gives up at most a factor of two on a lone overflowed query.
// LW = 128 (65 <= k <= 128): a quarter of the slices (4 x 128 winners, the same bytes and the same eight slots of the merge).
template <int D, int LW = 32>
__global__ void __launch_bounds__(256) topk_overflow_fixup_kernel(const float* __restrict__ Qn, const float* __restrict__ Kn,
                                                                  int64_t N, int k, int64_t idx_base,
                                                                  const int* __restrict__ overflow,
                                                                  const int* __restrict__ overflow_list,
                                                                  int64_t* __restrict__ overflow_idx_out,
                                                                  float* __restrict__ out_s, int64_t* __restrict__ out_i,
                                                                  int* __restrict__ done, float* __restrict__ part_s,
                                                                  int64_t* __restrict__ part_i, int64_t B,
                                                                  const unsigned char* __restrict__ flag,
                                                                  int* __restrict__ stats) {
  __shared__ float4 qs[D / 4];
  __shared__ __attribute__((aligned(16))) float tile[4][64 * RESCORE_LD];
  __shared__ float ps[4][LW];
  __shared__ int64_t pi[4][LW];
  __shared__ int ticket_s;
  const int n_over = *overflow;
  if (stats && blockIdx.x == 0 && threadIdx.x == 0) stats[20] = n_over;   // (final: every launch that counts runs before this one)
  if (stats && stats[16] == 0) {
    // the smallest / largest final k-th best score of the call's queries (stats[18] / [19]; a speculative call's verify
    // launch has recorded them already): one value per thread, wave-reduced, two atomics per wave that saw any.
    int lo = INT_MAX, hi = INT_MIN;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < B; q += (int64_t)gridDim.x * 256) {
      // (zero queries -- flag 2 -- have no k-th best; rows flagged 1 are listed for the scans below and hold what torch.empty
      // left or a stale candidate row that the scans rewrite during this very launch: neither may reach the history words)
      const float kth = flag[q] != 0 ? RG_NEG_INF : out_s[q * k + k - 1];
      if (kth > RG_NEG_INF) {
        lo = min(lo, f2ord(kth));
        hi = max(hi, f2ord(kth));
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      lo = min(lo, __shfl_xor(lo, off));
      hi = max(hi, __shfl_xor(hi, off));
    }
    if ((threadIdx.x & 63) == 0) {
      if (lo != INT_MAX) atomicMin(stats + 18, lo);
      if (hi != INT_MIN) atomicMax(stats + 19, hi);
    }
  }
  if (n_over <= 0) return;
  int SL = 1;
  if (n_over <= FILTER_FIX_MAX_Q)
    while (SL < FILTER_FIX_SLICES * 32 / LW && 2 * SL * n_over <= (int)gridDim.x) SL *= 2;
  const int64_t chunk = ((N + SL - 1) / SL + 63) / 64 * 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t item = blockIdx.x; item < (int64_t)n_over * SL; item += gridDim.x) {
    const int o = (int)(item / SL), sl = (int)(item % SL);
    const int64_t b = overflow_list[o];
    if (overflow_idx_out && threadIdx.x == 0 && sl == 0) overflow_idx_out[o] = b;
    __syncthreads();  // (the previous item's readers of qs)
    if (threadIdx.x < D / 4) qs[threadIdx.x] = reinterpret_cast<const float4*>(Qn + b * D)[threadIdx.x];
    __syncthreads();
    if (SL == 1) {
      exact_scan_query<D, LW>(qs, Kn, N, k, idx_base, tile, ps, pi, out_s + b * k, out_i + b * k);
      continue;
    }
    const int64_t lo = sl * chunk, hi = lo + chunk < N ? lo + chunk : N;
    float* my_s = part_s + ((int64_t)o * SL + sl) * LW;
    int64_t* my_i = part_i + ((int64_t)o * SL + sl) * LW;
    if (lo < hi) {
      exact_scan_query<D, LW>(qs, Kn + lo * D, hi - lo, k, lo, tile, ps, pi, my_s, my_i);   // (indices local to the bank)
    } else if (threadIdx.x < k) {
      my_s[threadIdx.x] = RG_NEG_INF;
      my_i[threadIdx.x] = INT64_MAX;
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) ticket_s = atomicAdd(done + o, 1);
    __syncthreads();
    if (ticket_s != SL - 1) continue;  // (workgroup-uniform)
    __threadfence();
    if (w == 0) {  // the query's last slice: SL k <= 512 partial winners, eight slots per lane
      float s8[8];
      int id8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = lane + 64 * u;
        s8[u] = RG_NEG_INF;
        id8[u] = INT_MAX;
        if (e < SL * k) {
          const int64_t at = ((int64_t)o * SL + e / k) * LW + e % k;
          const int64_t pv = __builtin_nontemporal_load(part_i + at);
          if (pv < INT_MAX) {
            s8[u] = __builtin_nontemporal_load(part_s + at);
            id8[u] = (int)pv;
          }
        }
      }
      wave_select<8, (LW > 64 ? 128 : 64)>(s8, id8, k, lane, idx_base, out_s + b * k, out_i + b * k);
    }
  }
}
