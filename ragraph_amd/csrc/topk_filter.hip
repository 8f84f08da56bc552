// Exact cosine top-k through a bf16 MFMA filter  (SimilarityFunctions.py:6-16 + ToyGraphBase.py:66-67, any batch size
// against banks of >= 64 k keys; D = 64 is the edge flavour's RAGraph_edge/modules/RAGraph.py:298-324).
//
// The fp32 tile kernel (topk_cosine.hip) spends 2·B·N·D fp32 MFMA flops; the bf16 matrix cores are 16x faster.  This
// path returns the SAME bits with most of the work on them:
//   1. a first lower bound theta[q] of the final k-th best exact score of q.  Banks of >= 8192 keys: the BOUND pass --
//      this file's kernel over a prefix of the bank, recording per query the best approximate score of each of G = 4 k
//      parts (a handful of queries: k); the parts' best keys are distinct, so k keys score at least (the k-th largest of
//      those maxima) - eps(q).  Smaller banks: the k-th score of an exact top-k over the first n0 keys (the fp32 tile
//      kernel, or up to 16384 queries a score slab + topk_rows).
//   2. filter (this file, bf16 MFMA): approximate scores s~ = bf16(q)·bf16(key), fp32 accumulate, over the next, larger
//      part of the bank.  With q^ = q + dq, k^ = k + dk: |s~ - s| <= |dq||k| + |q||dk| + |dq||dk| + accumulation error
//      (Cauchy-Schwarz) <= eps(q), computed from the query's actual |dq| and the bank's largest |dk| (<= 2^-7 in the worst
//      case, ~0.003 typically) -- a bound for EVERY pair.  A key of the exact top-k has s >= theta[q], hence
//      s~ >= theta[q] - eps(q): every key that passes goes to the query's candidate list; nothing else can be in the result.
//   3. rescoring: the exact score of every candidate as the fp32 fmaf chain in natural k order from +0 (one lane per
//      candidate) -- the chain the f32 MFMA and the oracle compute, so the same bits -- merged with the previous level's
//      winners, canonical top-k (score descending, index ascending).  That is the exact top-k of everything seen so far
//      and a tighter theta for the next level.  The schedule (n0, one to three levels) depends on the batch size:
//      filter_schedule() below, readable through ragraph_topk_cosine_filtered_plan.
// A query whose candidate list overflows its capacity (adversarial banks: thousands of keys within eps of the k-th
// best) is recomputed by an exact fp32 scan of the bank ON THE DEVICE (exact_scan_query: inside the sliced rescoring
// launch for <= 64 queries; otherwise topk_overflow_fixup_kernel, one launch behind the last level that cuts the scans of
// a few queries into key slices); *overflow only counts those rows.  The call never synchronises and reads nothing back.
// Levels may run on an int8 copy of the bank instead (v_mfma_i32_16x16x64_i8, integer thresholds: filter_common.h), whose
// candidate lists can carry the integer score that admitted each key (SCORED: topk_rescore_scored_kernel).
// One entry, three list widths (filter_list_width(k)): the MFMA kernels know no k and are the same launches for every k; the
// kernels that carry a list (filter_rescore.h, filter_verify_fixup.h) run in their LW = 32 instantiations for k <= 32, LW = 64
// for 33 .. 64, and LW = 128 for 65 .. 128, in which a wave holds two entries of a list per lane; plain lists only there
// (filter_scored_lists refuses k > 64).
//
// Two filter kernels share one bank layout (filter_common.h: MFMA fragment order of v_mfma_f32_16x16x32_bf16):
// topk_filter_direct_kernel (topk_filter_direct.hip) for up to 256 queries, and this file's RING kernel above that:
// workgroup = 8 waves x 64 queries = 512 queries (x 32 = 256, x 128 = 1024 at D = 64 on long streams); a wave keeps its
// queries as QW/16 groups of B operands (D/8 VGPRs each) and streams the bf16 bank (2 D bytes per key) through a 4-slot
// LDS ring of 32 KiB stages (64 / 128 / 256 keys at D = 256 / 128 / 64) filled by LDS-DMA, one 1-KiB block per
// global_load_lds_dwordx4 -- the LDS image is the HBM image, conflict-free for the lanes' ds_read_b128 -- handed over by
// FULL/FREE counters.  One fragment read feeds QW/16 MFMAs.  Candidates leave the MFMA stream through wave-private LDS
// buffers (branch-free pass masks, ballot + mbcnt positions) and reach the per-query lists in global memory in flushes.
// Work plan: segment_plan.h with zero warm-up cost (there are no lists): every workgroup gets the same number of stages.
#include "filter_common.h"
#include "rescore_common.h"
#include <new>
#include "segment_plan.h"
#include <cmath>
#include <type_traits>

namespace ragraph {

typedef __attribute__((address_space(3))) void lds_void_f;
typedef int i32x4 __attribute__((ext_vector_type(4)));

template <int D_>
struct FilterCfg {
  static constexpr int D = D_;
  static constexpr int WAVES = 8, THREADS = 512;
  static constexpr int ROW_BYTES = D * 2;                 // one bf16 key
  static constexpr int CR = D / 8;                        // 16-B chunks per row
  static constexpr int KSTEPS = D / 16;                   // 1-KiB blocks (A fragments) per 32-key sub-tile: 2 halves x KS32
  static constexpr int KS32 = D / 32;                     // MFMA k-steps (32 elements) per sub-tile: 8 / 4 / 2
  static constexpr int STAGE_BYTES = FILTER_STAGE_BYTES;
  static constexpr int STAGE_KEYS = STAGE_BYTES / ROW_BYTES;  // 64 / 128 / 256
  static constexpr int SUBS = STAGE_KEYS / 32;            // 32-key MFMA sub-tiles per stage: 2 / 4 / 8
  static constexpr int NSTEP = SUBS * KSTEPS;             // = 32 fragment steps (x QW/16 query groups) per stage for every D
  static constexpr int SLOTS = 4;                         // 128 KiB of ring; the hand-over protocol needs >= 3 slots
  static constexpr int DMAS = STAGE_BYTES / 1024 / WAVES; // 1 KiB DMA instructions per wave and stage = 4
  static constexpr int RPI = 1024 / ROW_BYTES;            // key rows per DMA instruction: 2 / 4 / 8
  static constexpr int CAND_BUF = 480;                    // entries of a wave's candidate buffer (8 B each)
  static constexpr size_t LDS_BYTES = (size_t)SLOTS * STAGE_BYTES + 64 + (size_t)WAVES * CAND_BUF * 8;
};
static_assert(FilterCfg<256>::NSTEP == 32 && FilterCfg<128>::NSTEP == 32 && FilterCfg<64>::NSTEP == 32, "32 steps per stage");

struct FilterParams {
  const float* Qn;        // [B,D] normalised queries (fp32)
  const uint16_t* Kb;     // bf16 keys in MFMA fragment order (filter_common.h), rows >= N zero
  FilterThr thr;          // how a query's pass threshold theta[q] - eps(q) is obtained (filter_common.h)
  int* count;             // [B][cstride] candidate slots reserved so far (filter_count_stride)
  int cstride;
  const uint16_t* Qb;     // queries as bf16 B operands in fragment order (padded to 32s), or NULL: convert from Qn
  int* cand;              // [B,cap] candidate key indices (local to this shard)
  int64_t B, N;           // N = end of the key range (keys >= N never pass)
  int cap;
  int64_t stage_base;     // first stage of the key range this launch filters
  int64_t qtiles, nstages_total;  // nstages_total = stages in the range
  int xcd_map, wgs_per_group, lb_min, depth[2];  // the launch's plan (segment_plan.h): RingWalker's mode, W, lb_min, depth0 / depth1
  int partner_lead;       // > 0: a wave's priority follows its SIMD partner's progress (see the stage loop); 0: off
  // bound pass (BOUND kernels): per query, the maxima of `ngroups` consecutive stage ranges of the launch's key range
  int* gmax;              // [B, ngroups] as order-preserving ints (f2ord), pre-filled with f2ord(-inf)
  int ngroups;
  FilterGate gate;        // a repair level behind a tight bound: returns at once unless the soft-miss count opens it
};

__device__ __forceinline__ void fring_wait(unsigned* ctr, unsigned target) {
  while (__hip_atomic_load(ctr, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < target) __builtin_amdgcn_s_sleep(1);
}
#ifndef RG_RING_RELAXED
#define RG_RING_RELAXED 1
#endif
// What a signal publishes is ordered by hand: `freec` (this wave is done READING the slot) follows the wave's own ds_reads in
// the LDS queue, which executes a wave's operations in order; `full` (this wave's share of the stage has LANDED) follows an
// explicit s_waitcnt vmcnt(0).  A release fence here would wait for every outstanding store of a candidate flush as well.
// The COMPILER must keep that order too: the asm ds_read / s_waitcnt statements in front of a signal carry no memory
// clobber, so an empty asm with one pins the relaxed atomic behind them (no instruction, no wait).
__device__ __forceinline__ void fring_signal(unsigned* ctr, int lane) {
  asm volatile("" ::: "memory");
  if (lane == 0) __hip_atomic_fetch_add(ctr, 1u, RG_RING_RELAXED ? __ATOMIC_RELAXED : __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

#include "filter_copies.h"

#include "filter_prepare.h"

#include "filter_ring.h"

#include "filter_rescore.h"

#include "filter_verify_fixup.h"

static int filter_device_cus() { return device_cus_multiple_of_8(); }  // per device (common.h)

}  // namespace ragraph

using namespace ragraph;

// Optional timing of the filter kernel alone (bench.py's roofline): events recorded around its launches on the caller's
// stream, into a CALLER-OWNED object attached to the calling thread (no process-global state: the attachment is
// thread-local, like the int8 cap).
struct ragraph_filter_profile {
  hipEvent_t ev[2 * 4];  // three filter levels + the bound pass (slot 3)
  int have, bound;
  int i8[4];
  int64_t keys[4];
};
static thread_local ragraph_filter_profile* t_prof = nullptr;
extern "C" ragraph_filter_profile* ragraph_filter_profile_create(void) {
  ragraph_filter_profile* p = new (std::nothrow) ragraph_filter_profile();
  if (!p) {
    set_error("profile: out of memory");
    return nullptr;
  }
  for (int i = 0; i < 2 * 4; ++i)
    if (hipEventCreate(&p->ev[i]) != hipSuccess) {
      for (int j = 0; j < i; ++j) (void)hipEventDestroy(p->ev[j]);
      delete p;
      set_error("profile: cannot create events");
      return nullptr;
    }
  return p;
}
extern "C" void ragraph_filter_profile_destroy(ragraph_filter_profile* p) {
  if (!p) return;
  if (t_prof == p) t_prof = nullptr;
  for (int i = 0; i < 2 * 4; ++i) (void)hipEventDestroy(p->ev[i]);
  delete p;
}
extern "C" ragraph_filter_profile* ragraph_filter_profile_attach(ragraph_filter_profile* p) {
  ragraph_filter_profile* old = t_prof;
  t_prof = p;
  if (p) p->have = p->bound = 0;
  return old;
}
// Milliseconds the filter kernel ran in the most recent call recorded into `p` (its launches summed; synchronises with
// them), or a negative number if none was timed.
extern "C" float ragraph_filter_profile_last_ms(ragraph_filter_profile* p) {
  if (!p || !p->have) return -1.f;
  float total = 0.f;
  if (p->bound) {
    float ms = 0.f;
    if (hipEventSynchronize(p->ev[7]) != hipSuccess || hipEventElapsedTime(&ms, p->ev[6], p->ev[7]) != hipSuccess) return -1.f;
    total += ms;
  }
  for (int l = 0; l < p->have; ++l) {
    float ms = 0.f;
    if (hipEventSynchronize(p->ev[2 * l + 1]) != hipSuccess || hipEventElapsedTime(&ms, p->ev[2 * l], p->ev[2 * l + 1]) != hipSuccess)
      return -1.f;
    total += ms;
  }
  return total;
}

// Per launch of the most recent call: slot 0..2 = the filter levels, slot 3 = the bound pass.  ms_host[s] (negative: no such
// launch), i8_host[s] = 1 if the level ran on the int8 copy, keys_host[s] = keys it covered.  Host arrays of 4 entries.
extern "C" int ragraph_filter_profile_levels(ragraph_filter_profile* p, float* ms_host, int* i8_host, int64_t* keys_host) {
  RG_REQUIRE(p && ms_host && i8_host && keys_host, RAGRAPH_EINVAL, "profile: null pointer");
  for (int s_ = 0; s_ < 4; ++s_) {
    ms_host[s_] = -1.f;
    i8_host[s_] = p->i8[s_];
    keys_host[s_] = p->keys[s_];
    const bool have = s_ == 3 ? p->bound != 0 : s_ < p->have;
    if (!have) continue;
    float ms = 0.f;
    if (hipEventSynchronize(p->ev[2 * s_ + 1]) == hipSuccess && hipEventElapsedTime(&ms, p->ev[2 * s_], p->ev[2 * s_ + 1]) == hipSuccess)
      ms_host[s_] = ms;
  }
  return RAGRAPH_OK;
}

#include "filter_schedule.h"

// A caller that knows its bank (ragraph_amd/kernels_index.py: the copy's measured error, or a call that overflowed) caps
// the int8 levels (filter_schedule.h: filter_i8_levels) of ITS thread's following calls: -1 = the library's rule, 0 = none.
// Thread-local: no shared state.
static thread_local int t_max_i8_levels = -1;
// A SPECULATIVE first bound for the calling thread's following filtered calls (NaN = none, the default): the owner of a bank
// that has answered many queries knows where their k-th best scores lie (the statistics words of every call), and a call
// that starts from theta = prior for every query needs no bound pass -- filter_verify_prior_kernel proves each query's
// answer afterwards and sends the (rare) misses to the exact scan, so the result is exact whatever the prior is.
static thread_local float t_prior = __builtin_nanf("");
extern "C" float ragraph_topk_cosine_filtered_set_prior(float theta_prior) {
  const float old = t_prior;
  t_prior = theta_prior;
  return old;
}
extern "C" int ragraph_topk_cosine_filtered_max_i8_levels(int n) {
  const int old = t_max_i8_levels;
  t_max_i8_levels = n < 0 ? -1 : n;
  return old;
}
// A TIGHT speculative bound on top of the prior (NaN = none, the default): see filter_call_plan and filter_verify_fixup.h.
static thread_local float t_tight = __builtin_nanf("");
extern "C" float ragraph_topk_cosine_filtered_set_tight_prior(float t) {
  const float old = t_tight;
  t_tight = t;
  return old;
}
int ragraph::filter_thread_i8_cap() { return t_max_i8_levels; }  // (topk_small.hip: the single-launch call honours the same cap)
float ragraph::filter_thread_prior() { return t_prior; }
int ragraph::launch_overflow_fixup(int D, const float* Qn, const float* Kn, int64_t N, int k, int64_t idx_base, const int* count,
                                   const int* list, float* out_s, int64_t* out_i, int* done, float* part_s, int64_t* part_i,
                                   int64_t B, void* stream) {
  hipStream_t st = as_stream(stream);
#define RG_FIX(D_)                                                                                                          \
  hipLaunchKernelGGL(topk_overflow_fixup_kernel<D_>, dim3(256), dim3(256), 0, st, Qn, Kn, N, k, idx_base, count, list,       \
                     (int64_t*)nullptr, out_s, out_i, done, part_s, part_i, B, (const unsigned char*)nullptr, (int*)nullptr)
  if (D == 256) RG_FIX(256);
  else if (D == 128) RG_FIX(128);
  else RG_FIX(64);
#undef RG_FIX
  RG_CHECK_LAUNCH("overflow fixup");
  return RAGRAPH_OK;
}

static bool filter_dim_ok(int D) { return D == 64 || D == 128 || D == 256; }

extern "C" int ragraph_keys_to_bf16(const float* Kn, int64_t N, int D, uint16_t* Kb, void* stream) {
  RG_REQUIRE(Kn && Kb, RAGRAPH_EINVAL, "keys_to_bf16: null pointer");
  RG_REQUIRE(N >= 1, RAGRAPH_EINVAL, "keys_to_bf16: N=%lld must be >= 1", (long long)N);
  RG_REQUIRE(filter_dim_ok(D), RAGRAPH_EUNSUPPORTED, "keys_to_bf16: D=%d not in {64,128,256}", D);
  RG_REQUIRE(aligned16(Kn) && aligned16(Kb), RAGRAPH_EINVAL, "keys_to_bf16: pointers must be 16-B aligned");
  const int64_t npad = filter_round_up(N);
  unsigned* tail = reinterpret_cast<unsigned*>(Kb + npad * D);  // the extra row: max_k |dk|^2 as float bits
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(tail, 0, (size_t)D * sizeof(uint16_t), st) != hipSuccess) {
    set_error("keys_to_bf16: memset failed");
    return RAGRAPH_EDEVICE;
  }
  const dim3 grid((unsigned)cdiv(npad * (D / 8), 256));
  if (D == 256) hipLaunchKernelGGL(keys_to_bf16_kernel<256>, grid, dim3(256), 0, st, Kn, N, npad, Kb, tail);
  else if (D == 128) hipLaunchKernelGGL(keys_to_bf16_kernel<128>, grid, dim3(256), 0, st, Kn, N, npad, Kb, tail);
  else hipLaunchKernelGGL(keys_to_bf16_kernel<64>, grid, dim3(256), 0, st, Kn, N, npad, Kb, tail);
  RG_CHECK_LAUNCH("keys_to_bf16");
  // the int8 copy behind it (filter_common.h): the granules' largest |k_i| -> the cut and the two scales, then quantise + lay out
  const FilterI8View v8 = filter_i8_view(Kb, N, D);
  signed char* Kb8 = const_cast<signed char*>(v8.K8);
  unsigned* tail8 = const_cast<unsigned*>(v8.tail8);
  if (hipMemsetAsync(tail8, 0, (size_t)D * sizeof(uint16_t) + filter_i8_table_bytes(N, D), st) != hipSuccess) {
    set_error("keys_to_bf16: memset failed");
    return RAGRAPH_EDEVICE;
  }
  float* gmax = const_cast<float*>(v8.gmax);
  unsigned* cls = const_cast<unsigned*>(v8.cls);
  const dim3 gridg((unsigned)v8.granules);
  if (D == 256) hipLaunchKernelGGL(i8_granule_absmax_kernel<256>, gridg, dim3(256), 0, st, Kn, N, gmax, tail8);
  else if (D == 128) hipLaunchKernelGGL(i8_granule_absmax_kernel<128>, gridg, dim3(256), 0, st, Kn, N, gmax, tail8);
  else hipLaunchKernelGGL(i8_granule_absmax_kernel<64>, gridg, dim3(256), 0, st, Kn, N, gmax, tail8);
  static const float lambda = [] {   // (experiments: RAGRAPH_I8_ONE_SCALE=1 -- the single scale of rounds 3 / 4; RAGRAPH_I8_CUT_LAMBDA)
    const char* e = getenv("RAGRAPH_I8_ONE_SCALE");
    if (e && e[0] == '1') return 0.f;
    const char* l = getenv("RAGRAPH_I8_CUT_LAMBDA");
    return l ? (float)atof(l) : 60.f;
  }();
  hipLaunchKernelGGL(i8_cut_kernel, dim3(1), dim3(1024), 0, st, gmax, v8.granules, D, lambda, tail8);
  const dim3 grid8((unsigned)cdiv(npad * (D / 16), 256));
  if (D == 256) hipLaunchKernelGGL(keys_to_i8_kernel<256>, grid8, dim3(256), 0, st, Kn, N, npad, Kb8, tail8, gmax, cls);
  else if (D == 128) hipLaunchKernelGGL(keys_to_i8_kernel<128>, grid8, dim3(256), 0, st, Kn, N, npad, Kb8, tail8, gmax, cls);
  else hipLaunchKernelGGL(keys_to_i8_kernel<64>, grid8, dim3(256), 0, st, Kn, N, npad, Kb8, tail8, gmax, cls);
  RG_CHECK_LAUNCH("keys_to_bf16(int8 copy)");
  return RAGRAPH_OK;
}

// rows of D uint16: the bf16 copy padded to whole ring stages + one row that carries the bank's largest rounding error,
// then the int8 copy (half as many rows) + one row with its largest error and its scale
constexpr int64_t FILTER_COPY_SLACK_ROWS = 256;  // rows of 2 D bytes: >= 16 KB at any supported D
extern "C" int64_t ragraph_keys_bf16_rows(int64_t N) {
  if (N < 1) return 0;
  const int64_t npad = filter_round_up(N);
  // + FILTER_COPY_SLACK_ROWS: at D = 64 a stage of the int8 copy is 512 keys, so the last stage of a bank padded to an odd
  // multiple of 256 keys reads 16 KB past the copy's rows (keys >= N never pass): the buffer must own those bytes
  // + the int8 copy's granule table (filter_i8_table_bytes: < 5 bytes per 32 KiB of int8 rows, i.e. per 64 rows of 2 D bytes at
  // most -- whatever D)
  return npad + 1 + npad / 2 + 1 + (npad / 4096 + 8) + FILTER_COPY_SLACK_ROWS;
}

extern "C" int ragraph_topk_cosine_filtered_cap(int k) { return FILTER_LIST_CAP; }

constexpr size_t FILTER_STATS_BYTES = 256;  // (the statistics block plus the slack that aligns it)
extern "C" size_t ragraph_topk_cosine_filtered_stats_offset(size_t ws_bytes) {
  return ws_bytes < FILTER_STATS_INTS * sizeof(int) ? 0 : (ws_bytes - FILTER_STATS_INTS * sizeof(int)) & ~(size_t)15;
}

// Everything one call keeps in its workspace behind level 0's scratch.
struct FilterWs {
  float* Qn;            // [B,D] normalised queries
  uint16_t* Qb;         // (B <= FILTER_QB_MAX_B) the same as bf16 B operands in fragment order, padded to whole groups of 32
  float* eq;            // [B] |dq|
  int* count;           // [B][filter_count_stride(B)] candidate slots reserved in the current level (per sub-list)
  unsigned char* flag;  // [B] the list overflowed at an earlier level
  int* cand;            // [B,cap] candidate keys
  int* gmax;            // [B, FILTER_BOUND_PARTS_MAX] part maxima of the bound pass
  float* theta;         // [B] the first bound
  int* overflow_list;   // [B] queries the final level sends to the exact fallback
  int* fix_done;        // [FILTER_FIX_MAX_Q] tickets, [.. x FILTER_FIX_SLICES x 32] partial winners of the sliced fallback scans
                        // (lists of 64: half the slices x 64 winners, the same bytes; lists of 128: a quarter x 128)
  float* fix_s;
  int64_t* fix_i;
  float* part_s;        // (B <= 64) sliced rescoring: [B][8][k] partial winners
  int* part_i;
  float* eq8;           // [B] |dq| of the int8 rounding, [B] the query's int8 scale (int8 levels)
  float* qscale;
  signed char* Qb8;     // (B <= FILTER_QB_MAX_B) the queries as int8 B operands in fragment order, padded to whole groups of 32
};

static size_t filter_ws_carve(char* w, const FilterShape& in, const FilterCall& c, FilterWs* out) {
  const int64_t B = in.B;
  const int D = in.D, k = in.k;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* ptr = w ? w + off : nullptr;
    off += align_up(bytes, 256);
    return ptr;
  };
  FilterWs f;
  f.Qn = reinterpret_cast<float*>(take((size_t)B * D * sizeof(float)));
  f.Qb = B <= FILTER_QB_MAX_B ? reinterpret_cast<uint16_t*>(take((size_t)((B + 31) / 32 * 32) * D * sizeof(uint16_t))) : nullptr;
  f.eq = reinterpret_cast<float*>(take((size_t)B * sizeof(float)));
  f.count = reinterpret_cast<int*>(take((size_t)B * filter_count_stride(B) * sizeof(int)));
  f.flag = reinterpret_cast<unsigned char*>(take((size_t)B));
  // (a call that may keep scored lists -- {key, I} -- gets 8 bytes per slot)
  f.cand = reinterpret_cast<int*>(take(filter_cand_bytes(B, c.cap, c.scored_slots ? sizeof(int2) : sizeof(int), D, k)));
  f.gmax = reinterpret_cast<int*>(take((size_t)B * filter_bound_parts(k, INT64_MAX, 256) * sizeof(int)));
  f.theta = reinterpret_cast<float*>(take((size_t)B * sizeof(float)));
  f.overflow_list = reinterpret_cast<int*>(take((size_t)B * sizeof(int)));
  f.fix_done = reinterpret_cast<int*>(take((size_t)FILTER_FIX_MAX_Q * sizeof(int)));
  f.fix_s = reinterpret_cast<float*>(take((size_t)FILTER_FIX_MAX_Q * FILTER_FIX_SLICES * 32 * sizeof(float)));
  f.fix_i = reinterpret_cast<int64_t*>(take((size_t)FILTER_FIX_MAX_Q * FILTER_FIX_SLICES * 32 * sizeof(int64_t)));
  f.part_s = B <= 64 ? reinterpret_cast<float*>(take((size_t)B * 8 * k * sizeof(float))) : nullptr;
  f.part_i = B <= 64 ? reinterpret_cast<int*>(take((size_t)B * 8 * k * sizeof(int))) : nullptr;
  f.eq8 = reinterpret_cast<float*>(take((size_t)B * sizeof(float)));
  f.qscale = reinterpret_cast<float*>(take((size_t)B * sizeof(float)));
  f.Qb8 = B <= FILTER_QB_MAX_B ? reinterpret_cast<signed char*>(take((size_t)((B + 31) / 32 * 32) * D)) : nullptr;
  if (out) *out = f;
  return off;
}

// ---- the host queries: readers of the call plan ---------------------------------------------------------------------
// The one argument check of the plan's readers and of the call: 0, or the error code of a shape no filtered call takes.
static int filter_shape_code(int64_t B, int64_t N, int D, int k) {
  if (!filter_dim_ok(D)) return RAGRAPH_EUNSUPPORTED;
  return B >= 1 && N >= 1 && k >= 1 && k <= RAGRAPH_TOPK_FILTER_MAX && k <= N ? RAGRAPH_OK : RAGRAPH_EINVAL;
}
// The list width a call of k keys runs at: the LW instantiation of the list-carrying kernels.
static int filter_list_width(int k) {
  return k <= 32 ? 32 : (k <= 64 ? 64 : 128);
}
#define RG_REQUIRE_FILTER_SHAPE(who, B, N, D, k)                                                                      \
  do {                                                                                                                \
    const int code__ = filter_shape_code(B, N, D, k);                                                                 \
    RG_REQUIRE(code__ != RAGRAPH_EUNSUPPORTED, RAGRAPH_EUNSUPPORTED, who ": D=%d not in {64,128,256}", D);           \
    RG_REQUIRE(code__ == RAGRAPH_OK, RAGRAPH_EINVAL, who ": bad B/N/k");                                              \
  } while (0)

// The shape a query asks about: one bank of N rows, or the largest of n_shards shards, without a prior.
static FilterShape filter_query_shape(int64_t B, int64_t N, int D, int k, int n_shards, bool exchange) {
  return {B, N, N, D, k, n_shards, exchange, __builtin_nanf(""), -1, false, filter_env(), filter_device_cus(), __builtin_nanf("")};
}
// The plan queries follow the thread's two bounds when BOTH are set and the tight one lies above the prior (the plan of a call
// under a tight bound); any other setting reports the plan without a prior, as ever.
static void filter_query_follow_tight(FilterShape& in) {
  if (t_prior == t_prior && t_tight == t_tight && t_tight > t_prior) {
    in.prior = t_prior;
    in.tight = t_tight;
  }
}

// A call may replace the planned bound pass by an exact level 0 (a shard shorter than twice the prefix, a shard's share of
// a pooled sample): the size covers whichever of the two needs more, and run_filtered checks the plan it really runs
// against ws_bytes before carving.
static size_t filter_workspace_bytes(FilterShape in, const FilterSchedule& sc) {
  const FilterCall planned = filter_call_plan(in, sc);
  in.exact_level0 = true;
  const FilterCall exact0 = filter_call_plan(in, sc);
  return (planned.level0_bytes > exact0.level0_bytes ? planned.level0_bytes : exact0.level0_bytes) +
         filter_ws_carve(nullptr, in, planned, nullptr) + FILTER_STATS_BYTES;
}
static size_t filter_workspace_bytes(int64_t B, int64_t N, int D, int k, int n_shards) {
  if (B < 1 || N < 1 || k < 1 || n_shards < 1 || !filter_dim_ok(D)) return 0;
  const FilterShape in = filter_query_shape(B, N, D, k, n_shards, n_shards > 1);
  return filter_workspace_bytes(in, filter_schedule(in));
}

// Everything an entry may be asked to hold -- what the size queries report and what filtered_entry insists on.  `own`: the size
// of the single bank's schedule at this k (filter_workspace_bytes(B, plan_N, D, k, 1): the caller has it, or its schedule).
// The floor rule: a list of 33 .. 128 keys needs no less than the same shape at k = 32 (a handful of queries keep 8 sub-lists
// per query while 8 k <= 256 and 4 beyond: the lists alone would make k = 33 the smaller call), a list of 65 .. 128 no less
// than at k = 64 -- a buffer sized for a call serves every shorter list of the same shape.  With an exchange: the schedule
// of n_shards shards that pool their first sample (another level-0 scratch), and a short shard's exact top-k.
static size_t filter_entry_bytes(size_t own, int64_t B, int64_t plan_N, int D, int k, int n_shards, bool exchange) {
  size_t need = own;
  auto at_least = [&](size_t bytes) {
    if (bytes > need) need = bytes;
  };
  if (k > 32 && plan_N >= 32) at_least(filter_workspace_bytes(B, plan_N, D, 32, 1));
  if (k > 64) at_least(filter_workspace_bytes(B, plan_N, D, 64, 1));
  if (exchange) {
    if (n_shards > 1) at_least(filter_workspace_bytes(B, plan_N, D, k, n_shards));
    at_least(ragraph_topk_cosine_workspace_bytes(B, plan_N, D, k));
  }
  return need;
}

// (k <= 32 is answered without the shape check, as ever: a size also where k > N)
extern "C" size_t ragraph_topk_cosine_filtered_workspace_bytes(int64_t B, int64_t N, int D, int k) {
  if (k > 32 && filter_shape_code(B, N, D, k) != RAGRAPH_OK) return 0;
  return filter_entry_bytes(filter_workspace_bytes(B, N, D, k, 1), B, N, D, k, 1, false);
}
// The sharded entry plans for (plan_N, n_shards): its first sample can be another one than the single bank's of plan_N rows
// (exchange = NULL runs the single-bank schedule: the `own` term).
extern "C" size_t ragraph_topk_cosine_filtered_sharded_workspace_bytes(int64_t B, int64_t plan_N, int D, int k, int n_shards) {
  if (!filter_dim_ok(D)) return 0;  // (ragraph_topk_cosine_f32 alone takes other widths)
  return filter_entry_bytes(filter_workspace_bytes(B, plan_N, D, k, 1), B, plan_N, D, k, n_shards, true);
}

// How many trailing levels of the plan run on the int8 copy, under the calling thread's cap (0 for a shape the entry refuses).
extern "C" int ragraph_topk_cosine_filtered_i8_levels(int64_t B, int64_t N, int D, int k) {
  if (filter_shape_code(B, N, D, k) != RAGRAPH_OK) return 0;
  FilterShape in = filter_query_shape(B, N, D, k, 1, false);
  in.i8_cap = t_max_i8_levels;
  filter_query_follow_tight(in);
  return filter_call_plan(in, filter_schedule(in)).i8_levels;
}

extern "C" int ragraph_topk_cosine_filtered_plan(int64_t B, int64_t N, int D, int k, int64_t plan[7]) {
  RG_REQUIRE(plan, RAGRAPH_EINVAL, "topk_cosine_filtered_plan: null pointer");
  RG_REQUIRE_FILTER_SHAPE("topk_cosine_filtered_plan", B, N, D, k);
  FilterShape in = filter_query_shape(B, N, D, k, 1, false);
  filter_query_follow_tight(in);
  // (the plan of one whole bank IS its schedule: filter_schedule leaves such a bank bound_keys <= N / 4 or <= ends[0] < N / 2
  // and n0 <= N, so filter_call_plan's adjustments to a shard's own length change none of the words below)
  const FilterCall c = filter_call_plan(in, filter_schedule(in));
  plan[0] = c.n0;
  plan[1] = c.level0 == FILTER_L0_BOUND ? 2 : (c.level0 == FILTER_L0_SLAB ? 1 : 0);
  plan[2] = c.nlev;
  for (int l = 0; l < FILTER_MAX_LEVELS; ++l) plan[3 + l] = l < c.nlev ? c.level[l].key1 : 0;
  plan[6] = c.bound_keys;
  return c.nlev;
}

// Would a sharded call of this shape speculate under a prior?  (Any valid one: the answer is the plan's, not the value's.)
extern "C" int ragraph_topk_cosine_filtered_sharded_speculates(int64_t B, int64_t plan_N, int D, int k, int n_shards) {
  if (filter_shape_code(B, plan_N, D, k) != RAGRAPH_OK || k > 32 || n_shards < 1) return 0;   // (no exchange beyond 32 keys)
  FilterShape in = filter_query_shape(B, plan_N, D, k, n_shards, true);
  in.prior = 0.f;
  return filter_call_plan(in, filter_schedule(in)).spec ? 1 : 0;
}

// The plan of a ring launch (segment_plan.h: ring_plan_choose walks every workgroup of two plans), kept per thread for the
// shapes it last saw: a call's launches repeat from call to call, and a launch must not simulate 256 workgroups every time.
static RingPlan ring_plan_cached(int64_t qtiles, int64_t NS, int CUS, int lb_min) {
  struct Entry {
    int64_t qtiles, NS;
    int CUS, lb_min;
    RingPlan pl;
  };
  constexpr int SLOTS = 16;
  thread_local Entry cache[SLOTS];
  thread_local int used = 0, victim = 0;
  for (int i = 0; i < used; ++i)
    if (cache[i].qtiles == qtiles && cache[i].NS == NS && cache[i].CUS == CUS && cache[i].lb_min == lb_min) return cache[i].pl;
  const RingPlan pl = ring_plan_choose(qtiles, NS, CUS, lb_min);
  const int at = used < SLOTS ? used++ : (victim = (victim + 1) % SLOTS);
  cache[at] = Entry{qtiles, NS, CUS, lb_min, pl};
  return pl;
}

// Ring-kernel launch shared by the filter levels and the bound pass (B > 256: the direct kernel takes smaller batches).
template <int D, int QW, bool BOUND, bool I8 = false, bool SCORED = false, bool PIPE = false, bool SKEW = false>
static int launch_ring(FilterParams p, int64_t B, int CUS, int prof_slot, hipStream_t st) {
  using C = FilterCfg<I8 ? D / 2 : D>;
  p.qtiles = cdiv(B, (int64_t)C::WAVES * QW);
  // shortest piece of a key stream a workgroup takes: 8 stages when there is work for everybody, fewer on short launches
  // (a bound pass of 18 stages x 6 query tiles gave 14 workgroups 8 stages each and 242 nothing: 19 us of stage loop where
  // 108 workgroups need 2.5; tools/check_segment_plan.cpp covers lb_min = 1)
  {
    const int64_t per_wg = p.qtiles * p.nstages_total / CUS;
    p.lb_min = per_wg >= 16 ? 8 : (per_wg >= 8 ? 4 : (per_wg >= 3 ? 2 : 1));
  }
  const RingPlan pl = ring_plan_cached(p.qtiles, p.nstages_total, CUS, p.lb_min);
  p.xcd_map = pl.mode;
  p.wgs_per_group = CUS / (pl.mode == RING_ONE ? 1 : 8);
  p.depth[0] = pl.depth[0];
  p.depth[1] = pl.depth[1];
  static DeviceOnce lds_once;  // per template instance and device (common.h)
  if (hipError_t e = raise_dynamic_lds(lds_once, &topk_filter_kernel<D, QW, BOUND, I8, SCORED, PIPE, SKEW>, (int)C::LDS_BYTES); e != hipSuccess) {
    set_error("topk_cosine_filtered: cannot raise dynamic LDS limit: %s", hipGetErrorString(e));
    return RAGRAPH_EDEVICE;
  }
  if (t_prof && prof_slot >= 0) (void)hipEventRecord(t_prof->ev[2 * prof_slot], st);
  hipLaunchKernelGGL((topk_filter_kernel<D, QW, BOUND, I8, SCORED, PIPE, SKEW>), dim3((unsigned)CUS), dim3(C::THREADS), C::LDS_BYTES, st, p);
  if (t_prof && prof_slot >= 0) (void)hipEventRecord(t_prof->ev[2 * prof_slot + 1], st);
  RG_CHECK_LAUNCH("topk_cosine_filtered(filter)");
  ring_stamps_report(BOUND, I8);
  if (prof_slot >= 0) ring_timing_report(prof_slot, D);
  return RAGRAPH_OK;
}

// Which kernel one pass over keys [key0, key1) of a bank copy runs -- a filter level, or the bound pass (bound): the direct
// kernel up to 256 queries (topk_filter_direct.hip: the stream, not the matrix work, is what such a call costs), more the
// ring kernel with qw = 64 queries per wave (four groups of 16), 96 or 128.
struct PassVariant {
  bool direct;
  int qw;
  bool bound, i8, scored, pipe, skew;
};
static PassVariant filter_pass_variant(int D, int64_t B, int64_t key0, int64_t key1, bool bound, bool int8, bool scored, int cus,
                                       const FilterEnv& env) {
  PassVariant v{};
  v.qw = 64;
  v.bound = bound;
  v.i8 = int8;
  v.scored = int8 && scored;
  if (B <= 256) {
    v.direct = true;
    return v;
  }
  // (an int8 level: the ring kernel over the int8 copy, stages of twice as many keys)
  const int64_t nstages = cdiv(key1 - key0, FILTER_STAGE_BYTES / ((int8 ? 1 : 2) * D));
  auto long_stream = [&](int64_t tile) { return cdiv(B, tile) * nstages >= 32 * (int64_t)cus; };
  if (!int8) {
    // D = 64: short rows leave registers for four query groups per wave (qw = 128): half the LDS reads and ring hand-overs per
    // MFMA (the edge flavour's D).  From 1024 queries (one full tile), and only where a workgroup keeps its 1024 queries for
    // a long stream: on a short bank the larger tiles mean fewer, shorter segments, each paying the operand loads again --
    // 8192 x 40000 x 64: 0.58 vs 0.46 ms
    if (!bound && D == 64 && B >= 1024 && long_stream(1024)) v.qw = 128;
    return v;
  }
  // int8 operands are 16 bytes per 64 elements: SIX query groups per wave (tile = 768 queries) fit the registers four
  // bf16 groups take (224 VGPRs, no scratch), and an A fragment then feeds six MFMAs, a stage 3072 cycles of them
  // between two ring hand-overs: the bench's last level 14.45 -> 13.8 ms (A/B on one box, profiles/r3_i8_ab.txt).
  // Eight groups (tile = 1024) spill (256 VGPRs + 80 B of scratch): 14.2 ms.  Long streams only, and only where the
  // larger tile does not add padding queries (the last tile of 4096 queries would be a third full).
  const int64_t pad64 = cdiv(B, (int64_t)512) * 512 - B;
  auto fits = [&](int64_t tile) {  // a long stream per workgroup, and at most 2 % more padding queries than tiles of 512
    return long_stream(tile) && (cdiv(B, tile) * tile - B - pad64) * 50 <= B;
  };
  // (D = 64: eight groups are 32 registers of operands -- no spill -- and 65 536 x 4M x 64 runs 15.5 ms against 16.3 with
  // six and 17.0 with four)
  const int qw = env.i8_qw ? env.i8_qw : (D == 64 && fits(1024) ? 128 : (fits(768) ? 96 : 64));
  const bool long128 = qw == 128 && long_stream(1024), long96 = qw == 96 && long_stream(768);
  // D = 256, four groups per wave: the epilogue of a sub-tile inside the next one's MFMAs (PIPE: 222 VGPRs) -- 512 x 1M 0.213 ->
  // 0.2005 ms, 1024 0.324 -> 0.308, 4096 1.053 -> 1.026, 16 384 3.53 -> 3.49; on the long streams that take six groups
  // it only draws level (13.03 vs 13.03 - 13.13 ms: six groups in one set of accumulators stay).  RAGRAPH_FILTER_PIPE=0/2: A/B
  if (D == 256 && ((env.pipe == 1 && !long128 && !long96) || env.pipe == 2)) v.pipe = true;
  else v.qw = long128 ? 128 : (long96 ? 96 : 64);
  // D = 256, six groups: the two sets' epilogues under each other's MFMAs (filter_ring.h, SKEW: 3 vector instructions between a
  // set's last MFMA and the next MFMA instead of 17) -- 100 000 x 1M: the launch 16.30 -> 15.98 ms, the step 17.92 -> 17.61
  // (three interleaved pairs, profiles/ring_group_skew.txt).  RAGRAPH_FILTER_SKEW=0: one decision per sub-tile -- A/B and tests
  v.skew = D == 256 && !v.pipe && v.qw == 96 && env.skew != 0;
  return v;
}

// The ring kernel's instantiations: the bound pass and the bf16 levels at 64 queries per wave (D = 64: also 128), the int8
// levels at 64 / 96 / 128 with plain or scored lists, and at D = 256 the pipelined form of 64 and the skewed form of 96.
template <int D>
static int launch_ring_variant(const PassVariant& v, const FilterParams& p, int64_t B, int cus, int prof_slot, hipStream_t st) {
  RG_REQUIRE(!v.direct && (v.qw == 64 || (v.i8 ? !v.pipe && (v.qw == 96 || v.qw == 128) : D == 64 && !v.bound && v.qw == 128)) &&
             (!v.pipe || (D == 256 && v.i8)), RAGRAPH_EINVAL, "topk_cosine_filtered: no ring kernel for D=%d qw=%d bound=%d int8=%d pipe=%d",
             D, v.qw, (int)v.bound, (int)v.i8, (int)v.pipe);
  if (v.bound) return launch_ring<D, 64, true>(p, B, cus, prof_slot, st);
  if (!v.i8) {
    if constexpr (D == 64)
      if (v.qw == 128) return launch_ring<D, 128, false>(p, B, cus, prof_slot, st);
    return launch_ring<D, 64, false>(p, B, cus, prof_slot, st);
  }
  if constexpr (D == 256) {
    if (v.pipe)
      return v.scored ? launch_ring<D, 64, false, true, true, true>(p, B, cus, prof_slot, st)
                      : launch_ring<D, 64, false, true, false, true>(p, B, cus, prof_slot, st);
    if (v.skew)
      return v.scored ? launch_ring<D, 96, false, true, true, false, true>(p, B, cus, prof_slot, st)
                      : launch_ring<D, 96, false, true, false, false, true>(p, B, cus, prof_slot, st);
  }
#define RG_RING_I8(QW_) \
  return v.scored ? launch_ring<D, QW_, false, true, true>(p, B, cus, prof_slot, st) : launch_ring<D, QW_, false, true>(p, B, cus, prof_slot, st)
  if (v.qw == 128) RG_RING_I8(128);
  if (v.qw == 96) RG_RING_I8(96);
  RG_RING_I8(64);
#undef RG_RING_I8
}

// One pass over keys [key0, key1) of the bf16 copy or (int8) of the int8 copy: a filter level (bound_groups = 0: candidates of
// every query whose threshold `thr` describes) or the bound pass (bound_groups part maxima into gmax).  prof_slot < 0: a repair
// launch -- not a level, not timed; `gate`: see FilterGate.
template <int D>
static int run_pass(const FilterWs& f, const uint16_t* Kb, const signed char* Kb8, int64_t B, int64_t key0, int64_t key1,
                    const FilterThr& thr, int cap, int bound_groups, bool int8, bool scored, const FilterEnv& env, int cus,
                    int prof_slot, hipStream_t st, FilterGate gate = FilterGate{nullptr, 0, 0}) {
  const PassVariant v = filter_pass_variant(D, B, key0, key1, bound_groups > 0, int8, scored, cus, env);
  const uint16_t* keys = v.i8 ? reinterpret_cast<const uint16_t*>(Kb8) : Kb;
  // (the queries' operand image of the copy's type; NULL beyond FILTER_QB_MAX_B queries: converted per segment)
  const uint16_t* Qimg = v.i8 ? reinterpret_cast<const uint16_t*>(f.Qb8) : f.Qb;
  if (v.direct) {
    DirectArgs a{};
    a.Qb = Qimg;
    a.Kb = keys;
    a.i8 = v.i8;
    a.scored = v.scored;
    a.B = B;
    a.key0 = key0;
    a.key1 = key1;
    a.thr = thr;
    a.count = f.count;
    a.cand = f.cand;
    a.cap = cap;
    a.nsub = rescore_slices(B, thr.k);
    a.gmax_out = f.gmax;
    a.bound_groups = bound_groups;
    a.gate = gate;
    if (t_prof && prof_slot >= 0) (void)hipEventRecord(t_prof->ev[2 * prof_slot], st);
    const int rc = launch_filter_direct<D>(a, st);
    if (t_prof && prof_slot >= 0) (void)hipEventRecord(t_prof->ev[2 * prof_slot + 1], st);
    return rc;
  }
  const int stage_keys = FILTER_STAGE_BYTES / ((v.i8 ? 1 : 2) * D);  // (bf16: key0 is a multiple of 256)
  RG_REQUIRE(!v.i8 || key0 % stage_keys == 0, RAGRAPH_EINVAL, "topk_cosine_filtered: an int8 level must start at a whole stage "
             "(key %lld, %d keys per stage)", (long long)key0, stage_keys);
  FilterParams p{};
  p.Qn = f.Qn;
  p.Kb = keys;
  p.thr = thr;
  p.count = f.count;
  p.cstride = filter_count_stride(B);
  p.Qb = Qimg;
  p.cand = f.cand;
  p.gmax = bound_groups > 0 ? f.gmax : nullptr;
  p.ngroups = bound_groups;
  p.B = B;
  p.N = key1;
  p.cap = cap;  // (scored lists: {key, I} pairs, the same number of slots -- filter_ws_carve gives them 8 bytes each)
  p.stage_base = key0 / stage_keys;
  p.nstages_total = cdiv(key1 - key0, stage_keys);
  p.partner_lead = env.partner_lead;
  p.gate = gate;
  return launch_ring_variant<D>(v, p, B, cus, prof_slot, st);
}

// Which kernel rescores a level's candidates.
enum RescoreKind {
  RESCORE_SCORED_SMALL,  // scored lists (filter_scored_lists: a large call's int8 level), from 8192 queries
  RESCORE_SCORED,
  RESCORE_WIDE_SLICED,   // a handful of queries: S workgroups per query, each with its sub-list
  RESCORE_WIDE_COOP,     // up to 256 queries: one workgroup per CU, its 70 KB of tiles cost no occupancy
  RESCORE_WIDE,          // too few queries to fill the chip with one wave each
  RESCORE_COOP_FEW,      // one wave per query, rows staged through LDS: 16-row tiles (the later levels over a sharded bank)
  RESCORE_COOP
};
static RescoreKind rescore_kind(int64_t B, int k, bool scored, bool few) {
  if (scored) return B >= 8192 ? RESCORE_SCORED_SMALL : RESCORE_SCORED;
  // the wide kernels up to 2048 queries -- measured: 512 queries 0.39 (wide) vs 0.44 ms, 1024-2048 equal, 4095: 1.98 vs 1.89
  if (B < 2048) return rescore_slices(B, k) > 1 ? RESCORE_WIDE_SLICED : (B <= 256 ? RESCORE_WIDE_COOP : RESCORE_WIDE);
  return few ? RESCORE_COOP_FEW : RESCORE_COOP;
}

// Exact rescoring of a level's candidates (+ merge with the running result when `merge`) and canonical selection.  Every
// kind lists the queries whose list overflowed for topk_overflow_fixup_kernel (scan_n = 0: the one-wave-per-query kernels'
// own wave scanning a million keys took 94 ms).
// SKIP (run_tight_repair's final launch alone, and only with idx_base == 0): the kernels' form that returns on an empty list of
// an unflagged query -- the merge would rewrite the row it read (filter_rescore.h).
template <int D, int LW, bool SKIP = false>
static int run_rescore(const FilterWs& f, const float* Kn, int64_t N, int64_t B, int cap, int k, int64_t idx_base, int merge,
                       int final_level, float* out_scores, int64_t* out_idx, int* overflow, RescoreKind kind, const FilterThr& thr,
                       int* cstat, hipStream_t st) {
  if constexpr (SKIP)
    RG_REQUIRE(merge && final_level && idx_base == 0 && !cstat, RAGRAPH_EINVAL, "topk_cosine_filtered: not a launch that may skip rows");
  const float* ps = merge ? out_scores : nullptr;
  const int64_t* pi = merge ? out_idx : nullptr;
  const int cs = filter_count_stride(B);
  const int64_t scan_n = 0;
#define RG_SCORED(SMALL_)                                                                                                        \
  hipLaunchKernelGGL((topk_rescore_scored_kernel<D, SMALL_, LW, SKIP>), dim3((unsigned)cdiv(B, 2)), dim3(128), 0, st, f.Qn, Kn, f.count,    \
                     reinterpret_cast<const int2*>(f.cand), B, cap, cs, k, idx_base, ps, pi, final_level, out_scores, out_idx,   \
                     overflow, f.overflow_list, f.flag, scan_n, thr, cstat)
#define RG_WIDE(SLICED_, COOP_, GRID_, PART_S_, PART_I_)                                                                         \
  hipLaunchKernelGGL((topk_rescore_wide_kernel<D, SLICED_, COOP_, LW, SKIP && !(SLICED_) && !(COOP_)>), GRID_, dim3(256), 0, st, f.Qn, Kn, f.count, f.cand, B, N,    \
                     cap, cs, k, idx_base, ps, pi, final_level, out_scores, out_idx, overflow, f.overflow_list, f.flag, PART_S_, \
                     PART_I_, cstat)
#define RG_COOP(FEW_)                                                                                                            \
  hipLaunchKernelGGL((topk_rescore_coop_kernel<D, 32, FEW_, (LW > 64 ? 128 : 64), SKIP && !(FEW_)>), dim3((unsigned)cdiv(B, 2)), dim3(128), 0, st, f.Qn, Kn, f.count,    \
                     f.cand, B, cap, cs, k, idx_base, ps, pi, final_level, out_scores, out_idx, overflow, f.overflow_list,       \
                     f.flag, scan_n, cstat)
  switch (kind) {
    case RESCORE_SCORED_SMALL:
    case RESCORE_SCORED:
      if constexpr (LW <= 64) {
        if (kind == RESCORE_SCORED_SMALL) RG_SCORED(true);
        else RG_SCORED(false);
      } else {  // (filter_scored_lists refuses k > 64: no plan asks for this)
        set_error("topk_cosine_filtered: no scored rescoring for lists of more than 64 keys");
        return RAGRAPH_EUNSUPPORTED;
      }
      break;
    case RESCORE_WIDE_SLICED:
      RG_WIDE(true, true, dim3((unsigned)B, (unsigned)rescore_slices(B, k)), f.part_s, f.part_i);
      wide_timing_report();
      break;
    case RESCORE_WIDE_COOP: RG_WIDE(false, true, dim3((unsigned)B), (float*)nullptr, (int*)nullptr); break;
    case RESCORE_WIDE: RG_WIDE(false, false, dim3((unsigned)B), (float*)nullptr, (int*)nullptr); break;
    case RESCORE_COOP_FEW:   // (the later levels of a sharded bank: no call of 65 .. 128 keys is sharded, and at this kernel's 128
                             // registers the two-entries-per-lane form would spill)
      if constexpr (LW <= 64) {
        RG_COOP(true);
      } else {
        set_error("topk_cosine_filtered: no 16-row rescoring for lists of more than 64 keys");
        return RAGRAPH_EUNSUPPORTED;
      }
      break;
    case RESCORE_COOP: RG_COOP(false); break;
  }
#undef RG_SCORED
#undef RG_WIDE
#undef RG_COOP
  RG_CHECK_LAUNCH("topk_cosine_filtered(rescore)");
  return RAGRAPH_OK;
}

// The arguments of ragraph_topk_cosine_filtered_sharded_f32 (the single bank: plan_N = N, no exchange, one shard).
struct FilteredArgs {
  const float* Q;
  int64_t B;
  const float *Kn, *Kp;
  const uint16_t* Kb;
  int64_t N;
  int D, k;
  int64_t idx_base;
  float* out_scores;
  int64_t* out_idx;
  int* overflow;
  int64_t* overflow_idx;
  void* ws;
  size_t ws_bytes;
  void* stream;
  int64_t plan_N;  // (from here on: the sharded entry's)
  float* theta;
  ragraph_exchange_fn exchange;
  void* ctx;
  int n_shards;
};

// theta = (first: =, else max with) the k-th exact score of the running result thr.prev_scores
static int launch_theta(FilterThr thr, int64_t B, int first, float* theta, hipStream_t st) {
  thr.gmax = nullptr;
  thr.theta = nullptr;
  hipLaunchKernelGGL(filter_theta_kernel, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, st, thr, B, first, theta);
  RG_CHECK_LAUNCH("topk_cosine_filtered(theta)");
  return RAGRAPH_OK;
}

// A shard too short for the plan's phases (FilterCall::exact_participant): its fp32 top-k once, offered at every exchange.
static int run_exact_participant(const FilteredArgs& a, const FilterCall& c) {
  hipStream_t st = as_stream(a.stream);
  RG_REQUIRE(a.ws_bytes >= ragraph_topk_cosine_workspace_bytes(a.B, a.N, a.D, a.k), RAGRAPH_EWORKSPACE,
             "topk_cosine_filtered: workspace too small for a short shard's exact top-k");
  int rc = ragraph_topk_cosine_bank_f32(a.Q, a.B, a.Kn, a.D == 256 ? a.Kp : nullptr, a.N, a.D, a.k, a.idx_base, a.out_scores,
                                        a.out_idx, a.ws, a.ws_bytes, a.stream);
  if (rc != RAGRAPH_OK) return rc;
  if (hipMemsetAsync(a.overflow, 0, sizeof(int), st) != hipSuccess) {
    set_error("topk_cosine_filtered: memset failed");
    return RAGRAPH_EDEVICE;
  }
  FilterThr t0{};
  t0.prev_scores = a.out_scores;
  t0.k = a.k;
  for (int ph = c.first_phase; ph < c.nlev; ++ph) {   // phase 0 (not under a speculative bound) + one exchange behind every level but the last
    if ((rc = launch_theta(t0, a.B, ph == c.first_phase, a.theta, st)) != RAGRAPH_OK) return rc;
    a.exchange(a.ctx, ph);
  }
  return RAGRAPH_OK;
}

// The 256-query repair's buffers, carved from the idle span [f.cand, f.theta) of the call's workspace (filter_call_plan's
// workspace rule guarantees filter_repair_bytes of it).
struct FilterRepairWs {
  FilterWs f;        // what run_pass / run_rescore read of a call of FILTER_REPAIR_Q queries
  int* list;         // [256] row numbers of the soft misses
  float* Q;          // [256, D] their raw rows
  float* theta;      // [256] their bounds
  float* out_s;      // [256, k] the repaired rows (local indices)
  int64_t* out_i;
  int* dummy;        // (the prepare launch's *overflow = 0)
};
static FilterRepairWs filter_repair_carve(const FilterWs& f, int D, int k, bool int8, size_t slot_bytes) {
  char* w = reinterpret_cast<char*>(f.cand);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* ptr = w + off;
    off += align_up(bytes, 256);
    return ptr;
  };
  const size_t q = FILTER_REPAIR_Q;
  FilterRepairWs r{};
  r.f.cand = reinterpret_cast<int*>(take(q * FILTER_LIST_CAP * slot_bytes));
  r.Q = reinterpret_cast<float*>(take(q * D * sizeof(float)));
  r.f.Qn = reinterpret_cast<float*>(take(q * D * sizeof(float)));
  if (int8) r.f.Qb8 = reinterpret_cast<signed char*>(take(q * D));
  else r.f.Qb = reinterpret_cast<uint16_t*>(take(q * D * sizeof(uint16_t)));
  r.f.count = reinterpret_cast<int*>(take(q * FILTER_COUNT_STRIDE * sizeof(int)));
  r.out_s = reinterpret_cast<float*>(take(q * k * sizeof(float)));
  r.out_i = reinterpret_cast<int64_t*>(take(q * k * sizeof(int64_t)));
  r.list = reinterpret_cast<int*>(take(q * sizeof(int)));
  r.theta = reinterpret_cast<float*>(take(q * sizeof(float)));
  r.f.eq = reinterpret_cast<float*>(take(q * sizeof(float)));
  r.f.eq8 = reinterpret_cast<float*>(take(q * sizeof(float)));
  r.f.qscale = reinterpret_cast<float*>(take(q * sizeof(float)));
  r.f.flag = reinterpret_cast<unsigned char*>(take(q));
  r.dummy = reinterpret_cast<int*>(take(sizeof(int)));
  r.f.theta = r.theta;
  r.f.overflow_list = f.overflow_list;   // (never written: the repair's rescoring is not a final one)
  r.f.fix_done = f.fix_done;
  return r;
}

// Step 6b of a call under a tight bound (the comment block in filter_verify_fixup.h tells the whole story).
template <int D, int LW>
static int run_tight_repair(const FilteredArgs& a, const FilterCall& c, const FilterShape& in, const FilterWs& f, FilterThr thr,
                            const signed char* K8, int* stats, hipStream_t st) {
  const int64_t B = a.B, N = a.N;
  const int k = a.k;
  const FilterLevel& lv = c.level[c.nlev - 1];
  const size_t slot = c.scored_slots ? sizeof(int2) : sizeof(int);
  RG_REQUIRE((size_t)(reinterpret_cast<char*>(f.theta) - reinterpret_cast<char*>(f.cand)) >= filter_repair_bytes(D, k, slot),
             RAGRAPH_EWORKSPACE, "topk_cosine_filtered: the repair's buffers do not fit the idle lists");
  const FilterRepairWs r = filter_repair_carve(f, D, k, lv.int8, slot);
  hipLaunchKernelGGL(filter_tight_verdict_kernel, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, st, a.out_scores, a.out_idx, B, k,
                     in.tight, in.prior, f.flag, f.theta, r.list, stats);
  RG_CHECK_LAUNCH("topk_cosine_filtered(soft verdict)");
  // 1 .. 256 soft misses: a compact call of the direct kernel
  hipLaunchKernelGGL(filter_repair_gather_kernel<D>, dim3(FILTER_REPAIR_Q), dim3(64), 0, st, a.Q, f.theta, r.list, r.Q, r.theta, stats);
  RG_CHECK_LAUNCH("topk_cosine_filtered(repair gather)");
  hipLaunchKernelGGL((filter_prep_kernel<D, 1>), dim3(FILTER_REPAIR_Q / 4), dim3(256), 0, st, r.Q, (int64_t)FILTER_REPAIR_Q, r.f.Qn,
                     r.f.eq, r.f.count, r.f.flag, r.dummy, (int*)nullptr, k, r.f.Qb, filter_count_stride(FILTER_REPAIR_Q),
                     lv.int8 ? r.f.eq8 : nullptr, r.f.qscale, r.f.Qb8, r.f.fix_done, (int*)nullptr, FilterStatsInit{},
                     (float*)nullptr, 0.f);
  RG_CHECK_LAUNCH("topk_cosine_filtered(repair prepare)");
  FilterThr thr2 = thr;
  thr2.theta = r.theta;
  thr2.prev_scores = nullptr;
  thr2.gmax = nullptr;
  thr2.eq = r.f.eq;
  thr2.eq8 = r.f.eq8;
  thr2.qscale = r.f.qscale;
  thr2.flag = r.f.flag;
  int rc = run_pass<D>(r.f, a.Kb, K8, FILTER_REPAIR_Q, 0, N, thr2, FILTER_LIST_CAP, 0, lv.int8, c.repair_scored, in.env, in.cus, -1, st,
                       FilterGate{stats + 22, 1, FILTER_REPAIR_Q});
  if (rc != RAGRAPH_OK) return rc;
  rc = run_rescore<D, LW>(r.f, a.Kn, N, FILTER_REPAIR_Q, FILTER_LIST_CAP, k, 0, 0, 0, r.out_s, r.out_i, r.dummy,
                      rescore_kind(FILTER_REPAIR_Q, k, c.repair_scored, false), thr2, nullptr, st);
  if (rc != RAGRAPH_OK) return rc;
  hipLaunchKernelGGL((filter_repair_scatter_kernel<(LW > 64 ? 128 : 64)>), dim3(FILTER_REPAIR_Q), dim3(64), 0, st, r.list, r.out_s, r.out_i, r.f.flag, k,
                     a.out_scores, a.out_idx, f.flag, stats);
  RG_CHECK_LAUNCH("topk_cosine_filtered(repair scatter)");
  // more than 256: one more level for everybody (proven queries carry theta = +inf)
  thr.theta = f.theta;
  thr.gmax = nullptr;
  thr.prev_scores = a.out_scores;
  rc = run_pass<D>(f, a.Kb, K8, B, 0, N, thr, c.cap, 0, lv.int8, lv.scored, in.env, in.cus, -1, st,
                   FilterGate{stats + 22, FILTER_REPAIR_Q + 1, INT_MAX});
  if (rc != RAGRAPH_OK) return rc;
  // the call's final rescoring: the level's lists (empty unless it ran) merged with the running rows.  Without an index
  // base a query with an empty list and no flag keeps its row as it is, and its wave returns before reading anything else
  if (a.idx_base == 0 && in.env.final_skip)
    return run_rescore<D, LW, true>(f, a.Kn, N, B, c.cap, k, 0, 1, 1, a.out_scores, a.out_idx, a.overflow,
                                    rescore_kind(B, k, lv.scored, false), thr, nullptr, st);
  return run_rescore<D, LW>(f, a.Kn, N, B, c.cap, k, a.idx_base, 1, 1, a.out_scores, a.out_idx, a.overflow,
                        rescore_kind(B, k, lv.scored, false), thr, nullptr, st);
}

// Steps 3 - 7 of a call (1, 2: filtered_entry): executes the plan `c` that filter_call_plan made of the shape `in` -- carve,
// prepare, first bound, the levels, verify / fixup -- and decides nothing itself.
template <int D, int LW>
static int run_filtered(const FilteredArgs& a, const FilterCall& c, const FilterShape& in) {
  hipStream_t st = as_stream(a.stream);
  const int64_t B = a.B, N = a.N;
  const int k = a.k;
  float* const out_scores = a.out_scores;
  int64_t* const out_idx = a.out_idx;
  const bool sharded = a.exchange != nullptr, bound = c.level0 == FILTER_L0_BOUND;
  static const int ablate = [] {  // RAGRAPH_FILTER_ABLATE=1: no key passes the filter (timing only, results invalid)
    const char* e = getenv("RAGRAPH_FILTER_ABLATE");
    return e ? atoi(e) : 0;
  }();
  if (t_prof) t_prof->have = t_prof->bound = 0;

  // 3. carve: level 0's scratch, the call's buffers, the statistics words
  char* w = static_cast<char*>(a.ws);
  FilterWs f;
  const size_t used = c.level0_bytes + filter_ws_carve(w + c.level0_bytes, in, c, &f) + FILTER_STATS_BYTES;
  RG_REQUIRE(used <= a.ws_bytes, RAGRAPH_EWORKSPACE, "topk_cosine_filtered: the schedule of this call needs %zu bytes of workspace, "
             "%zu given", used, a.ws_bytes);
  // the call's candidate statistics: the last FILTER_STATS_INTS ints of the workspace AS PASSED (ragraph_topk_cosine_filtered_stats_offset)
  int* stats = reinterpret_cast<int*>(w + ragraph_topk_cosine_filtered_stats_offset(a.ws_bytes));
  const unsigned* max_kerr2 = reinterpret_cast<const unsigned*>(a.Kb + filter_round_up(N) * D);
  // the int8 copy lies behind the bf16 copy and its tail row (ragraph_keys_to_bf16)
  const FilterI8View v8 = filter_i8_view(a.Kb, N, D);

  // 4. prepare -- one launch: normalised queries, their bf16 rounding errors, empty lists, clear flags (+ group maxima at -inf;
  // under a speculative bound theta = the prior)
  FilterStatsInit stats_init{};
  stats_init.nlev = c.nlev;
  for (int l = 0; l < c.nlev; ++l) {
    stats_init.i8[l] = c.level[l].int8;
    const int64_t lk = c.level[l].key1 - c.level[l].key0;
    stats_init.keys[l] = lk > INT_MAX ? INT_MAX : (int)lk;
  }
  // (the zero-query count: every workgroup of the prepare launch adds to it, so it is zeroed in front of the launch)
  if (hipMemsetAsync(stats + 15, 0, sizeof(int), st) != hipSuccess) {
    set_error("topk_cosine_filtered: memset failed");
    return RAGRAPH_EDEVICE;
  }
#define RG_PREP(R_)                                                                                                                     \
  hipLaunchKernelGGL((filter_prep_kernel<D, R_>), dim3((unsigned)cdiv(B <= FILTER_QB_MAX_B ? (B + 31) / 32 * 32 : B, 4 * (R_))), dim3(256), 0, st, a.Q, B, \
                     f.Qn, f.eq, f.count, f.flag, a.overflow, bound ? f.gmax : nullptr, c.parts, c.bf16_image ? f.Qb : nullptr,         \
                     filter_count_stride(B), c.i8_levels > 0 ? f.eq8 : nullptr, f.qscale, B <= FILTER_QB_MAX_B ? f.Qb8 : nullptr, f.fix_done, \
                     stats, stats_init, c.spec ? (sharded ? a.theta : f.theta) : nullptr, c.tight ? in.tight : in.prior)
  if (B >= 8192) RG_PREP(4);   // (100 000 x 256: 120 us with one row per wave, 74 with two or four, 162 with eight)
  else RG_PREP(1);
#undef RG_PREP
  RG_CHECK_LAUNCH("topk_cosine_filtered(prepare)");

  FilterThr thr{};   // (theta, prev_scores, gmax: per launch)
  thr.eq = f.eq;
  thr.max_kerr2 = max_kerr2;
  thr.eq8 = f.eq8;
  thr.qscale = f.qscale;
  thr.tail8 = v8.tail8;
  thr.cls8 = v8.cls;
  thr.flag = f.flag;
  thr.k = k;
  thr.ngroups = c.parts;
  thr.ablate = ablate;
  // 5. the first bound: group maxima of a bf16 pass over a prefix, or an exact level 0 over the first n0 keys (out_scores /
  // out_idx hold every level's running result, local indices)
  int rc = RAGRAPH_OK;
  switch (c.level0) {
    case FILTER_L0_NONE: break;  // (nothing to compute: the prepare launch has written theta)
    case FILTER_L0_BOUND:
      rc = run_pass<D>(f, a.Kb, v8.K8, B, 0, c.bound_keys, thr, c.cap, c.parts, false, false, in.env, in.cus, 3, st);
      if (t_prof) {
        t_prof->bound = 1;
        t_prof->i8[3] = 0;
        t_prof->keys[3] = c.bound_keys;
      }
      break;
    case FILTER_L0_SLAB: {
      float* S = reinterpret_cast<float*>(w);  // one slab of scores, reused: written and read back while it is in cache
      for (int64_t b0 = 0; b0 < B && rc == RAGRAPH_OK; b0 += FILTER_SLAB_MAX_B) {
        const int64_t nb = B - b0 < FILTER_SLAB_MAX_B ? B - b0 : FILTER_SLAB_MAX_B;
        rc = ragraph_linear_f32(f.Qn + b0 * D, nb, D, a.Kn, c.n0, nullptr, RAGRAPH_ACT_NONE, 0.f, S, a.stream);
        if (rc == RAGRAPH_OK)
          rc = ragraph_topk_rows_f32(S, nb, c.n0, c.n0, k, out_scores + b0 * k, out_idx + b0 * k, a.stream);
      }
      break;
    }
    case FILTER_L0_TILE:
      rc = ragraph_topk_cosine_bank_f32(a.Q, B, a.Kn, D == 256 ? a.Kp : nullptr, c.n0, D, k, 0, out_scores, out_idx, a.ws,
                                        c.level0_bytes, a.stream);
      break;
  }
  if (rc != RAGRAPH_OK) return rc;
  if (sharded && c.spec) {  // theta = the prior on every shard (the prepare launch wrote it): nothing to pool, no phase 0
    thr.theta = a.theta;
  } else if (sharded) {  // the first bound leaves through theta / out_scores, and comes back as a bound on the k-th best of ALL shards
    thr.gmax = bound ? f.gmax : nullptr;
    thr.prev_scores = out_scores;
    if (bound) {  // k lower bounds of distinct keys' exact scores, descending, where a level leaves its exact top-k
      hipLaunchKernelGGL(filter_bound_scores_kernel<2>, dim3((unsigned)cdiv(B, 4)), dim3(256), 0, st, thr, B, out_scores, a.theta);
      RG_CHECK_LAUNCH("topk_cosine_filtered(theta)");
    } else if ((rc = launch_theta(thr, B, 1, a.theta, st)) != RAGRAPH_OK) {
      return rc;
    }
    a.exchange(a.ctx, 0);
    thr.theta = a.theta;
  } else if (bound && c.parts > k) {  // theta = the k-th largest of the part maxima, minus eps
    thr.gmax = f.gmax;
    if constexpr (LW > 64)   // (up to 256 parts: four per lane)
      hipLaunchKernelGGL(filter_bound_scores_kernel<4>, dim3((unsigned)cdiv(B, 4)), dim3(256), 0, st, thr, B, (float*)nullptr, f.theta);
    else
      hipLaunchKernelGGL(filter_bound_scores_kernel<2>, dim3((unsigned)cdiv(B, 4)), dim3(256), 0, st, thr, B, (float*)nullptr, f.theta);
    RG_CHECK_LAUNCH("topk_cosine_filtered(theta)");
  }

  // 6. the levels: filter, rescore (+ merge with the running result), sharpen the bound for the next one
  for (int l = 0; l < c.nlev; ++l) {
    const FilterLevel& lv = c.level[l];
    thr.gmax = (l == 0 && bound && !sharded && c.parts == k) ? f.gmax : nullptr;  // (k parts: the minimum, inline)
    if (!sharded) thr.theta = (c.spec || (l == 0 && bound && c.parts > k)) ? f.theta : nullptr;
    thr.prev_scores = out_scores;
    rc = run_pass<D>(f, a.Kb, v8.K8, B, lv.key0, lv.key1, thr, c.cap, 0, lv.int8, lv.scored, in.env, in.cus, l, st);
    if (t_prof) {
      t_prof->i8[l] = lv.int8;
      t_prof->keys[l] = lv.key1 - lv.key0;
    }
    if (rc != RAGRAPH_OK) return rc;
    if (t_prof) t_prof->have = l + 1;
    rc = run_rescore<D, LW>(f, a.Kn, N, B, c.cap, k, a.idx_base, l > 0, l == c.level_final, out_scores, out_idx, a.overflow,
                        rescore_kind(B, k, lv.scored, sharded && l > 0), thr, stats + 2 + l, st);
    if (rc != RAGRAPH_OK) return rc;
    if (l + 1 == c.nlev) break;
    if (sharded) {  // this shard's k-th exact score so far sharpens theta; then the other shards'
      if ((rc = launch_theta(thr, B, 0, a.theta, st)) != RAGRAPH_OK) return rc;
      a.exchange(a.ctx, 1 + l);
    } else if (c.spec) {  // the next level filters with max(prior, the exact k-th best so far)
      if ((rc = launch_theta(thr, B, 0, f.theta, st)) != RAGRAPH_OK) return rc;
    }
  }

  // 6b. a tight bound: the soft verdict and the repair (filter_verify_fixup.h), every launch enqueued unconditionally
  if (c.tight && (rc = run_tight_repair<D, LW>(a, c, in, f, thr, v8.K8, stats, st)) != RAGRAPH_OK) return rc;

  // 7. verify / fixup
  if (c.spec && !sharded) {   // (a shard's lists prove nothing alone: the owner of a row verifies the MERGED k-th best)
    hipLaunchKernelGGL(filter_verify_prior_kernel, dim3((unsigned)cdiv(B, 256 * FILTER_VERIFY_ROWS)), dim3(256), 0, st, out_scores, B, k, in.prior, 1, f.flag,
                       a.overflow, f.overflow_list, stats, c.tight ? in.tight : 0.f, c.tight ? (in.tight - in.prior) / 16.f : 0.f);
    RG_CHECK_LAUNCH("topk_cosine_filtered(verify)");
  }
  // overflowed queries (none on ordinary banks) and the queries a prior was too high for: exact fp32 scan on the device --
  // no host read-back
  hipLaunchKernelGGL((topk_overflow_fixup_kernel<D, LW>), dim3(256), dim3(256), 0, st, f.Qn, a.Kn, N, k, a.idx_base,
                     a.overflow, f.overflow_list, a.overflow_idx, out_scores, out_idx, f.fix_done, f.fix_s, f.fix_i, B, f.flag,
                     sharded ? nullptr : stats);
  RG_CHECK_LAUNCH("topk_cosine_filtered(overflow fallback)");
  return RAGRAPH_OK;
}

// Steps 1 and 2 of a call: validate, plan, and hand the plan to whoever executes it.  The thread's prior and int8 cap and the
// per-call switches are read here and nowhere else.  The schedule (its pow() search) is computed once for a single bank of
// up to 32 keys a list; filter_entry_bytes adds one for each floor (k > 32: k = 32; k > 64: k = 64) and, for a shard among
// several that pool their first sample, the pooled one -- which that shard computes again as the call's own.
// filter_call_plan (cheap arithmetic) runs twice per size, once for the call.
template <int LW>
static int run_filtered_dim(const FilteredArgs& a, const FilterCall& c, const FilterShape& in) {
  if (a.D == 256) return run_filtered<256, LW>(a, c, in);
  if (a.D == 128) return run_filtered<128, LW>(a, c, in);
  return run_filtered<64, LW>(a, c, in);
}
static int filtered_entry(const FilteredArgs& a) {
  const int64_t B = a.B, N = a.N, plan_N = a.plan_N;
  const int D = a.D, k = a.k;
  RG_REQUIRE(a.Q && a.Kn && a.Kb && a.out_scores && a.out_idx && a.overflow && a.ws, RAGRAPH_EINVAL, "topk_cosine_filtered: null pointer");
  RG_REQUIRE(a.n_shards >= 1, RAGRAPH_EINVAL, "topk_cosine_filtered: n_shards=%d", a.n_shards);
  RG_REQUIRE_FILTER_SHAPE("topk_cosine_filtered", B, N, D, k);
  RG_REQUIRE(N < (int64_t)INT_MAX - 1024, RAGRAPH_EUNSUPPORTED, "topk_cosine_filtered: shard rows must fit int32");
  RG_REQUIRE(plan_N >= N && (a.exchange || plan_N - N <= 1024), RAGRAPH_EINVAL, "topk_cosine_filtered: plan_N must be the largest shard's size");
  RG_REQUIRE(!a.exchange || a.theta, RAGRAPH_EINVAL, "topk_cosine_filtered: an exchange needs the theta buffer");
  RG_REQUIRE(aligned16(a.Q) && aligned16(a.Kn) && aligned16(a.Kb) && aligned16(a.ws), RAGRAPH_EINVAL,
             "topk_cosine_filtered: pointers must be 16-B aligned");
  // every call owns at least what the single bank of plan_N rows needs; the schedule behind that size is this call's own
  // unless the call is one of several shards that pool their first sample.  An entry refuses whatever is shorter than its
  // size query reports, whichever schedule this call runs: the same function answers both.
  const FilterShape one = filter_query_shape(B, plan_N, D, k, 1, false);
  const FilterSchedule sc_one = filter_schedule(one);
  const size_t need = filter_entry_bytes(filter_workspace_bytes(one, sc_one), B, plan_N, D, k, a.n_shards, a.exchange != nullptr);
  RG_REQUIRE(a.ws_bytes >= need, RAGRAPH_EWORKSPACE, "topk_cosine_filtered: workspace %zu < %zu", a.ws_bytes, need);
  const FilterShape in{B, N, plan_N, D, k, a.n_shards, a.exchange != nullptr, t_prior, t_max_i8_levels, false, one.env, one.cus, t_tight};
  const FilterCall c = filter_call_plan(in, a.exchange && a.n_shards > 1 ? filter_schedule(in) : sc_one);
  if (c.exact_participant) return run_exact_participant(a, c);
  switch (filter_list_width(k)) {   // (widest first: the order the kernels are instantiated in, and so their labels, stays)
    case 128: return run_filtered_dim<128>(a, c, in);
    case 64: return run_filtered_dim<64>(a, c, in);
    default: return run_filtered_dim<32>(a, c, in);
  }
}

extern "C" int ragraph_topk_cosine_filtered_f32(const float* Q, int64_t B, const float* Kn, const float* Kp,
                                                const uint16_t* Kb, int64_t N, int D, int k, int64_t idx_base,
                                                float* out_scores, int64_t* out_idx, int* overflow,
                                                int64_t* overflow_idx, void* ws, size_t ws_bytes, void* stream) {
  return filtered_entry({Q, B, Kn, Kp, Kb, N, D, k, idx_base, out_scores, out_idx, overflow, overflow_idx, ws, ws_bytes, stream,
                         N, nullptr, nullptr, nullptr, 1});
}

extern "C" int ragraph_topk_cosine_filtered_sharded_f32(const float* Q, int64_t B, const float* Kn, const float* Kp,
                                                        const uint16_t* Kb, int64_t N, int D, int k, int64_t idx_base,
                                                        float* out_scores, int64_t* out_idx, int* overflow,
                                                        int64_t* overflow_idx, void* ws, size_t ws_bytes, void* stream,
                                                        int64_t plan_N, float* theta, ragraph_exchange_fn exchange,
                                                        void* ctx, int n_shards) {
  // (no exchange for lists of 33 .. 128 keys: this entry stays at the LW = 32 instantiations, with or without an exchange)
  RG_REQUIRE(k <= 32, RAGRAPH_EINVAL, "topk_cosine_filtered_sharded: an exchange takes lists of up to 32 keys (k=%d)", k);
  return filtered_entry({Q, B, Kn, Kp, Kb, N, D, k, idx_base, out_scores, out_idx, overflow, overflow_idx, ws, ws_bytes, stream,
                         plan_N, theta, exchange, ctx, n_shards});
}

extern "C" int ragraph_verify_merged_prior_f32(const float* merged_scores, int64_t R, int k, float prior, int speculative,
                                               const int* stats_words, const int* overflow, float* out5, void* stream) {
  RG_REQUIRE(out5 && (merged_scores || R == 0), RAGRAPH_EINVAL, "verify_merged_prior: null pointer");
  RG_REQUIRE(R >= 0 && k >= 1, RAGRAPH_EINVAL, "verify_merged_prior: bad R/k");
  hipLaunchKernelGGL(verify_merged_prior_kernel, dim3(1), dim3(256), 0, as_stream(stream), merged_scores, R, k, prior, speculative,
                     stats_words, overflow, out5);
  RG_CHECK_LAUNCH("verify_merged_prior");
  return RAGRAPH_OK;
}

extern "C" int ragraph_theta_sharpen_f32(const float* gathered, int G, int64_t B, int m, int k, float* theta, void* stream) {
  RG_REQUIRE(gathered && theta, RAGRAPH_EINVAL, "theta_sharpen: null pointer");
  RG_REQUIRE(G >= 1 && m >= 1 && k >= 1 && G * m <= 64 && G * m >= k, RAGRAPH_EINVAL,
             "theta_sharpen: need k <= G*m <= 64 (G=%d m=%d k=%d)", G, m, k);
  if (B <= 0) return RAGRAPH_OK;
  if (G * m <= 32 && B >= 4096)
    hipLaunchKernelGGL(theta_sharpen2_kernel, dim3((unsigned)cdiv(B, 8)), dim3(256), 0, as_stream(stream), gathered, G, B, m, k,
                       theta);
  else
    hipLaunchKernelGGL(theta_sharpen_kernel, dim3((unsigned)cdiv(B, 4)), dim3(256), 0, as_stream(stream), gathered, G, B, m, k,
                       theta);
  RG_CHECK_LAUNCH("theta_sharpen");
  return RAGRAPH_OK;
}
