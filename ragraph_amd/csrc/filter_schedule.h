// Host side: what a filtered call decides before it launches anything -- the level schedule (filter_schedule; exported as
// ragraph_topk_cosine_filtered_plan) and the call plan made from it (filter_call_plan).  Host functions without device
// pointers or launches.  filter_call_plan is a pure function of its FilterShape; filter_schedule also reads seven schedule-
// experiment switches, once per process as before (RAGRAPH_FILTER_I8_DIRECT, _I8_DIRECT_D64, _N0DIV, _FORCE_N0, _FORCE_L,
// _I8_CANDF) or per call (_FRACS).
// Part of csrc/topk_filter.hip (textually included there, inside its namespace / after its helpers): split out in round 6 so
// that the ring, the candidate path and the launch plumbing can be read -- and changed -- apart.  No include guard on purpose:
// these are not stand-alone headers.

// Schedule of a call: exact fp32 top-k over the first n0 keys (its k-th score is the first bound), then bf16 filter +
// exact rescoring over [0, e1), [e1, e2), ... [.., N).  A level's k-th exact score is the next level's bound, so a level
// lets through ~1.3 k (its end / the previous end) keys per query.
//   * Large batches (the bench's 100 k queries): n0 = N/256, ends N/32, N/4, N -- ~100, ~100 and ~40 candidates per
//     query; level 0 is the fp32 tile kernel.  The matrix work dominates, three levels keep the rescoring at ~8 %.
//   * Small and medium batches (B <= 16384): a level costs ~60 us whatever it filters (launches, ring prologue, the
//     rescoring kernel's latency) while candidates are cheap, so fewer, steeper levels win; and level 0 is a slab --
//     the dense kernel (same fmaf chains as everything else) writes the B x n0 scores, topk_rows selects -- which
//     spreads over the whole chip where the tile kernel would run one query tile on a few CUs.  n0 and the number of
//     levels minimise   slab(B, n0) + L (60 us + B * 1.3 k r * 0.4 ns),  r = (N / n0)^(1/L),  under 1.3 k r <= cap / 2.
constexpr int FILTER_MAX_LEVELS = 3;
static int64_t filter_round_up(int64_t n) { return (n + FILTER_PAD_KEYS - 1) / FILTER_PAD_KEYS * FILTER_PAD_KEYS; }

struct FilterSchedule {
  int64_t bound_keys;               // > 0: no exact level 0 -- the first bound comes from a bf16 pass over keys [0, bound_keys)
  int64_t n0;                       // level 0: exact top-k over keys [0, n0)   (bound_keys == 0)
  int slab0;                        // level 0 by dense kernel + topk_rows (needs B * n0 floats of workspace)
  int nlev;                         // filter levels
  int64_t ends[FILTER_MAX_LEVELS];  // their ends (multiples of 256 except the last = N)
  int i8_levels;                    // the last i8_levels levels run on the int8 copy (filter_common.h)
};

constexpr int64_t FILTER_SLAB_MAX_B = 16384;
// up to this many queries the prepare launch also leaves the queries as bf16 (and int8) B operands in fragment order: the direct
// kernel's image (<= 256), and the ring kernel's operand load -- 32 independent 16-byte loads per lane instead of eight
// dependent batches of fp32 loads + conversions (13 us per segment at D = 256), which short launches cannot amortise
// (every filtered call: KeyIndex cuts batches at 262 144 queries.  Large batches have long segments on ONE GPU -- the images
// save ~0.7 % of the bench step -- but the short launches of a key-sharded rank do not: the bound launch of one rank of 8
// spent a quarter of its 0.27 ms converting operands.  The images are 3 D bytes per query: 77 MB at 100 000 queries.)
constexpr int64_t FILTER_QB_MAX_B = 262144;
constexpr int64_t FILTER_SLAB_MAX_SCORES = (int64_t)1 << 26;  // 256 MiB of scores

// The switches a call's decisions read.  The first five are flipped BETWEEN calls by tests and A/B runs: read once per call,
// at the entry, and handed down.  The last two are read once per process.
struct FilterEnv {
  int i8;            // RAGRAPH_FILTER_I8 = n: the last n levels run on the int8 copy (0: none); -1: the rule
  int scored;        // RAGRAPH_FILTER_SCORED = 0 / 1: scored candidate lists off / on; -1: the rule
  int pipe;          // RAGRAPH_FILTER_PIPE (filter_pass_variant; default 1)
  int skew;          // RAGRAPH_FILTER_SKEW (filter_pass_variant; default 1; 0: six groups with one decision per sub-tile)
  int partner_lead;  // RAGRAPH_FILTER_PARTNER_LEAD (0 = equal priorities, the hardware's age order; default 1)
  int i8_qw;         // RAGRAPH_FILTER_I8_QW: queries per wave of the int8 levels (0: the rule)
  int scored_shards;    // RAGRAPH_FILTER_SCORED_SHARDS: sharded banks of up to this many shards keep scored lists (default 2)
  int spec_two_shards;  // RAGRAPH_FILTER_SPEC_SHARDS_TWO_LEVELS: from this many shards a three-level plan runs two levels
                        // under a prior (default 2: every sharded bank; 0 = never)
  int tight_levels;     // RAGRAPH_FILTER_TIGHT_LEVELS: levels of a call under a tight bound (default 1; 2: the plan's last two -- A/B)
  int final_skip;       // RAGRAPH_FILTER_FINAL_SKIP: the final rescoring of a call under a tight bound returns on an empty list
                        // (filter_rescore.h: SKIP; default 1; 0: every wave reads and rewrites its row -- A/B)
};
static int filter_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
static FilterEnv filter_env() {
  static const int scored_shards = filter_env_int("RAGRAPH_FILTER_SCORED_SHARDS", 2);
  static const int spec_two_shards = filter_env_int("RAGRAPH_FILTER_SPEC_SHARDS_TWO_LEVELS", 2);
  return {filter_env_int("RAGRAPH_FILTER_I8", -1), filter_env_int("RAGRAPH_FILTER_SCORED", -1), filter_env_int("RAGRAPH_FILTER_PIPE", 1),
          filter_env_int("RAGRAPH_FILTER_SKEW", 1),
          filter_env_int("RAGRAPH_FILTER_PARTNER_LEAD", 1), filter_env_int("RAGRAPH_FILTER_I8_QW", 0), scored_shards, spec_two_shards,
          filter_env_int("RAGRAPH_FILTER_TIGHT_LEVELS", 1), filter_env_int("RAGRAPH_FILTER_FINAL_SKIP", 1)};
}

// Scored candidate lists for the int8 levels (topk_rescore_scored_kernel): calls whose rescoring is bound by the row
// gathers, i.e. the ones that take the one-wave-per-query kernels.
// D = 256 only: measured with / without (ms per call, profiles/r3_scored_ab.txt) 2048 x 1M x 256: 0.874 / 0.836, 16384:
// 4.50 / 4.21, 100 000: 24.4 / 22.8; but 50 000 x 2M x 128: 12.71 / 12.63 and 65 536 x 4M x 64: 15.73 / 15.93 -- shorter rows
// are cheaper to fetch and their scores spread wider against the same eps (fewer extra candidates to prune), so the
// second round only adds latency.
// k <= 16: round 1 is 16 rows and lists beyond 256 entries take the plain path -- 50 000 x 1M x 256 at k = 16: 14.5 / 13.7 ms,
// k = 20: 15.6 / 15.8, k = 32: 18.7 / 20.3.
static bool filter_scored_lists(int64_t B, int D, int k, const FilterEnv& env) {
  // every call of the ring kernel (> 256 queries) ...: a scored list needs so few rows that ONE wave per query beats the
  // four-wave workgroups of the wide kernels even at a few hundred queries, whose single level admits ~380 candidates per
  // query and prunes 90 % of them (257 x 1M x 256: 0.214 -> 0.189 ms, 512: 0.267 -> 0.228, 1024: 0.436 -> 0.377, 1536: 0.580 ->
  // 0.490)
  // ... and the direct kernel's calls of 65 - 256 queries (entries carry ceil(I / 256)): 128 x 1M: 0.111 -> 0.106 ms, 256:
  // 0.148 -> 0.136.  Up to 64 queries the direct kernel keeps several sub-lists per query and several workgroups rescore
  // each: one wave per query measured slower there (one query 0.075 -> 0.080 ms).
  if (B < 65) return false;
  if (k > 64) return false;  // (lists of 65 .. 128 keys: the scored rounds keep a lane per previous winner -- plain lists, whatever
                             // RAGRAPH_FILTER_SCORED says)
  if (env.scored >= 0) return env.scored != 0;
  return D == 256 && k <= 16;
}

// A handful of queries: S workgroups rescore a query (S k <= 256 partial winners for the merge launch), and the direct
// kernel keeps S sub-lists per query, one per rescoring workgroup (filter_common.h: FILTER_COUNT_STRIDE).
static int rescore_slices(int64_t B, int k) {
  int S = B <= 16 ? 8 : (B <= 32 ? 4 : (B <= 64 ? 2 : 1));  // (part_s / part_i exist up to 64 queries)
  while (S > 1 && S * k > 256) S >>= 1;
  return S;
}
constexpr int FILTER_LIST_CAP = 2048;  // (ragraph_topk_cosine_filtered_cap)
// slots of a query's candidate region: one list, or (<= 64 queries) one full-size list per rescoring slice
static int filter_cap(int64_t B, int k) { return FILTER_LIST_CAP * (B <= 64 ? rescore_slices(B, k) : 1); }

// Banks of >= 8192 keys (KeyIndex sends >= 16384) take their first bound from the BOUND pass instead of an
// exact level 0: the filter kernel itself runs over the first bound_keys keys and records, per query, the best approximate
// score of each of k consecutive parts; the smallest of the k maxima, minus eps, bounds the final k-th best from below
// (filter_prepare_kernel).  As a bound it is worth the exact k-th best of ~bound_keys / (ln k + 1) keys, and it costs a
// bf16 pass with no lists, no inserts and no fp32 matrix work: 0.7 ms instead of the tile kernel's 3.2 ms for the
// bench's 100 k queries, 40 us instead of the slab's 110 us for 256.
constexpr int64_t FILTER_BOUND_MIN_KEYS = 8192;

// Parts of the bound pass's prefix: 4 k (at most 128), as many as the prefix has stages (a part is at least one ring stage;
// sub-tiles of the direct kernel are finer), never fewer than k.
static int filter_bound_parts(int k, int64_t bound_keys, int D, int64_t B = 1 << 20, int n_shards = 1) {
  // Lists of 65 .. 128 keys: up to 256 parts (four part maxima per lane of the selection) at every batch size -- 128 parts
  // are exactly k at k = 128, the minimum of k maxima is worth prefix / (ln k + 1) = prefix / 5.9, and a level may have a ratio
  // of at most 6: no schedule would fit between the two.
  if (B <= 64 && k <= 64) return k;  // a handful of queries: the minimum of k part maxima, taken inside the filter launch's prologue
                          // (filter_threshold) -- the extra selection launch would cost more than the shorter prefix saves
  int64_t g = 4 * (int64_t)k;
  if (g > (k > 64 ? 256 : 128)) g = k > 64 ? 256 : 128;
  if (n_shards > 1) g = (g + n_shards - 1) / n_shards;  // (pooled through the exchange: 4 k parts over all shards)
  const int64_t avail = bound_keys == INT64_MAX ? g : bound_keys / (FILTER_STAGE_BYTES / (2 * D));
  if (g > avail) g = avail;
  return (int)(g < k ? k : g);
}
// prefix keys per key of exact sample the bound is worth (see filter_bound_scores_kernel)
// Lists of 65 .. 128 keys have at most 256 parts for k values, fewer than 4 k: the k-th largest of G part maxima over n keys
// sits where a key's tail probability p has G (1 - (1 - p)^(n / G)) = k, i.e. p n = -G ln(1 - k / G), while the exact k-th best
// of n0 keys has p n0 = k: the prefix is worth n0 = n x / -ln(1 - x) keys, x = k / G (x = 1/4: 1.15 and x = 1/2: 1.39 -- the
// 1.2 and 1.5 below), growing to the ln k + 1 of the minimum of k maxima as x -> 1; taken with 10 % of margin.
static double filter_bound_eff(int k, int parts) {
  if (k > 64 && parts < 4 * k) {
    const double worst = log((double)k) + 1.0;
    if (parts <= k) return worst;
    const double x = (double)k / (double)parts, eff = 1.1 * -log(1.0 - x) / x;
    return eff < worst ? (eff > 1.2 ? eff : 1.2) : worst;
  }
  if (parts >= 4 * k || parts >= 128) return 1.2;
  if (parts >= 2 * k) return 1.5;
  return log((double)k) + 1.0;
}

// D = 64: a stage of the int8 copy holds 512 keys (32 KB / 64 B) and a level starts at a whole stage, so the inner level ends
// are multiples of 512 -- a level that started at an odd multiple of 256 would begin with the previous level's last 256
// keys again, and a key listed twice breaks the selection (distinct pairs are what its ranks count).
static void filter_align_ends(FilterSchedule& sc, int D) {
  if (D != 64) return;
  for (int l = 0; l + 1 < sc.nlev; ++l) {
    const int64_t e = sc.ends[l] / 512 * 512;
    if (e >= 512 && (l == 0 || e > sc.ends[l - 1])) sc.ends[l] = e;
  }
  if (sc.bound_keys > sc.ends[0]) sc.bound_keys = sc.ends[0] / FILTER_PAD_KEYS * FILTER_PAD_KEYS;
}

// Everything the decisions of one call depend on.  The entry reads the calling thread's prior and int8 cap and the
// per-call switches ONCE into this; the host queries fill it with what they are asked about.
struct FilterShape {
  int64_t B, N, plan_N;  // N = this shard's rows, plan_N = the largest shard's (one bank: N, up to 1024 rows of slack)
  int D, k, n_shards;
  bool exchange;         // a sharded call: the phases' bounds travel through the caller's exchange
  float prior;           // the thread's speculative first bound (NaN: none)
  int i8_cap;            // the thread's cap on int8 levels (-1: the rule)
  bool exact_level0;     // size queries: the plan if the bound pass gives way to an exact level 0 (see filter_call_plan)
  FilterEnv env;
  int cus;               // filter_device_cus()
  float tight;           // the thread's tight speculative bound (NaN: none; honoured under a valid prior below it only)
};

// Sharded banks of up to this many shards keep the SCORED lists on their int8 levels (and the schedule that goes with them):
// a shard's own round-1 bound comes from 1 / G of the keys while the level's threshold was pooled over all shards' earlier
// levels -- at G = 2 the shard's bound is still the sharper one (half of the bank against a quarter), from G = 4 it is not and
// the second round only adds latency (profiles/r3_emul.txt).  RAGRAPH_FILTER_SCORED_SHARDS (FilterEnv::scored_shards): A/B.
// n_shards > 1 (row-sharded bank, N = the largest shard): the shards pool their first samples through the exchange, so
// the sample is planned for the WHOLE bank and every shard scans its share of the prefix.  (The schedule of in.plan_N keys: in.N plays no part.)
static FilterSchedule filter_schedule(const FilterShape& in) {
  const int64_t B = in.B, N = in.plan_N;
  const int D = in.D, k = in.k, n_shards = in.exchange ? in.n_shards : 1, cus = in.cus;
  const FilterEnv& env = in.env;
  FilterSchedule sc{};
  const int cap = 2048;
  // scored lists (one bank, >= 2048 queries): an int8 level's rescoring fetches about a third of its candidates' rows, which
  // makes int8 pay on EVERY level (the bench step, 2 / 3 int8 levels: 24.3 / 23.85 ms; without the scores 26.9 / 27.7)
  const bool scored = (n_shards == 1 || n_shards <= env.scored_shards) && B >= 2048 && filter_scored_lists(B, D, k, env);  // (below 2048 queries the plain lists' plans
                                                                                   // stay: a smaller first sample measured slower)
  // (the model's price of an int8 candidate under scored lists, relative to the plain lists'; fitted: 0.6 moves 8192+ queries
  // x 1M keys from two levels to three, all int8 -- 8192: 2.37 -> 2.33 ms, 16384: 4.30 -> 4.13 -- while 0.45 also shrank the
  // first sample of 2048 - 8192 queries, which measured 2 - 4 % slower)
  constexpr double scored_cand = 0.6;
  const bool bound = N >= FILTER_BOUND_MIN_KEYS;
  // int8 levels (filter_common.h): D = 128 / 256, the ring kernel's batch sizes, banks long enough to be matrix-bound (an
  // int8 level quantises its queries from the fp32 rows per segment where the bf16 levels of up to 16384 queries load a
  // prepared image -- Cora-sized 2708 x 10 000 x 128: 0.087 -> 0.100 ms)
  // (D = 64, the edge flavour: one MFMA per 16-key half and query group, so the epilogue weighs more -- 65 536 x 4M x 64:
  // 22.5 -> 15.5 ms with eight groups per wave; eps is the same 0.02 but the scores' spread is 1/8: fewer extra candidates)
  // (with the prepared int8 operand image and the scored lists, D = 256 also pays on banks of 32 768+ keys from 2048 queries:
  // 4096 x 40 000: 0.189 -> 0.160 ms, 2100 x 60 000: 0.180 -> 0.150, 16 384 x 50 000: 0.64 -> 0.49; not at D = 128 -- 8192 x
  // 50 000: 0.237 -> 0.244 -- nor on shorter banks -- 8192 x 20 000 x 256: 0.221 -> 0.238)
  const bool i8_ok = (D == 64 || D == 128 || D == 256) && B > 256 &&
                     (N * n_shards >= 65536 || (D == 256 && B >= 2048 && N * n_shards >= 32768));
  const bool mid_i8 = i8_ok && N * n_shards < 65536;
  static const bool i8_direct_env = [] { const char* e = getenv("RAGRAPH_FILTER_I8_DIRECT"); return !e || atoi(e) != 0; }();  // A/B
  // (D = 64, round 5: the edge flavour's calls of up to 256 queries -- half the stream, the scores' spread 1/8 against the
  // same eps; RAGRAPH_FILTER_I8_DIRECT_D64=0: A/B)
  static const bool i8_direct_d64 = [] { const char* e = getenv("RAGRAPH_FILTER_I8_DIRECT_D64"); return !e || atoi(e) != 0; }();
  const bool i8_direct = (D == 128 || D == 256 || (D == 64 && i8_direct_d64)) && B <= 256 && N * n_shards >= 65536 && i8_direct_env;
  // bound_keys / eff_div ~ the exact sample the bound is worth: planned for 4 k parts, corrected below if the prefix is
  // too short for that many
  const double eff_div = filter_bound_eff(k, k > 64 ? 256 : (B <= 64 ? k : 4 * k));
  auto prefix_for = [&](int64_t n0) {  // prefix whose bound is worth the exact k-th best of n0 keys
    if (k > 64) {
      // Lists of 65 .. 128 keys: p parts need p ring stages, and fewer parts are worth less per key (filter_bound_eff) -- the
      // shortest prefix over every part count the prefix itself has room for.
      const int64_t stage = FILTER_STAGE_BYTES / (2 * D);
      int64_t best = INT64_MAX;
      for (int p = 256; p >= k; --p) {
        int64_t need = filter_round_up((int64_t)((double)n0 * filter_bound_eff(k, p)));
        if (need < p * stage) need = filter_round_up(p * stage);
        if (filter_bound_parts(k, need, D, B) >= p && need < best) best = need;
      }
      return best;
    }
    int64_t nA = filter_round_up((int64_t)((double)n0 * eff_div));
    const int parts = filter_bound_parts(k, nA, D, B);
    if (parts < 4 * k && (parts < 128 || (k > 64 && parts < 256))) nA = filter_round_up((int64_t)((double)n0 * filter_bound_eff(k, parts)));
    return nA;
  };
  if (B > FILTER_SLAB_MAX_B || N < 4 * 4096) {
    // (the first sample: with 4 k parts the bound pass is cheap enough for N / 64 -- fewer candidates at the first level,
    // whose sub-tiles otherwise nearly all take the candidate path: 100k x 1M: 38.0 -> 36.5 ms against N / 256;
    // RAGRAPH_FILTER_N0DIV: A/B)
    static const int64_t n0div = [] { const char* e = getenv("RAGRAPH_FILTER_N0DIV"); return e ? (int64_t)atoll(e) : (int64_t)64; }();
    int64_t n0 = N * n_shards / n0div;  // (over all shards)
    if (n0 < 4096) n0 = 4096;
    int64_t nA = bound ? prefix_for(n0) : 0;
    if (n_shards > 1) {  // this shard's share
      n0 /= n_shards;
      nA = filter_round_up(nA / n_shards);
      const int64_t min_keys = filter_round_up((int64_t)k * (FILTER_STAGE_BYTES / (2 * D)));
      if (nA < min_keys) nA = min_keys;
    }
    if (n0 > N) n0 = N;
    if (n0 < k) n0 = k < N ? k : N;
    if (bound) {
      if (nA > N / 4) nA = N / 4 / FILTER_PAD_KEYS * FILTER_PAD_KEYS;
      sc.bound_keys = nA;
    }
    sc.n0 = n0;
    sc.slab0 = 0;  // (measured at 100 k queries: slabs of 16384 cost 3.6 ms -- dense kernel 104 TFLOP/s, topk_rows bound
                   // by its list inserts -- against the tile kernel's 3.2 ms)
    sc.nlev = 0;
    int64_t prev = n0;
    // (RAGRAPH_FILTER_FRACS="a,b": the first ends as fractions N/a, N/b of the bank -- schedule experiments)
    int64_t fracs[2] = {32, 4};
    int nfr = 2;
    if (const char* fe = getenv("RAGRAPH_FILTER_FRACS")) {
      long long a = 0, b = 0;
      nfr = sscanf(fe, "%lld,%lld", &a, &b);
      if (nfr < 1 || a < 2) nfr = 0;
      fracs[0] = a;
      fracs[1] = b;
      if (nfr == 2 && b < 2) nfr = 1;
    }
    if (k > 64) {
      // Lists of 65 .. 128 keys: a level may admit 1.3 k (end / previous end) <= cap / 2 keys, a ratio of 6 at k = 128, and the
      // fixed fractions break that wherever the sample is not N / 64 (the last level of a 130 000-key bank would have a ratio
      // of 8).  Three levels of EQUAL ratio (N / n0)^(1/3) <= 4 instead -- on the banks whose sample is N / 64 these are the
      // ends N / 16 and N / 4 the fractions give.
      nfr = 0;
      const double r3 = pow((double)N / (double)n0, 1.0 / 3.0);
      double e = (double)n0;
      for (int l = 0; l < 2; ++l) {
        e *= r3;
        const int64_t ei = filter_round_up((int64_t)e);
        if (ei * 2 >= N || ei <= prev) break;
        sc.ends[sc.nlev++] = ei;
        prev = ei;
      }
    }
    for (int fi = 0; fi < nfr; ++fi) {
      const int64_t frac = fracs[fi];
      int64_t e = filter_round_up(N / frac);
      if (e < 4 * prev) e = filter_round_up(4 * prev);  // a level is at least 4x what came before
      if (e * 2 >= N) break;                            // too close to the end: the last level takes the rest
      sc.ends[sc.nlev++] = e;
      prev = e;
    }
    sc.ends[sc.nlev++] = N;
    // the k keys behind the bound must lie inside the first level (it has to find at least k candidates)
    if (sc.bound_keys > sc.ends[0]) sc.bound_keys = sc.ends[0] / FILTER_PAD_KEYS * FILTER_PAD_KEYS;
    if (sc.bound_keys / (FILTER_STAGE_BYTES / (2 * D)) < k) sc.bound_keys = 0;  // every part needs a stage of its own
    sc.i8_levels = i8_ok && B >= 1024 ? (scored ? 3 : 2) : 0;  // (banks below 4 x 4096 keys come here with any batch)
    if (k > 32) {
      // Lists of 33 .. 64 keys (the wide entry; plans of k <= 32 never come here): a level admits ~1.3 k (its end / the previous
      // end) keys per query and an int8 level i8_candf = 2 times that.  The cost-model branch below refuses a plan beyond half the
      // list capacity; these fixed fractions get the same test per int8 level, earliest first -- at k = 10 a ratio of 8 is 208
      // int8 candidates, at k = 64 it would be 1331 of 2048 slots on AVERAGE, and overflows (exact scans) the common case.
      while (sc.i8_levels > 0) {
        const int l0 = sc.nlev - sc.i8_levels;
        if (l0 < 0) {
          sc.i8_levels = sc.nlev;
          continue;
        }
        const double before = l0 ? (double)sc.ends[l0 - 1] : (double)sc.n0;
        if (1.3 * k * ((double)sc.ends[l0] / before) * 2.0 <= cap / 2) break;
        --sc.i8_levels;
      }
    }
    filter_align_ends(sc, D);
    return sc;
  }
  double best = 1e30;
  int64_t best_n0 = 4096, best_nA = 0;
  int best_L = FILTER_MAX_LEVELS, best_i8 = 0;
  // RAGRAPH_FILTER_FORCE_N0 / _L: schedule experiments (n0 = the exact sample the first bound is worth, L levels)
  static const int64_t force_n0 = [] { const char* e = getenv("RAGRAPH_FILTER_FORCE_N0"); return e ? (int64_t)atoll(e) : (int64_t)0; }();
  static const int force_L = [] { const char* e = getenv("RAGRAPH_FILTER_FORCE_L"); return e ? atoi(e) : 0; }();
  const int stage_keys = FILTER_STAGE_BYTES / (2 * D);
  const double tiles = (double)((B + 511) / 512);
  for (int64_t n0 = 4096; n0 * 4 <= N; n0 *= 2) {
    if (force_n0 > 0 && n0 != force_n0) continue;
    double first;  // cost of the first bound, us
    int64_t nA = 0;
    if (bound) {
      nA = prefix_for(n0);
      // (lists of 33 .. 64 keys: every part of the prefix is a ring stage of its own, so k parts are 4 - 16 k keys before the
      // bound is worth anything -- at D = 64, 48 parts are worth 4096 keys and span 19 968.  A quarter of a 70 000-key bank
      // holds no such prefix, no sample passes this test, and the call would run the default three levels behind a score slab
      // with nothing for a prior to replace; half the bank -- the limit filter_call_plan itself sets -- does.  k <= 32: unchanged.)
      if (nA * (k > 32 ? 2 : 4) > N) break;
      if (B <= 256)  // direct kernel: the prefix streams at ~5 TB/s (8.7 / 22 / 40 us for 54 k / 216 k / 216 k keys x 1 / 16 / 256 queries)
        first = 6.0 + (double)nA * 2.0 * D / 5.0e6 * (1.0 + (double)B / 320.0);
      else
        first = 35.0 + (double)nA * 2.0 * D / 3.0e6 + tiles * (double)(nA / stage_keys) * 3.1 / 256.0;
    } else {
      if (B * n0 > FILTER_SLAB_MAX_SCORES) break;
      first = 30.0 + (double)B * (double)n0 * (2.0 * D / 1.0e8 + 4.0 / 3.0e6);
    }
    for (int L = 1; L <= FILTER_MAX_LEVELS; ++L) {
      if (force_L > 0 && L != force_L) continue;
      const double r = pow((double)N / (double)n0, 1.0 / L);
      // (lists of 65 .. 128 keys: the prefix must lie inside the first level -- cut down to it, the bound would be worth less than
      // the n0 keys the first level's ratio is planned from; and they plan against 97 % of half a list: the ends are rounded to
      // whole pads and stages behind this test)
      if (k > 64 && bound && L > 1 && (double)nA > (double)n0 * r - 512.0) continue;
      if (1.3 * k * r > (k > 64 ? 0.97 : 1.0) * (cap / 2) && !(force_n0 > 0 && force_L > 0)) continue;
      // a level: launches + the rescoring kernels' latency floor, plus ~0.4 - 0.5 ns per candidate (1 KB row gather each)
      if (B <= 256) {
        // Direct kernel.  On the int8 copy its pass streams half the bytes and does half the matrix work (one query: 78 ->
        // 40 us of kernel; 256: 124 -> ~75) while ~3x the candidates come back: the same model with 3.9 k r candidates per
        // level and that saving decides between the two -- and moves n0 up when int8 wins.
        // (int8 wins at every batch size from 1 to 256 on the 1M x 256 bank -- 0.106 -> 0.074, 0.124 -> 0.091, 0.139 -> 0.109,
        // 0.192 -> 0.153 ms -- so where it is eligible the model only chooses ITS schedule; the two constants are not
        // comparable across the dtypes)
        // (lists of 65 .. 128 keys: three times 1.3 k r passes half a list from a ratio of 2 at k = 128 -- the bf16 schedule stays
        // in the race, or large banks would be left without any plan that fits)
        for (int q8 = i8_direct && k <= 64 ? 1 : 0; q8 <= (i8_direct ? 1 : 0); ++q8) {
          const double cands = 1.3 * k * r * (q8 ? 3.0 : 1.0);
          // (a handful of queries keep S sub-lists of `cap` slots each: filter_cap)
          if (cands > cap * (q8 ? rescore_slices(B, k) : 1) / 2 && !(force_n0 > 0 && force_L > 0)) continue;
          // (the sliced / wide rescoring of a small call is a latency chain: measured 1.2 - 3.7 ns per candidate on the int8
          // schedules -- forced n0 at 1 / 16 / 64 queries, profiles/r3_i8_ab.txt -- where round 2 fitted 0.5 to its bf16 ones)
          const double cost = first + L * (25.0 + (double)B * cands * (q8 ? 2.0e-3 : 0.5e-3)) + (L - 1) * (q8 ? 30.0 : 15.0)  /* (a second pass start-up; 256 queries, int8: one level 0.156, two 0.162 ms) */
                              - (q8 ? 32.0 + 0.08 * (double)B : 0.0);
          if (cost < best) {
            best = cost;
            best_n0 = n0;
            best_nA = nA;
            best_L = L;
            best_i8 = q8 ? L : 0;
          }
        }
        continue;
      }
      // Ring kernel: + the matrix work of each level -- 2 B keys D at ~1.25 PFLOP/s on the bf16 copy, ~2.4 Pop/s on the
      // int8 copy, whose ~5x wider bound passes ~3x the candidates -- for 0, 1 or 2 trailing int8
      // levels.  (Without int8 the matrix term is the same for every (n0, L): the choice among those is round 2's.)
      // Measured against forced schedules at 512 / 1024 / 2048 queries x 1M keys (profiles/r3_i8_ab.txt).
      // (a candidate costs ~0.4 ns while a level's rescoring is a latency chain -- up to ~1000 queries -- and ~0.18 ns once it
      // is bound by the row gathers: 100 000 queries x ~130 candidates x 1 KiB in 1.8 ms)
      const double per_cand = 0.18e-3 + 0.22e-3 * (B <= 1024 ? 1.0 : 1024.0 / (double)B);
      // (int8 candidates per bf16 candidate.  3.0 until the copy got its two scales and the calls their speculative bounds; 2.0
      // fits what tools/i8_rule_grid.py measures now -- 105 shapes of 300 .. 16 384 queries x 70 k .. 1 M keys x D = 64 / 128 /
      // 256, KeyIndex in its steady state, geomean 0.971 of the old rule's time; the banks of 150 k - 500 k keys that moved to
      // int8 0.77 - 0.9 (1100 x 300 k x 256: 0.188 -> 0.144 ms); 1.5 loses up to 1.6 x on 70 k-key banks.  profiles/r5_i8_rule_grid.txt)
      static const double i8_candf = [] { const char* e = getenv("RAGRAPH_FILTER_I8_CANDF"); return e ? atof(e) : 2.0; }();  // A/B
      // (mid_i8 -- D = 256 banks of 32 768 .. 65 535 keys: the constants below were fitted on million-key banks and overprice
      // these shapes' candidates; what measured faster there is the bf16 plan with every level moved to int8: see below)
      for (int i8 = 0; i8 <= (i8_ok && !mid_i8 ? (L < 2 || scored ? L : 2) : 0); ++i8) {
        double cost = first, e_prev = 0.0, e = (double)n0;
        bool fits = true;
        for (int l = 0; l < L; ++l) {
          e = l + 1 == L ? (double)N : e * r;
          const bool q8 = l >= L - i8;
          const double cands = 1.3 * k * r * (q8 ? i8_candf : 1.0);
          if (cands > (k > 64 ? 0.97 : 1.0) * (cap / 2) && !(force_n0 > 0 && force_L > 0)) fits = false;
          cost += 60.0 + (e - e_prev) * (double)B * 2.0 * D / (q8 ? 2.4e9 : 1.25e9) +
                  (double)B * cands * per_cand * (q8 && scored ? scored_cand : 1.0);
          e_prev = e;
        }
        if (fits && cost < best) {
          best = cost;
          best_n0 = n0;
          best_nA = nA;
          best_L = L;
          best_i8 = i8;
        }
      }
    }
  }
  sc.bound_keys = bound ? (best_nA ? best_nA : prefix_for(4096)) : 0;
  if (bound && B > 128 && B <= 256 && n_shards == 1) {
    // the direct kernel deals the prefix's 16-KiB units over all waves of the chip in contiguous runs: 2.4 units per wave take
    // as long as 3 -- a prefix of whole rounds (8 waves x CUs units) costs what it reads: 256 queries x 1M 0.1406 -> 0.1381 ms,
    // 192: 0.1198 -> 0.1180 (up to 128 queries, whose pass is cheaper per key, the shorter prefix loses more than it saves:
    // 64 queries 0.110 -> 0.116).
    const int64_t round_keys = (int64_t)8 * cus * (16384 / (2 * D));
    int64_t r = (sc.bound_keys + round_keys / 2) / round_keys;
    if (r < 1) r = 1;
    if (r * round_keys * 4 <= N && r * round_keys >= (int64_t)k * 4 * (FILTER_STAGE_BYTES / (2 * D))) sc.bound_keys = r * round_keys;
  }
  sc.n0 = best_n0;
  sc.i8_levels = mid_i8 ? best_L : best_i8;
  // (lists of 65 .. 128 keys: the row top-k behind the slab stops at 64 -- an exact level 0 is ragraph_topk_cosine_bank_f32, whose
  // own slabs end in the ordered large-k selection)
  sc.slab0 = k > 64 ? 0 : 1;
  sc.nlev = 0;
  const double r = pow((double)N / (double)best_n0, 1.0 / best_L);
  // (lists of 65 .. 128 keys: the mid-sized banks' all-int8 plan only where its levels keep to half a list)
  if (k > 64 && mid_i8 && 1.3 * k * r * 2.0 > cap / 2) sc.i8_levels = best_i8;
  double e = (double)best_n0;
  for (int l = 0; l + 1 < best_L; ++l) {
    e *= r;
    const int64_t ei = filter_round_up((int64_t)e);
    if (ei * 2 >= N) break;
    sc.ends[sc.nlev++] = ei;
  }
  sc.ends[sc.nlev++] = N;
  if (sc.bound_keys > sc.ends[0]) sc.bound_keys = sc.ends[0] / FILTER_PAD_KEYS * FILTER_PAD_KEYS;
  if (sc.bound_keys / stage_keys < k) sc.bound_keys = 0;  // every part needs a stage of its own: else the exact slab
  if (sc.bound_keys == 0 && B * sc.n0 > FILTER_SLAB_MAX_SCORES) sc.slab0 = 0;
  filter_align_ends(sc, D);
  return sc;
}

// Which levels run on the int8 copy: the LAST level of a large batch (D = 128 / 256).  Its threshold is the highest of the
// call, so the ~4x wider eps costs ~100 extra candidates per query (1 KiB row gathers: ~2.5 ms at the bench shape) where
// the matrix work of three quarters of the bank halves (25.6 -> ~13 ms).  Earlier levels and smaller batches stay on
// bf16: a level of a few thousand queries is not matrix-bound enough to pay for the extra rescoring.
// RAGRAPH_FILTER_I8 = n forces the last n levels (0: none) -- A/B runs and the tests of the int8 path on small shapes.
// i8_cap: the calling thread's cap (ragraph_topk_cosine_filtered_max_i8_levels: -1 = the rule below, 0 = none).
static int filter_i8_levels(const FilterSchedule& sc, int64_t B, int i8_cap, const FilterEnv& env) {
  if (B <= 256) {  // the direct kernel's int8 form: every level or none, as the schedule planned
    if (i8_cap == 0 || sc.i8_levels == 0) return 0;
    return sc.nlev;
  }
  if (env.i8 >= 0) return env.i8 < sc.nlev ? env.i8 : sc.nlev;
  if (i8_cap == 0) return 0;
  // The schedule plans them (filter_schedule: sc.i8_levels -- the level STRUCTURE never depends on the per-thread cap, so
  // the shards of a bank keep the same phases whatever each thinks of its rows).  Measured on the 1M x 256 bank (ms per
  // call, 0 / 1 / 2 int8 levels on round 2's schedules; profiles/r3_i8_ab.txt): 1024 queries 0.538 / 0.519 / 0.505; 2048:
  // 0.98 / 0.80 / 0.83; 4096: 1.75 / 1.34 / 1.28; 16384: 6.09 / 4.55 / 4.19; 100 000 (the bench step): 38.3 / 28.3 / 26.9
  // (three: 27.7); with the schedule chosen for int8 (two levels, the second on int8): 512: 0.314 -> 0.276, 1024: 0.509 -> 0.426.
  int n = sc.i8_levels < sc.nlev ? sc.i8_levels : sc.nlev;
  if (i8_cap > 0 && n > i8_cap) n = i8_cap;
  return n;
}

enum FilterLevel0 {
  FILTER_L0_NONE,   // theta = the prior (the prepare launch writes it)
  FILTER_L0_BOUND,  // the bound pass over keys [0, bound_keys) of the bf16 copy, `parts` part maxima per query
  FILTER_L0_SLAB,   // exact top-k of the first n0 keys: dense kernel + topk_rows
  FILTER_L0_TILE    // ... the fp32 tile kernel
};
struct FilterLevel {
  int64_t key0, key1;
  bool int8, scored;  // on the int8 copy; with {key, I} lists
};
// What a call does, in the order it does it.  run_filtered executes this and decides nothing itself; the size query and the
// host queries read the same object.
struct FilterCall {
  int cap;                 // slots of a query's candidate region (filter_cap)
  bool scored_slots;       // ... of 8 bytes: the call may keep scored lists (sharded calls of the same shape do not use them)
  bool exact_participant;  // a shard too short for the plan's phases: its fp32 top-k, offered at every exchange (nlev,
                           // spec and first_phase are all that is planned for it)
  bool spec;               // speculative first bound: no bound pass, no phase 0, a verify launch behind the last level
  FilterLevel0 level0;
  size_t level0_bytes;     // level 0's scratch at the head of the workspace: the tile kernel's, or the score slab
  int64_t n0, bound_keys;  // keys of an exact level 0 / of the bound pass (0: none)
  int parts;               // part maxima per query of the bound pass (else k)
  int nlev, i8_levels;
  FilterLevel level[FILTER_MAX_LEVELS];
  bool bf16_image;         // the prepare launch writes the queries' bf16 operand image: only launches on the bf16 copy read it -- a
                           // call whose levels all run on the int8 copy and that has no bound pass, e.g. every call under a
                           // prior, saves writing 2 D bytes per query
  int first_phase;         // sharded calls: the exchange is called at phases first_phase .. nlev - 1
  bool tight;              // the levels start from theta = the tight bound; behind them the soft verdict and the repair launches
                           // (run_filtered step 6b), whose rescoring is the call's FINAL one -- no level's is (level_final)
  bool repair_scored;      // ... the 256-query repair keeps scored lists
  int level_final;         // the level whose rescoring is the call's final one (adds idx_base, lists overflows), or -1
};

// What the 256-query repair behind a tight bound keeps besides its candidate lists: the gathered rows, their normalised form and
// operand image, its own small per-query arrays and result rows (run_filtered carves them: FilterRepairWs).
static size_t filter_repair_bytes(int D, int k, size_t slot_bytes) {
  const size_t q = FILTER_REPAIR_Q;
  return q * FILTER_LIST_CAP * slot_bytes + 2 * q * D * sizeof(float) + q * D * sizeof(uint16_t) + q * FILTER_COUNT_STRIDE * sizeof(int) +
         align_up(q * k * sizeof(float), 256) + align_up(q * k * sizeof(int64_t), 256) + 16 * 1024 /* ten arrays of <= 1 KiB, aligned */;
}

// Bytes of a call's candidate region.  Lists of 33 .. 64 keys (the wide entry) are plain by rule (filter_scored_lists: 4-byte
// slots), which would leave the calls of 257 to about 350 queries without the idle room the repair behind a tight bound lives
// in: their region is at least the repair's size, so every ring-kernel call of the wide entry honours a tight bound.  (k <= 32:
// the lists and nothing else, as the workspace sizes pinned by the tests have it.)
static size_t filter_cand_bytes(int64_t B, int cap, size_t slot_bytes, int D, int k) {
  size_t bytes = (size_t)B * cap * slot_bytes;
  if (k > 32 && B > FILTER_REPAIR_Q) {
    const size_t need = filter_repair_bytes(D, k, slot_bytes);
    if (bytes < need) bytes = need;
  }
  return bytes;
}

static void filter_drop_first_level(FilterSchedule& sc) {
  for (int l = 0; l + 1 < sc.nlev; ++l) sc.ends[l] = sc.ends[l + 1];
  --sc.nlev;
  if (sc.i8_levels > sc.nlev) sc.i8_levels = sc.nlev;
}

// The plan of one call from the schedule of (B, plan_N, D, k, exchange ? n_shards : 1): every adjustment of that schedule
// to the prior, to this shard's own length and to the sharing of the first sample happens here, once.
static FilterCall filter_call_plan(const FilterShape& in, FilterSchedule sc) {
  const int64_t B = in.B, N = in.N, plan_N = in.plan_N;
  const int D = in.D, k = in.k, ns = in.exchange ? in.n_shards : 1;
  const int stage_keys = FILTER_STAGE_BYTES / (2 * D);
  FilterCall c{};
  c.cap = filter_cap(B, k);
  c.scored_slots = filter_scored_lists(B, D, k, in.env);
  const bool prior_ok = in.prior == in.prior && in.prior > -2.f && in.prior < 2.f;
  // Under the prior the first level goes.  A first level exists to give the second a tighter bound than the bound pass
  // could; the prior already is one.  Measured with it (1M x 256, ms per call, two levels / one): 2048 queries 0.544 / 0.512,
  // 4096: 0.920 / 0.898 -- but 16 384: 3.18 / 3.85, and the three levels of 100 000 queries stay (20.5 ms per step against 22.8
  // with two): up to 4096 queries one level.
  // Three levels under the prior, many shards: the first level (1 / 32 of the shard) exists to sharpen the bound pass's
  // bound, and under the group's prior it passes about ONE candidate per query and shard (measured, 8 shards of the 1M bank) --
  // a filter launch on the bf16 copy, a rescoring launch over every query and an exchange for nothing.  From
  // RAGRAPH_FILTER_SPEC_SHARDS_TWO_LEVELS shards (default 2: every sharded bank; 0 = never) the call runs levels [0, N / 4) and
  // [N / 4, N): emulated rank of 2 / 4 / 8, ms per step: 11.14 -> 10.83, 6.29 -> 5.92, 3.73 -> 3.46 (profiles/r6_multi_one_gpu.txt).
  const int spec_two = in.env.spec_two_shards;
  auto drop_first_level_under_prior = [&] {
    if ((sc.nlev == 2 && B <= 4096) || (in.exchange && sc.nlev == 3 && spec_two > 0 && in.n_shards >= spec_two))
      filter_drop_first_level(sc);
  };
  if (in.exchange) {
    // Sharded banks: whether the call speculates must be the SAME decision on every rank -- it removes the bound pass AND its
    // exchange (phase 0) --, so it is taken from what every rank shares: the prior (the caller derives it from pooled
    // statistics and sets it on every rank alike) and the PLAN's bound pass (plan_N), before any adjustment to this shard's
    // own length.  The proof is the caller's too: a query is exact iff the k-th best of the MERGED lists reaches the prior
    // (ragraph_amd/sharded.py verifies at the rows' owner and re-runs without the prior).
    c.spec = prior_ok && sc.bound_keys > 0;
    if (c.spec) drop_first_level_under_prior();
    // A shard SHORTER than the largest one (shards of a bank whose exact duplicates were collapsed per shard hold different
    // numbers of unique rows): the same phases -- the exchanges must line up across the ranks -- over proportionally fewer
    // keys; a shard too short for that structure takes part as an EXACT participant: its fp32 top-k once, offered at every
    // exchange (exact scores of k distinct keys are valid lower bounds at every phase).
    if (plan_N - N > 1024) {
      int64_t prev = 0;
      for (int l = 0; l + 1 < sc.nlev; ++l) {
        int64_t e = (int64_t)((double)sc.ends[l] * (double)N / (double)plan_N) / 512 * 512;   // (512: whole int8 stages at any width)
        if (e < prev + 512 || e + 512 > N) c.exact_participant = true;
        sc.ends[l] = e;
        prev = e;
      }
      sc.bound_keys = (int64_t)((double)sc.bound_keys * (double)N / (double)plan_N) / FILTER_PAD_KEYS * FILTER_PAD_KEYS;
      if (sc.nlev > 1 && sc.bound_keys > sc.ends[0]) sc.bound_keys = sc.ends[0];
      if (sc.bound_keys / stage_keys < (int64_t)filter_bound_parts(k, sc.bound_keys, D, B, in.n_shards)) sc.bound_keys = 0;
      if (sc.n0 > N) sc.n0 = N;
      if (N < 16384 || N * 8 < plan_N) c.exact_participant = true;
    }
  }
  c.first_phase = c.spec ? 1 : 0;   // phase 0 pools the first bounds: not under a speculative one
  c.nlev = sc.nlev;
  if (c.exact_participant) return c;
  sc.ends[sc.nlev - 1] = N;
  // The bound pass gives way to an exact level 0 where its prefix is more than half of this shard -- or where a size query
  // asks what that would need: the workspace is sized for whichever of the two needs more.
  if (sc.bound_keys > N / 2 || in.exact_level0) {
    sc.bound_keys = 0;
    if (sc.n0 > N) sc.n0 = N;
  }
  if (in.exchange && in.n_shards > 1 && sc.bound_keys > 0 && B <= FILTER_SLAB_MAX_B && plan_N >= 4 * 4096) {  // (the cost-model branch)
    // G shards pool their samples through the exchange (the k-th largest of the union of every shard's best group
    // maxima): each scans 1/G of the prefix one bank would -- at least one stage per part
    const int64_t min_keys = filter_round_up((int64_t)k * stage_keys);
    const int64_t bk = filter_round_up(sc.bound_keys / in.n_shards);
    sc.bound_keys = bk < min_keys ? (min_keys < sc.bound_keys ? min_keys : sc.bound_keys) : bk;
  }
  if (!in.exchange) {
    // One bank whose schedule has a bound pass to save: theta = prior for every query, every level filters with max(prior,
    // the running k-th best), and the verify launch behind the last level sends the queries the prior was too high for to
    // the exact scan.
    // (Lists of 65 .. 128 keys speculate whatever their first bound is: k parts of one ring stage each are 8 - 33 k keys, which
    // the smaller banks do not have inside their first half, and the exact level 0 such a plan falls back to -- fp32 score
    // slabs over n0 keys -- is the dearer thing for a prior to replace.)
    c.spec = prior_ok && (sc.bound_keys > 0 || k > 64) && N == plan_N;
    if (c.spec) drop_first_level_under_prior();
  }
  // A TIGHT bound t (ragraph_topk_cosine_filtered_set_tight_prior) on top of the prior p: one bank, the ring kernel's batch sizes,
  // p < t.  Every query starts from theta = t, and no intermediate level can sharpen beyond a bound that is about the lowest
  // k-th best the bank has answered (the k-th best of a quarter of the bench's bank is 0.246 against t = 0.249), so the call runs
  // ONE level over [0, N) -- on int8, with scored lists, where the plan's last level would -- and no theta launch.  A query
  // whose k-th best found is below t is a SOFT miss: repaired on the device from max(p, what it found), see run_filtered.
  // Workspace rule: the repair's buffers live in regions that are idle by then -- the candidate lists the level's rescoring
  // has consumed and gmax behind them (no bound pass under a prior) -- and the size queries do not change; a shape whose lists
  // + gmax are smaller than filter_repair_bytes (fewer than about 300 queries at D = 256) ignores the tight bound.
  // RAGRAPH_FILTER_TIGHT_LEVELS=2 keeps the plan's last two levels under the tight bound (A/B): the bench step, interleaved on one
  // box, 19.05 / 19.01 ms with two levels against 18.66 / 18.70 with one; up to 4096 queries the call under the prior runs one
  // level anyway.  The step against the three levels under the prior alone: 19.68 - 19.83 -> 18.30 - 18.31 ms (profiles/tight_prior.txt).
  {
    const size_t slot = c.scored_slots ? sizeof(int2) : sizeof(int);
    const size_t idle = align_up(filter_cand_bytes(B, c.cap, slot, D, k), 256) + align_up((size_t)B * filter_bound_parts(k, INT64_MAX, 256) * sizeof(int), 256);
    c.tight = c.spec && !in.exchange && B > 256 && in.tight == in.tight && in.tight > in.prior && in.tight < 2.f &&
              idle >= filter_repair_bytes(D, k, slot);
  }
  if (c.tight)
    while (sc.nlev > (in.env.tight_levels == 2 ? 2 : 1)) filter_drop_first_level(sc);
  const bool bound = sc.bound_keys > 0 && !c.spec;
  c.level0 = c.spec ? FILTER_L0_NONE : (bound ? FILTER_L0_BOUND : (sc.slab0 ? FILTER_L0_SLAB : FILTER_L0_TILE));
  c.level0_bytes = sc.bound_keys > 0 ? 0
                   : sc.slab0        ? align_up((size_t)(B < FILTER_SLAB_MAX_B ? B : FILTER_SLAB_MAX_B) * (size_t)sc.n0 * sizeof(float), 256)
                                     : ragraph_topk_cosine_workspace_bytes(B, sc.n0, D, k);
  c.n0 = sc.n0;
  c.bound_keys = sc.bound_keys;
  c.parts = bound ? filter_bound_parts(k, sc.bound_keys, D, B, ns) : k;
  c.nlev = sc.nlev;
  c.i8_levels = filter_i8_levels(sc, B, in.i8_cap, in.env);
  c.bf16_image = B <= FILTER_QB_MAX_B && (B <= 256 || bound || c.nlev > c.i8_levels);
  for (int l = 0; l < c.nlev; ++l) {
    FilterLevel& lv = c.level[l];
    lv.key0 = l ? sc.ends[l - 1] : 0;   // the first level re-reads [0, n0): its keys pass the bound and need no merge
    lv.key1 = sc.ends[l];
    lv.int8 = l >= c.nlev - c.i8_levels;
    // (sharded banks keep the plain lists: a level's threshold already is the k-th best over ALL shards -- sharper than
    // anything round 1 can find among this shard's keys, so nothing is pruned and only the second round's latency and the
    // 16-row tiles' occupancy are lost: emulated rank of 2 / 4 / 8 GPUs 13.49 -> 13.26 / 7.61 -> 8.00 / 4.76 -> 5.24 ms per
    // step, profiles/r3_emul.txt.  RAGRAPH_FILTER_SCORED_SHARDS = largest shard count that takes them: A/B.)
    lv.scored = lv.int8 && (!in.exchange || in.n_shards <= in.env.scored_shards) && c.scored_slots;
  }
  c.level_final = c.tight ? -1 : c.nlev - 1;
  c.repair_scored = c.tight && c.level[c.nlev - 1].scored;
  return c;
}
