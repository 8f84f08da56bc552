// Exhaustive host-side check of the canonical top-k order's keys (ragraph_amd/csrc/topk_order.h, its plain-C++ part).
// Every float that is no NaN, in ascending numeric order (-inf .. -0, +0 .. +inf), goes through both key maps:
//   * order_key strictly increases, except that -0 and +0 share one key; order_unkey returns the float, +0 for both zeros;
//   * f2ord strictly increases, -0 below +0; ord2f returns the exact bits;
//   * small_f2u is nonzero, has the same order, and small_u2f returns the exact bits.
// Then, over the cross product of a pool of edge (score, id) pairs and the empty entry: the unsigned order of pair_key is
// cand_better, the empty entry is the minimum (key 0), pair_key_real agrees on real pairs, its words are order_key and pair_lo,
// and pair_score / pair_id decode them;
// the three-word cand_better is the two-word one with the third word as the last tie-break; a NaN is never preferred, and the
// maps keep a NaN's bits and its place outside the infinities.  Prints the f2ord words of the pool's scores
// (tests/test_cpu_topk_order.py decodes them with ragraph_amd.filter_stats.ord2f).  Exit status 0 = every check held.
//   g++ -O2 -std=c++17 -I ragraph_amd/csrc tools/check_topk_order.cpp -o /tmp/check_topk_order && /tmp/check_topk_order
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "topk_order.h"

using namespace ragraph;

static float f_of(uint32_t b) { return __builtin_bit_cast(float, b); }
static uint32_t b_of(float f) { return __builtin_bit_cast(uint32_t, f); }

static int fails = 0;
#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond) && ++fails <= 20) {   \
      printf("FAILED %s: ", #cond);   \
      printf(__VA_ARGS__);            \
      printf("\n");                   \
    }                                 \
  } while (0)

int main() {
  // ---- the walk: bits 0xFF800000 (-inf) down to 0x80000000 (-0), then 0x00000000 (+0) up to 0x7F800000 (+inf)
  uint64_t walked = 0;
  bool have_prev = false;
  uint32_t pb = 0, pkey = 0, psm = 0;
  int pord = 0;
  auto visit = [&](uint32_t b) {
    const float f = f_of(b);
    const uint32_t key = order_key(f), sm = small_f2u(f);
    const int ord = f2ord(f);
    const bool zeros = have_prev && pb == 0x80000000u && b == 0u;
    if (have_prev) {
      CHECK(zeros ? key == pkey : key > pkey, "order_key at %08x after %08x: %08x, %08x", b, pb, key, pkey);
      CHECK(ord > pord, "f2ord at %08x after %08x: %d, %d", b, pb, ord, pord);
      CHECK(sm > psm, "small_f2u at %08x after %08x: %08x, %08x", b, pb, sm, psm);
    }
    CHECK(b_of(order_unkey(key)) == (b == 0x80000000u ? 0u : b), "order_unkey(order_key(%08x)) = %08x", b, b_of(order_unkey(key)));
    CHECK(b_of(ord2f(ord)) == b, "ord2f(f2ord(%08x)) = %08x", b, b_of(ord2f(ord)));
    CHECK(sm != 0u, "small_f2u(%08x) = 0", b);
    CHECK(b_of(small_u2f(sm)) == b, "small_u2f(small_f2u(%08x)) = %08x", b, b_of(small_u2f(sm)));
    have_prev = true;
    pb = b, pkey = key, psm = sm, pord = ord;
    ++walked;
  };
  for (uint32_t b = 0xFF800000u; b >= 0x80000000u; --b) visit(b);
  for (uint32_t b = 0u; b <= 0x7F800000u; ++b) visit(b);
  CHECK(walked == 2ull * 0x7F800001ull, "walked %llu floats", (unsigned long long)walked);
  printf("floats walked: %llu\n", (unsigned long long)walked);

  // ---- NaN: never preferred; the maps keep the bits, the sign bit decides the side of the infinities
  const float inf = std::numeric_limits<float>::infinity();
  for (uint32_t nb : {0x7FC00000u, 0x7F800001u, 0x7FFFFFFFu, 0xFFC00000u, 0xFF800001u, 0xFFFFFFFFu}) {
    const float n = f_of(nb);
    for (float other : {-inf, -1.f, 0.f, 1.f, inf, n}) {
      CHECK(!cand_better(n, 0, other, 1) && !cand_better(other, 1, n, 0), "cand_better prefers around NaN %08x", nb);
      CHECK(!cand_better(n, 0, 0, other, 1, 1) && !cand_better(other, 1, 1, n, 0, 0), "three-word cand_better around NaN %08x", nb);
    }
    CHECK(b_of(order_unkey(order_key(n))) == nb && b_of(ord2f(f2ord(n))) == nb && b_of(small_u2f(small_f2u(n))) == nb, "NaN %08x bits", nb);
    if (nb & 0x80000000u) {
      CHECK(order_key(n) < order_key(-inf) && f2ord(n) < f2ord(-inf) && small_f2u(n) < small_f2u(-inf), "NaN %08x not below -inf", nb);
    } else {
      CHECK(order_key(n) > order_key(inf) && f2ord(n) > f2ord(inf) && small_f2u(n) > small_f2u(inf), "NaN %08x not above +inf", nb);
    }
  }
  CHECK(small_f2u(f_of(0xFFFFFFFFu)) == 0u, "small_f2u of the all-ones NaN");

  // ---- the pair key against cand_better on the edge pool
  const float dmin = std::numeric_limits<float>::denorm_min(), adj = 0.1f;
  const float scores[] = {-0.f, 0.f, -dmin, dmin, -1.f, 1.f, -inf, inf, adj, std::nextafterf(adj, 1.f)};
  const int ids[] = {0, 1, INT_MAX - 1};
  struct Pair {
    float s;
    int id;
  };
  Pair pool[sizeof(scores) / sizeof(scores[0]) * 3 + 1];
  int np = 0;
  for (float s : scores)
    for (int id : ids) pool[np++] = {s, id};
  const Pair empty = {-inf, RG_IDX_NONE};
  pool[np++] = empty;
  CHECK(pair_key(empty.s, empty.id) == 0ull, "the empty entry's key");
  for (int a = 0; a < np; ++a) {
    const Pair x = pool[a];
    const unsigned long long kx = pair_key(x.s, x.id);
    if (x.id != RG_IDX_NONE) {
      CHECK(kx > 0ull, "a real pair's key is 0: %08x %d", b_of(x.s), x.id);
      CHECK(kx == pair_key_real(x.s, x.id), "pair_key_real %08x %d", b_of(x.s), x.id);
      CHECK(pair_id((unsigned)kx) == x.id && (unsigned)kx == pair_lo(x.id) && (unsigned)(kx >> 32) == order_key(x.s) && b_of(pair_score(kx)) == (b_of(x.s) == 0x80000000u ? 0u : b_of(x.s)), "decode %08x %d", b_of(x.s), x.id);
    }
    for (int b = 0; b < np; ++b) {
      const Pair y = pool[b];
      const unsigned long long ky = pair_key(y.s, y.id);
      CHECK((kx > ky) == cand_better(x.s, x.id, y.s, y.id), "pair (%08x, %d) against (%08x, %d)", b_of(x.s), x.id, b_of(y.s), y.id);
      for (int lx = 0; lx < 2; ++lx)
        for (int ly = 0; ly < 2; ++ly) {
          const bool same = x.s == y.s && x.id == y.id;
          CHECK(cand_better(x.s, x.id, lx, y.s, y.id, ly) == (same ? lx < ly : cand_better(x.s, x.id, y.s, y.id)),
                "three words (%08x, %d, %d) against (%08x, %d, %d)", b_of(x.s), x.id, lx, b_of(y.s), y.id, ly);
        }
    }
  }
  printf("pairs checked: %d x %d\n", np, np);
  for (float s : scores) printf("f2ord %08x %d\n", b_of(s), f2ord(s));
  printf(fails ? "FAILED: %d checks\n" : "all checks held\n", fails);
  return fails ? 1 : 0;
}
