// Exhaustive host-side check of the ring kernel's plan (ragraph_amd/csrc/segment_plan.h: RingWalker, ring_plan_choose): for
// qtiles 64 .. 200 x NS x CUS x lb_min, the plan ring_plan_choose takes covers every (query tile, stage) exactly once, has no
// empty segment, every workgroup's walk ends, and its most loaded workgroup never has more stages than the plan of XCD
// groups alone (RING_XCD).  The same checks on RING_SPLIT itself wherever it exists, taken or not.
//   g++ -O2 -std=c++17 -I ragraph_amd/csrc tools/check_ring_plan.cpp -o /tmp/check_ring_plan && /tmp/check_ring_plan
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "segment_plan.h"

using namespace ragraph;

// Walks every workgroup of the plan; returns the most loaded one's stages, or -1 (and says why).
static int64_t walk(int64_t qtiles, int64_t NS, int CUS, int lb_min, const RingPlan& pl) {
  std::vector<std::vector<std::pair<int64_t, int64_t>>> tiles(qtiles);
  int64_t worst = 0;
  for (int b = 0; b < CUS; ++b) {
    RingWalker rw(qtiles, NS, pl.mode == RING_ONE ? CUS : CUS / 8, lb_min, pl.mode, pl.depth[0], pl.depth[1], b);
    Segment s;
    int64_t load = 0;
    int nseg = 0;
    while (rw.next(s)) {
      const int64_t t = rw.qtile(s);
      if (t < 0 || t >= qtiles || s.st0 < 0 || s.st1 > NS || s.st0 >= s.st1) {
        printf("bad segment qtiles=%ld NS=%ld CUS=%d lb_min=%d mode=%d workgroup %d: tile %ld [%ld,%ld)\n", (long)qtiles, (long)NS, CUS,
               lb_min, pl.mode, b, (long)t, (long)s.st0, (long)s.st1);
        return -1;
      }
      tiles[t].push_back({s.st0, s.st1});
      load += s.st1 - s.st0;
      if (++nseg > 100000) {
        printf("runaway walk qtiles=%ld NS=%ld CUS=%d lb_min=%d mode=%d workgroup %d\n", (long)qtiles, (long)NS, CUS, lb_min, pl.mode, b);
        return -1;
      }
    }
    worst = std::max(worst, load);
  }
  for (int64_t t = 0; t < qtiles; ++t) {
    auto& v = tiles[t];
    std::sort(v.begin(), v.end());
    int64_t pos = 0;
    for (auto& sg : v) {
      if (sg.first != pos) {
        printf("gap/overlap qtiles=%ld NS=%ld CUS=%d lb_min=%d mode=%d tile %ld at %ld (segment starts %ld)\n", (long)qtiles, (long)NS, CUS,
               lb_min, pl.mode, (long)t, (long)pos, (long)sg.first);
        return -1;
      }
      pos = sg.second;
    }
    if (pos != NS) {
      printf("tile %ld covered to %ld of %ld (qtiles=%ld CUS=%d lb_min=%d mode=%d)\n", (long)t, (long)pos, (long)NS, (long)qtiles, CUS, lb_min, pl.mode);
      return -1;
    }
  }
  return worst;
}

// With arguments "qtiles NS CUS" (any number of triples): prints the plan launch_ring takes for each and checks it.
static int lb_min_of(int64_t qtiles, int64_t NS, int CUS) {  // (launch_ring's rule)
  const int64_t per_wg = qtiles * NS / CUS;
  return per_wg >= 16 ? 8 : (per_wg >= 8 ? 4 : (per_wg >= 3 ? 2 : 1));
}

int main(int argc, char** argv) {
  if (argc > 1) {
    for (int a = 1; a + 2 < argc; a += 3) {
      const int64_t qtiles = atoll(argv[a]), NS = atoll(argv[a + 1]);
      const int CUS = atoi(argv[a + 2]), lb_min = lb_min_of(qtiles, NS, CUS);
      const RingPlan pl = ring_plan_choose(qtiles, NS, CUS, lb_min);
      const int64_t got = walk(qtiles, NS, CUS, lb_min, pl);
      if (got < 0) return 1;
      int idle = 0;  // workgroups the leftover group gives nothing
      if (pl.mode == RING_SPLIT)
        for (int b = 0; b < CUS; ++b) {
          SegmentWalker w(qtiles % 8, NS, CUS, lb_min, 0, pl.depth[1], b);
          Segment s;
          idle += !w.next(s);
        }
      printf("plan %ld x %ld x %d: mode %d lb_min %d load %ld idle %d\n", (long)qtiles, (long)NS, CUS, pl.mode, lb_min, (long)got, idle);
    }
    return 0;
  }
  long checked = 0, split_taken = 0, split_possible = 0;
  for (int64_t qtiles = 64; qtiles <= 200; ++qtiles)
    for (int64_t NS : {1, 3, 8, 63, 489, 7813})
      for (int CUS : {64, 128, 256})
        for (int lb_min : {1, 8}) {
          const RingPlan pl = ring_plan_choose(qtiles, NS, CUS, lb_min);
          const int64_t got = walk(qtiles, NS, CUS, lb_min, pl);
          if (got < 0) return 1;
          if (pl.mode == RING_SPLIT && got != pl.load) {
            printf("planner's load %ld != walked %ld (qtiles=%ld NS=%ld CUS=%d lb_min=%d)\n", (long)pl.load, (long)got, (long)qtiles, (long)NS, CUS, lb_min);
            return 1;
          }
          // the parent plan: XCD groups alone, with the depths the launch gave them before the split existed
          RingPlan par{RING_XCD, {0, 0}, 0};
          const bool shallow = qtiles * NS / CUS < 16;
          const int64_t nq0 = (qtiles + 7) / 8;
          if (!shallow) {
            par.depth[0] = SegmentWalker::choose_depth(nq0, NS, CUS / 8, lb_min, 0).depth;
            if (qtiles % 8) par.depth[1] = SegmentWalker::choose_depth(nq0 - 1, NS, CUS / 8, lb_min, 0).depth;
          }
          const int64_t parent = walk(qtiles, NS, CUS, lb_min, par);
          if (parent < 0) return 1;
          if (got > parent) {
            printf("chosen plan (mode %d) loads %ld > parent %ld (qtiles=%ld NS=%ld CUS=%d lb_min=%d)\n", pl.mode, (long)got, (long)parent,
                   (long)qtiles, (long)NS, CUS, lb_min);
            return 1;
          }
          if (pl.mode == RING_XCD && (pl.depth[0] != par.depth[0] || pl.depth[1] != par.depth[1])) {
            printf("parent plan kept with other depths (qtiles=%ld NS=%ld CUS=%d lb_min=%d)\n", (long)qtiles, (long)NS, CUS, lb_min);
            return 1;
          }
          if (qtiles % 8) {  // the split itself, taken or not
            ++split_possible;
            split_taken += pl.mode == RING_SPLIT;
            RingPlan sp{RING_SPLIT, {par.depth[1], shallow ? 0 : SegmentWalker::choose_depth(qtiles % 8, NS, CUS, lb_min, 0).depth}, 0};
            if (walk(qtiles, NS, CUS, lb_min, sp) < 0) return 1;
          } else if (pl.mode != RING_XCD) {
            printf("a split without leftover tiles (qtiles=%ld)\n", (long)qtiles);
            return 1;
          }
          ++checked;
        }
  printf("ring plans checked: %ld (split taken in %ld of %ld with leftover tiles)\n", checked, split_taken, split_possible);
  // the bench shape: 131 tiles x 7813 stages on 256 workgroups, lb_min = 8
  {
    const int64_t qtiles = 131, NS = 7813;
    const int CUS = 256, lb_min = 8;
    const RingPlan pl = ring_plan_choose(qtiles, NS, CUS, lb_min);
    RingPlan par{RING_XCD, {SegmentWalker::choose_depth(17, NS, 32, lb_min, 0).depth, SegmentWalker::choose_depth(16, NS, 32, lb_min, 0).depth}, 0};
    const int64_t parent = walk(qtiles, NS, CUS, lb_min, par), got = walk(qtiles, NS, CUS, lb_min, pl);
    const int64_t even = qtiles * NS / CUS;  // (3998.06 stages per workgroup)
    printf("bench shape 131 x 7813 x 256: mode %d, most loaded workgroup %ld stages (parent %ld, even %ld)\n", pl.mode, (long)got, (long)parent, (long)even);
    if (got < 0 || got > even + lb_min + 1) {
      printf("bench shape: %ld stages, more than %ld + lb_min + 1\n", (long)got, (long)even);
      return 1;
    }
  }
  return 0;
}
