"""What a filtered call EXECUTES, shape by shape: every branch of the call plan (csrc/filter_schedule.h: filter_call_plan) run
once on small banks, the result bit-equal to the fp32 kernel's, and the plan the call left behind -- the statistics words'
level count, per-level keys and int8 flags and speculative word, the attached profile's bound-pass flag and keys -- equal to
the row RECORDED FROM THE PARENT COMMIT'S LIBRARY on an MI355X, before the driver became an executor of that plan.
A deliberate change of the schedule must re-record the rows (tools/record_filter_call_plans.py)."""
import ctypes
import threading

import pytest
import torch

# (B, N, D, k): what the shape reaches (ragraph_topk_cosine_filtered_plan, tests/test_cpu_filter_plan.py)
SHAPES = {
    "direct_i8_sublists": (7, 70000, 256, 10),        # direct kernel, one int8 level, eight sub-lists
    "direct_two_i8": (64, 100000, 128, 10),           # direct, two int8 levels
    "direct_three_bf16_k32": (1, 65536, 256, 32),     # direct, three bf16 levels, k = 32
    "direct_scored": (200, 70000, 256, 10),           # direct, scored list
    "ring_one_bf16_wide": (300, 40000, 256, 10),      # ring, one bf16 level, wide rescoring
    "ring_one_i8_scored": (2100, 70000, 256, 10),     # ring, one int8 level, scored
    "ring_two_bf16_coop": (3000, 20000, 128, 10),     # two bf16 levels, coop rescoring
    "tile_branch_two_scored_i8": (17000, 66000, 256, 10),  # tile-kernel branch of the schedule, two scored int8 levels,
                                                           # wide prepare, small scored rescoring
    "three_levels_two_i8": (17000, 200000, 128, 10),  # three levels, the last two int8
    "d64_two_i8": (17000, 100000, 64, 10),            # D = 64, two int8 levels
    "exact_level0_tile": (300, 5000, 256, 10),        # exact level 0 on the tile kernel
    "exact_level0_slab": (300, 20000, 64, 32),        # exact level 0 as a slab, two levels
}
PRIOR_SHAPES = ("ring_one_bf16_wide", "ring_two_bf16_coop", "direct_i8_sublists")   # (the second: two levels become one)

# A single call: (levels, ((keys, int8), ...) per level, speculative word, bound pass ran, its keys).
# A sharded call: per rank that plan (None: the shard is an exact participant) and the phases its exchange saw.
RECORDED = {
    "d64_two_i8": (2, ((16384, 1), (83616, 1)), 0, 1, 6144),
    "direct_i8_sublists": (1, ((70000, 1),), 0, 1, 13568),
    "direct_scored": (1, ((70000, 1),), 0, 1, 9984),
    "direct_three_bf16_k32": (3, ((10496, 0), (15616, 0), (39424, 0)), 0, 1, 10496),
    "direct_two_i8": (2, ((20480, 1), (79520, 1)), 0, 1, 13568),
    "exact_level0_slab": (2, ((7168, 0), (12832, 0)), 0, 0, 0),
    "exact_level0_tile": (1, ((5000, 0),), 0, 0, 0),
    "ring_one_bf16_wide": (1, ((40000, 0),), 0, 1, 9984),
    "ring_one_i8_scored": (1, ((70000, 1),), 0, 1, 9984),
    "ring_two_bf16_coop": (2, ((7168, 0), (12832, 0)), 0, 1, 5120),
    "three_levels_two_i8": (3, ((16384, 0), (49152, 1), (134464, 1)), 0, 1, 5120),
    "tile_branch_two_scored_i8": (2, ((16384, 1), (49616, 1)), 0, 1, 5120),
    "ring_one_bf16_wide+prior": (1, ((40000, 0),), 1, 0, 0),
    "ring_two_bf16_coop+prior": (1, ((20000, 0),), 1, 0, 0),
    "direct_i8_sublists+prior": (1, ((70000, 1),), 1, 0, 0),
    "two_shards": ((
        (3, ((8192, 0), (24576, 1), (67232, 1)), 0, 1, 2560),
        (3, ((8192, 0), (24576, 1), (67232, 1)), 0, 1, 2560)),
        ((0, 1, 2), (0, 1, 2))),
    "two_shards+prior": ((
        (2, ((32768, 1), (67232, 1)), 1, 0, 0),
        (2, ((32768, 1), (67232, 1)), 1, 0, 0)),
        ((1,), (1,))),
    "three_shards": ((
        (1, ((40000, 0),), 0, 1, 3328),
        (1, ((20000, 0),), 0, 1, 1792),
        None),
        ((0,), (0,), (0,))),
}


_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _free_the_banks():
    """The banks, their copies, the queries and the fp32 results live on the device for this module only."""
    yield
    _cache.clear()
    torch.cuda.empty_cache()


def _bank(dev, N, D):
    """Random unit rows from a seeded generator, their filter copies: one bank per (N, D), shared and never written."""
    from ragraph_amd import kernels as K

    if ("bank", N, D) not in _cache:
        g = torch.Generator(device=dev).manual_seed(1000 + N % 997 + D)
        kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
        _cache["bank", N, D] = (kn, K.keys_to_bf16(kn))
    return _cache["bank", N, D]


def _case(dev, B, N, D, k):
    """(queries, bank, copies, the fp32 kernel's scores and indices): one zero query, one query equal to the last key."""
    from ragraph_amd import kernels as K

    if ("case", B, N, D, k) not in _cache:
        kn, kb = _bank(dev, N, D)
        g = torch.Generator(device=dev).manual_seed(B + 7 * k)
        q = torch.randn(B, D, device=dev, generator=g)
        q[0] = kn[N - 1]
        if B > 1:
            q[1] = 0
        s0, i0 = K.topk_cosine(q, kn, k)
        _cache["case", B, N, D, k] = (q, kn, kb, s0, i0)
    return _cache["case", B, N, D, k]


def _low_prior(s0, q):
    """The smallest true k-th best of the non-zero queries, minus 0.01: no query misses."""
    nonzero = q.abs().sum(dim=1) > 0
    return float(s0[nonzero, -1].min()) - 0.01


def _filtered_with_plan(q, kn, kb, k, read_plan=True, **kw):
    """K.topk_cosine_filtered with a profile attached to this thread -> (scores, idx, overflow, the executed plan).
    read_plan=False: an exact participant, which prepares no statistics words and times no filter launch."""
    from ragraph_amd import _native as N
    from ragraph_amd import kernels as K

    L = N.lib()
    prof = L.ragraph_filter_profile_create()
    assert prof
    L.ragraph_filter_profile_attach(prof)
    try:
        s, i, over, stats = K.topk_cosine_filtered(q, kn, kb, k, return_stats=True, **kw)
        st = [int(x) for x in stats.cpu()]
        ms, i8, keys = (ctypes.c_float * 4)(), (ctypes.c_int * 4)(), (ctypes.c_int64 * 4)()
        N.check(L.ragraph_filter_profile_levels(prof, ms, i8, keys), "profile_levels")
    finally:
        L.ragraph_filter_profile_attach(None)
        L.ragraph_filter_profile_destroy(prof)
    if not read_plan:
        return s, i, over, None
    assert st[0] == K.FILTER_STATS_MAGIC
    nlev = st[1]
    levels = tuple((st[11 + l], st[8 + l]) for l in range(nlev))
    assert [ms[l] >= 0 for l in range(3)] == [l < nlev for l in range(3)]           # the profile timed exactly these launches
    assert tuple((int(keys[l]), int(i8[l])) for l in range(nlev)) == levels         # ... over the same keys
    bound = ms[3] >= 0
    return s, i, over, (nlev, levels, st[16], int(bound), int(keys[3]) if bound else 0)


def single_call_plan(dev, name, with_prior):
    from ragraph_amd import kernels as K

    B, N, D, k = SHAPES[name]
    q, kn, kb, s0, i0 = _case(dev, B, N, D, k)
    if with_prior:
        K.set_filter_prior(_low_prior(s0, q))
    try:
        s, i, over, plan = _filtered_with_plan(q, kn, kb, k)
    finally:
        K.set_filter_prior(None)
    assert int(over) == 0
    assert torch.equal(i, i0) and torch.equal(s, s0)
    return plan


def sharded_call_plans(dev, name_or_shape, bounds, exact, with_prior):
    """Threads as ranks, one stream each, the exchanges through a barrier as ShardedToyGraphBase does them with RCCL (k-th of the
    union of every shard's best m values at every phase): merged lists == the fp32 kernel's over the whole bank, bit for
    bit.  -> (per rank: executed plan or None, per rank: phases seen)."""
    from ragraph_amd import kernels as K

    B, N, D, k = SHAPES.get(name_or_shape, name_or_shape)
    q, kn, kb, s0, i0 = _case(dev, B, N, D, k)
    G = len(bounds)
    plan_n = max(hi - lo for lo, hi in bounds)
    shards = [kn[lo:hi].contiguous() for lo, hi in bounds]
    copies = [K.keys_to_bf16(s) for s in shards]
    prior = _low_prior(s0, q) if with_prior else None
    torch.cuda.synchronize()
    barrier = threading.Barrier(G, timeout=60)
    slots, out, phases, errs = [None] * G, [None] * G, [[] for _ in range(G)], []
    m = min(k, 2 * (-(-k // G)))

    def exchange_for(r):
        def exchange(phase, theta, scores):
            phases[r].append(phase)
            torch.cuda.current_stream().synchronize()          # this shard's numbers are final
            slots[r] = scores[:, :m].clone()
            torch.cuda.current_stream().synchronize()
            barrier.wait()
            K.theta_sharpen(torch.stack(slots).contiguous(), theta, k)   # [G, B, m], as an all_gather leaves it
            torch.cuda.current_stream().synchronize()
            barrier.wait()
        exchange.n_shards = G
        return exchange

    def run(r):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                K.set_filter_prior(prior)                      # (thread-local: every rank sets the group's prior)
                try:
                    s, i, over, plan = _filtered_with_plan(q, shards[r], copies[r], k, read_plan=not exact[r],
                                                           idx_base=bounds[r][0], exchange=exchange_for(r), plan_n=plan_n)
                finally:
                    K.set_filter_prior(None)
                torch.cuda.current_stream().synchronize()
                out[r] = (s, i, int(over), plan)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    ms, mi = K.topk_merge(torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out]))
    assert torch.equal(mi, i0) and torch.equal(ms, s0)
    assert all(o[2] == 0 for o in out)
    return tuple(o[3] for o in out), tuple(tuple(p) for p in phases)


TWO_SHARDS = ("three_levels_two_i8", ((0, 100000), (100000, 200000)), (False, False))
# 40 000, 20 000 and 3 000 rows of one 63 000-row bank: the plan's shard, the rescaled shard, the exact participant
THREE_SHARDS = ((300, 63000, 256, 10), ((0, 40000), (40000, 60000), (60000, 63000)), (False, False, True))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_call_executes_the_recorded_plan(dev, name):
    assert single_call_plan(dev, name, False) == RECORDED[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", PRIOR_SHAPES)
def test_call_under_a_prior_executes_the_recorded_plan(dev, name):
    plan = single_call_plan(dev, name, True)
    assert plan[2] == 1 and plan[3] == 0           # the speculative word is set, and there is no bound pass
    assert plan == RECORDED[name + "+prior"]


@pytest.mark.gpu
@pytest.mark.parametrize("with_prior", (False, True))
def test_two_shards_execute_the_recorded_plans(dev, with_prior):
    plans, phases = sharded_call_plans(dev, *TWO_SHARDS, with_prior)
    if with_prior:   # no phase 0, and the two levels that the three-level plan (plan_N = 100 000) collapses to
        assert all(0 not in p for p in phases) and all(p[0] == 2 and p[2] == 1 for p in plans)
    else:
        assert all(p[0] == 0 for p in phases)
    assert (plans, phases) == RECORDED["two_shards+prior" if with_prior else "two_shards"]


@pytest.mark.gpu
def test_three_unequal_shards_execute_the_recorded_plans(dev):
    plans, phases = sharded_call_plans(dev, *THREE_SHARDS, False)
    assert phases[0] == phases[1] == phases[2] and phases[0][0] == 0
    assert (plans, phases) == RECORDED["three_shards"]

