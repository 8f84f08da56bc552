"""The host queries under a TIGHT speculative bound (csrc/filter_schedule.h: filter_call_plan; no GPU): with both of the thread's
bounds set and the tight one above the prior, the plan of the bench shape is one level over the whole bank; with the tight bound
unset or at most the prior it is the recorded three; the workspace size queries never change."""
import ctypes

import pytest

BENCH = (100_000, 1_000_000, 256, 10)
SHAPES = [BENCH, (4096, 1_000_000, 256, 10), (300, 70_000, 256, 10), (700, 20_000, 128, 5), (1100, 70_000, 64, 8), (260, 70_000, 256, 10)]


@pytest.fixture()
def lib():
    from ragraph_amd import _native as N

    L = N.lib()
    yield L
    L.ragraph_topk_cosine_filtered_set_prior(float("nan"))
    L.ragraph_topk_cosine_filtered_set_tight_prior(float("nan"))


def _plan(L, shape):
    plan = (ctypes.c_int64 * 7)()
    rc = L.ragraph_topk_cosine_filtered_plan(*shape, plan)
    return rc, list(plan)


def test_the_setter_is_thread_local_state_that_returns_the_previous_value(lib):
    old = lib.ragraph_topk_cosine_filtered_set_tight_prior(0.25)
    assert old != old                                                       # NaN: the default
    assert lib.ragraph_topk_cosine_filtered_set_tight_prior(float("nan")) == 0.25


def test_both_bounds_set_plan_one_level_over_the_whole_bank(lib):
    rc0, plan0 = _plan(lib, BENCH)
    i8_0 = lib.ragraph_topk_cosine_filtered_i8_levels(*BENCH)
    assert rc0 == 3 and plan0[2] == 3 and plan0[5] == BENCH[1] and i8_0 >= 1      # the recorded three levels
    lib.ragraph_topk_cosine_filtered_set_prior(0.226)
    assert _plan(lib, BENCH) == (rc0, plan0)                                # the prior alone: the queries answer as ever
    for t in (float("nan"), 0.226, 0.2):                                    # unset, equal, below the prior: ignored
        lib.ragraph_topk_cosine_filtered_set_tight_prior(t)
        assert _plan(lib, BENCH) == (rc0, plan0) and lib.ragraph_topk_cosine_filtered_i8_levels(*BENCH) == i8_0
    lib.ragraph_topk_cosine_filtered_set_tight_prior(0.249)
    rc, plan = _plan(lib, BENCH)
    assert rc == 1 and plan[2] == 1 and plan[3] == BENCH[1] and plan[4] == 0 and plan[5] == 0
    assert lib.ragraph_topk_cosine_filtered_i8_levels(*BENCH) == 1          # ... on int8, as the last level was
    lib.ragraph_topk_cosine_filtered_set_prior(float("nan"))                # the tight bound without a prior: ignored
    assert _plan(lib, BENCH) == (rc0, plan0)


def test_a_shape_below_the_workspace_rule_keeps_its_plan(lib):
    small = (260, 1_000_000, 256, 10)
    rc0, plan0 = _plan(lib, small)
    lib.ragraph_topk_cosine_filtered_set_prior(0.2)
    lib.ragraph_topk_cosine_filtered_set_tight_prior(0.25)
    rc, plan = _plan(lib, small)
    # (the prior's own rule -- one level up to 4096 queries -- is what such a call runs; its ends are the plan's last)
    assert plan[3 + rc - 1] == small[1] and rc <= rc0


def test_workspace_sizes_do_not_depend_on_the_bounds(lib):
    sizes = [lib.ragraph_topk_cosine_filtered_workspace_bytes(*s) for s in SHAPES]
    sharded = [lib.ragraph_topk_cosine_filtered_sharded_workspace_bytes(*s, 2) for s in SHAPES]
    lib.ragraph_topk_cosine_filtered_set_prior(0.2)
    lib.ragraph_topk_cosine_filtered_set_tight_prior(0.25)
    assert [lib.ragraph_topk_cosine_filtered_workspace_bytes(*s) for s in SHAPES] == sizes
    assert [lib.ragraph_topk_cosine_filtered_sharded_workspace_bytes(*s, 2) for s in SHAPES] == sharded
