"""The host queries of the filtered top-k (csrc/topk_filter.hip, csrc/filter_schedule.h), on the host: no GPU.

Every number below was RECORDED FROM THE PARENT COMMIT'S LIBRARY, before the call plan (filter_call_plan) became the one
object that the driver, the size query and the three plan queries read.  They pin what those queries answer: a workspace
size that drifts from the call's carve-up is an out-of-bounds device write that no host check sees, and a plan query that
drifts from the call misleads the owner of a bank (kernels_index.py, sharded.py).  A deliberate change of the schedule or of
the workspace layout must re-record them.
(Without a device the CU count the schedule reads is 256, an MI355X's own; RAGRAPH_TOPK_CUS must not be set.)"""
import ctypes
import hashlib

import pytest

GRID_B = (1, 12, 40, 64, 65, 256, 257, 512, 1024, 2047, 2048, 4096, 8192, 16384, 16385, 100000)
GRID_N = (4096, 8191, 8192, 16383, 16384, 20000, 65535, 65536, 70003, 1000000, 4000000)
GRID_K = (1, 10, 16, 17, 32)
SHARDS_WS = (1, 2, 3, 8)
SHARDS_SPEC = (2, 4)
I8_WORD = 13   # position of ragraph_topk_cosine_filtered_i8_levels in a row of values


def values(L, B, N, D, k):
    """What the five host queries answer for one shape: workspace bytes, sharded workspace bytes for SHARDS_WS, the plan's
    seven words and its return value, the int8 level count, sharded_speculates for SHARDS_SPEC."""
    plan = (ctypes.c_int64 * 7)()
    rc = L.ragraph_topk_cosine_filtered_plan(B, N, D, k, plan)
    return ((L.ragraph_topk_cosine_filtered_workspace_bytes(B, N, D, k),)
            + tuple(L.ragraph_topk_cosine_filtered_sharded_workspace_bytes(B, N, D, k, G) for G in SHARDS_WS)
            + tuple(int(w) for w in plan) + (rc, L.ragraph_topk_cosine_filtered_i8_levels(B, N, D, k))
            + tuple(L.ragraph_topk_cosine_filtered_sharded_speculates(B, N, D, k, G) for G in SHARDS_SPEC))


def grid_digest(L, D):
    h = hashlib.sha256()
    for B in GRID_B:
        for N in GRID_N:
            for k in GRID_K:
                h.update((",".join(str(v) for v in values(L, B, N, D, k)) + ";").encode())
    return h.hexdigest()


@pytest.fixture()
def lib(monkeypatch):
    from ragraph_amd import _native as N

    for name in ("RAGRAPH_TOPK_CUS", "RAGRAPH_FILTER_I8", "RAGRAPH_FILTER_SCORED"):
        monkeypatch.delenv(name, raising=False)
    return N.lib()

# sha256 over values() of every (B, N, k) of the grid, in grid_digest's order
GRID_SHA256 = {
    64: "5935fa38f91873ab058c22509560d4b9239a6f0d8f4e329e7a1f695fe38ecb46",
    128: "a5818e1d291168e700e22d9124cb1d765bc23837365c4e1de7b166cfb22d0a7d",
    256: "fdd03277424675d52c0497df6f420c3d04732d3dc3915138630d0f74aef2857d",
}

# ((B, N, D, k), values(), int8 levels (default, RAGRAPH_FILTER_I8 = 0, 1, 2, thread cap 0)),  # what the shape reaches
ROWS = [
    ((7, 70000, 256, 10), (6909440, 6909440, 6909440, 6909440, 6909440, 4096, 2, 1, 70000, 0, 0, 13568, 1, 1, 1, 1),
     (1, 1, 1, 1, 0)),  # bound pass over 13568 keys, 1 level, 1 int8; speculates sharded 1/1
    ((64, 100000, 128, 10), (8511232, 25632768, 25632768, 25632768, 25632768, 4096, 2, 2, 20480, 100000, 0, 13568, 2, 2, 1, 1),
     (2, 2, 2, 2, 0)),  # bound pass over 13568 keys, 2 levels, 2 int8; speculates sharded 1/1
    ((1, 65536, 256, 32), (6407680, 6407680, 6407680, 6407680, 6407680, 4096, 2, 3, 10496, 26112, 65536, 10496, 3, 0, 1, 1),
     (0, 0, 0, 0, 0)),  # bound pass over 10496 keys, 3 levels, 0 int8; speculates sharded 1/1
    ((200, 70000, 256, 10), (16566016, 56204800, 56204800, 56204800, 56204800, 8192, 2, 1, 70000, 0, 0, 9984, 1, 1, 1, 1),
     (1, 1, 1, 1, 0)),  # bound pass over 9984 keys, 1 level, 1 int8; speculates sharded 1/1
    ((300, 40000, 256, 10), (21687808, 48307200, 48307200, 48307200, 48307200, 8192, 2, 1, 40000, 0, 0, 9984, 1, 0, 1, 1),
     (0, 0, 1, 1, 0)),  # bound pass over 9984 keys, 1 level, 0 int8; speculates sharded 1/1
    ((2100, 70000, 256, 10), (113676544, 113676544, 113676544, 113676544, 113676544, 8192, 2, 1, 70000, 0, 0, 9984, 1, 1, 1, 1),
     (1, 0, 1, 1, 0)),  # bound pass over 9984 keys, 1 level, 1 int8; speculates sharded 1/1
    ((3000, 20000, 128, 10), (83270144, 83270144, 83270144, 83270144, 83270144, 4096, 2, 2, 7168, 20000, 0, 5120, 2, 0, 1, 1),
     (0, 0, 1, 2, 0)),  # bound pass over 5120 keys, 2 levels, 0 int8; speculates sharded 1/1
    ((17000, 66000, 256, 10), (341299968, 341299968, 341299968, 428680192, 405968128, 4096, 2, 2, 16384, 66000, 0, 5120, 2, 2, 1, 1),
     (2, 0, 1, 2, 0)),  # bound pass over 5120 keys, 2 levels, 2 int8; speculates sharded 1/1
    ((17000, 200000, 128, 10), (178090752, 178090752, 178090752, 178090752, 178090752, 4096, 2, 3, 16384, 65536, 200000, 5120, 3, 2, 1, 1),
     (2, 0, 1, 2, 0)),  # bound pass over 5120 keys, 3 levels, 2 int8; speculates sharded 1/1
    ((17000, 100000, 64, 10), (166118144, 166118144, 299942144, 266894336, 266894336, 4096, 2, 2, 16384, 100000, 0, 6144, 2, 2, 1, 1),
     (2, 0, 1, 2, 0)),  # bound pass over 6144 keys, 2 levels, 2 int8; speculates sharded 1/1
    ((300, 5000, 256, 10), (17079808, 17079808, 17079808, 17079808, 17079808, 4096, 0, 1, 5000, 0, 0, 0, 1, 0, 0, 0),
     (0, 0, 1, 1, 0)),  # tile kernel over 4096 keys, 1 level, 0 int8
    ((300, 20000, 64, 32), (14005760, 24076800, 24076800, 24076800, 24076800, 4096, 1, 2, 7168, 20000, 0, 0, 2, 0, 0, 0),
     (0, 0, 1, 2, 0)),  # slab of 4096 keys, 2 levels, 0 int8
    ((100000, 1000000, 256, 10), (2008796672, 2008796672, 2008796672, 2008796672, 2008796672, 15625, 2, 3, 62720, 250880, 1000000, 18944, 3, 3, 1, 1),
     (3, 0, 1, 2, 0)),  # bound pass over 18944 keys, 3 levels, 3 int8; speculates sharded 1/1
    ((4096, 200000, 256, 10), (618373376, 618373376, 618373376, 618373376, 618373376, 32768, 2, 1, 200000, 0, 0, 39424, 1, 1, 1, 1),
     (1, 0, 1, 1, 0)),  # bound pass over 39424 keys, 1 level, 1 int8; speculates sharded 1/1
    ((1, 1000000, 256, 10), (6455552, 6455552, 6455552, 6455552, 6455552, 16384, 2, 1, 1000000, 0, 0, 54272, 1, 1, 1, 1),
     (1, 1, 1, 1, 0)),  # bound pass over 54272 keys, 1 level, 1 int8; speculates sharded 1/1
    ((16, 1000000, 256, 10), (11596032, 11596032, 11596032, 11596032, 11596032, 65536, 2, 1, 1000000, 0, 0, 216576, 1, 1, 1, 1),
     (1, 1, 1, 1, 0)),  # bound pass over 216576 keys, 1 level, 1 int8; speculates sharded 1/1
    ((17, 1000000, 256, 32), (9170432, 9170432, 9170432, 9170432, 9170432, 32768, 2, 2, 181248, 1000000, 0, 146432, 2, 2, 1, 1),
     (2, 2, 2, 2, 0)),  # bound pass over 146432 keys, 2 levels, 2 int8; speculates sharded 1/1
    ((64, 1000000, 256, 10), (24297216, 24297216, 24297216, 24297216, 24297216, 65536, 2, 1, 1000000, 0, 0, 216576, 1, 1, 1, 1),
     (1, 1, 1, 1, 0)),  # bound pass over 216576 keys, 1 level, 1 int8; speculates sharded 1/1
    ((65, 1000000, 256, 10), (41601536, 41601536, 41601536, 41601536, 41601536, 131072, 2, 1, 1000000, 0, 0, 157440, 1, 1, 1, 1),
     (1, 1, 1, 1, 0)),  # bound pass over 157440 keys, 1 level, 1 int8; speculates sharded 1/1
    ((128, 1000000, 256, 10), (75770880, 75770880, 75770880, 75770880, 75770880, 131072, 2, 1, 1000000, 0, 0, 157440, 1, 1, 1, 1),
     (1, 1, 1, 1, 0)),  # bound pass over 157440 keys, 1 level, 1 int8; speculates sharded 1/1
    ((129, 1000000, 256, 10), (76338944, 76338944, 76338944, 76338944, 76338944, 131072, 2, 1, 1000000, 0, 0, 131072, 1, 1, 1, 1),
     (1, 1, 1, 1, 0)),  # bound pass over 131072 keys, 1 level, 1 int8; speculates sharded 1/1
    ((256, 1000000, 256, 10), (145245696, 145245696, 145245696, 145245696, 145245696, 131072, 2, 1, 1000000, 0, 0, 131072, 1, 1, 1, 1),
     (1, 1, 1, 1, 0)),  # bound pass over 131072 keys, 1 level, 1 int8; speculates sharded 1/1
    ((257, 1000000, 256, 10), (78443008, 78443008, 78443008, 78443008, 78443008, 65536, 2, 1, 1000000, 0, 0, 78848, 1, 1, 1, 1),
     (1, 0, 1, 1, 0)),  # bound pass over 78848 keys, 1 level, 1 int8; speculates sharded 1/1
    ((1023, 1000000, 256, 10), (561553664, 561553664, 561553664, 561553664, 561553664, 131072, 2, 1, 1000000, 0, 0, 157440, 1, 1, 1, 1),
     (1, 0, 1, 1, 0)),  # bound pass over 157440 keys, 1 level, 1 int8; speculates sharded 1/1
    ((1024, 1000000, 256, 10), (562095360, 562095360, 562095360, 562095360, 562095360, 131072, 2, 1, 1000000, 0, 0, 157440, 1, 1, 1, 1),
     (1, 0, 1, 1, 0)),  # bound pass over 157440 keys, 1 level, 1 int8; speculates sharded 1/1
    ((2047, 1000000, 256, 10), (580744448, 580744448, 580744448, 580744448, 580744448, 65536, 2, 2, 256000, 1000000, 0, 78848, 2, 2, 1, 1),
     (2, 0, 1, 2, 0)),  # bound pass over 78848 keys, 2 levels, 2 int8; speculates sharded 1/1
    ((2048, 1000000, 256, 10), (312334592, 312334592, 312334592, 580770048, 580770048, 32768, 2, 2, 181248, 1000000, 0, 39424, 2, 2, 1, 1),
     (2, 0, 1, 2, 0)),  # bound pass over 39424 keys, 2 levels, 2 int8; speculates sharded 1/1
    ((2048, 1000000, 256, 17), (564222208, 564222208, 564222208, 564222208, 564222208, 65536, 2, 2, 256000, 1000000, 0, 78848, 2, 2, 1, 1),
     (2, 0, 1, 2, 0)),  # bound pass over 78848 keys, 2 levels, 2 int8; speculates sharded 1/1
    ((8192, 1000000, 256, 10), (1230450944, 1230450944, 1230450944, 2304192768, 2304192768, 32768, 2, 2, 181248, 1000000, 0, 39424, 2, 2, 1, 1),
     (2, 0, 1, 2, 0)),  # bound pass over 39424 keys, 2 levels, 2 int8; speculates sharded 1/1
    ((16384, 1000000, 256, 10), (1380864256, 1380864256, 1380864256, 4602089728, 4602089728, 16384, 2, 3, 64512, 254208, 1000000, 19712, 3, 3, 1, 1),
     (3, 0, 1, 2, 0)),  # bound pass over 19712 keys, 3 levels, 3 int8; speculates sharded 1/1
    ((16385, 1000000, 256, 10), (329188096, 329188096, 329188096, 329188096, 329188096, 15625, 2, 3, 62720, 250880, 1000000, 18944, 3, 3, 1, 1),
     (3, 0, 1, 2, 0)),  # bound pass over 18944 keys, 3 levels, 3 int8; speculates sharded 1/1
    ((512, 8191, 128, 10), (19757824, 19757824, 19757824, 19757824, 19757824, 4096, 0, 1, 8191, 0, 0, 0, 1, 0, 0, 0),
     (0, 0, 1, 1, 0)),  # tile kernel over 4096 keys, 1 level, 0 int8
    ((512, 8192, 128, 10), (19757824, 19757824, 19757824, 19757824, 19757824, 4096, 2, 1, 8192, 0, 0, 2048, 1, 0, 1, 1),
     (0, 0, 1, 1, 0)),  # bound pass over 2048 keys, 1 level, 0 int8; speculates sharded 1/1
    ((2048, 32767, 256, 10), (77453568, 77453568, 77453568, 77453568, 77453568, 4096, 2, 1, 32767, 0, 0, 5120, 1, 0, 1, 1),
     (0, 0, 1, 1, 0)),  # bound pass over 5120 keys, 1 level, 0 int8; speculates sharded 1/1
    ((2048, 32768, 256, 10), (77453568, 77453568, 77453568, 77453568, 77453568, 4096, 2, 1, 32768, 0, 0, 5120, 1, 1, 1, 1),
     (1, 0, 1, 1, 0)),  # bound pass over 5120 keys, 1 level, 1 int8; speculates sharded 1/1
    ((2048, 65535, 128, 10), (92395776, 92395776, 92395776, 92395776, 92395776, 8192, 2, 1, 65535, 0, 0, 9984, 1, 0, 1, 1),
     (0, 0, 1, 1, 0)),  # bound pass over 9984 keys, 1 level, 0 int8; speculates sharded 1/1
    ((2048, 65536, 128, 10), (92395776, 92395776, 92395776, 92395776, 92395776, 8192, 2, 1, 65536, 0, 0, 9984, 1, 0, 1, 1),
     (0, 0, 1, 1, 0)),  # bound pass over 9984 keys, 1 level, 0 int8; speculates sharded 1/1
    ((100000, 16383, 64, 10), (930396672, 930396672, 930396672, 930396672, 1119196672, 4096, 2, 1, 16383, 0, 0, 3840, 1, 0, 1, 1),
     (0, 0, 1, 1, 0)),  # bound pass over 3840 keys, 1 level, 0 int8; speculates sharded 1/1
    ((100000, 16384, 64, 10), (930396672, 930396672, 930396672, 930396672, 1119196672, 4096, 2, 1, 16384, 0, 0, 4096, 1, 0, 1, 1),
     (0, 0, 1, 1, 0)),  # bound pass over 4096 keys, 1 level, 0 int8; speculates sharded 1/1
    ((65536, 4000000, 64, 10), (606671104, 606671104, 606671104, 606671104, 606671104, 62500, 2, 3, 249856, 1000448, 4000000, 75008, 3, 2, 1, 1),
     (2, 0, 1, 2, 0)),  # bound pass over 75008 keys, 3 levels, 2 int8; speculates sharded 1/1
    ((50000, 2000000, 128, 10), (507553536, 507553536, 507553536, 507553536, 507553536, 31250, 2, 3, 125184, 500736, 2000000, 37632, 3, 2, 1, 1),
     (2, 0, 1, 2, 0)),  # bound pass over 37632 keys, 3 levels, 2 int8; speculates sharded 1/1
    ((2708, 10000, 128, 10), (77167360, 77167360, 77167360, 77167360, 77167360, 4096, 2, 1, 10000, 0, 0, 2304, 1, 0, 1, 1),
     (0, 0, 1, 1, 0)),  # bound pass over 2304 keys, 1 level, 0 int8; speculates sharded 1/1
]


@pytest.mark.parametrize("D", sorted(GRID_SHA256))
def test_host_queries_over_the_grid_equal_the_recorded_digest(lib, D):
    assert grid_digest(lib, D) == GRID_SHA256[D]


@pytest.mark.parametrize("shape,base,i8", ROWS)
def test_host_queries_equal_the_recorded_rows(lib, shape, base, i8):
    assert values(lib, *shape) == base


@pytest.mark.parametrize("shape,base,i8", ROWS)
@pytest.mark.parametrize("force", (0, 1, 2))
def test_forced_int8_levels_change_the_level_count_only(lib, monkeypatch, shape, base, i8, force):
    monkeypatch.setenv("RAGRAPH_FILTER_I8", str(force))      # (read per call)
    assert values(lib, *shape) == base[:I8_WORD] + (i8[1 + force],) + base[I8_WORD + 1:]


@pytest.mark.parametrize("shape,base,i8", ROWS)
def test_thread_cap_zero_changes_the_level_count_only(lib, shape, base, i8):
    old = lib.ragraph_topk_cosine_filtered_max_i8_levels(0)
    try:
        got = values(lib, *shape)
    finally:
        lib.ragraph_topk_cosine_filtered_max_i8_levels(-1)
    assert old == -1
    assert got == base[:I8_WORD] + (i8[4],) + base[I8_WORD + 1:]


def test_queries_refuse_what_the_call_refuses(lib):
    from ragraph_amd import _native as N

    plan = (ctypes.c_int64 * 7)()
    assert lib.ragraph_topk_cosine_filtered_plan(16, 100000, 100, 10, plan) == N.EUNSUPPORTED
    assert N.last_error() == "topk_cosine_filtered_plan: D=100 not in {64,128,256}"
    for bad in ((0, 100000, 256, 10), (16, 0, 256, 10), (16, 100000, 256, 0), (16, 100000, 256, 129), (16, 5, 256, 10)):
        assert lib.ragraph_topk_cosine_filtered_plan(*bad, plan) == N.EINVAL
        assert N.last_error() == "topk_cosine_filtered_plan: bad B/N/k"
        assert lib.ragraph_topk_cosine_filtered_i8_levels(*bad) == 0
        assert lib.ragraph_topk_cosine_filtered_sharded_speculates(*bad, 2) == 0
    assert lib.ragraph_topk_cosine_filtered_sharded_speculates(16, 100000, 256, 33, 2) == 0   # (no exchange beyond 32 keys)
    assert lib.ragraph_topk_cosine_filtered_plan(16, 100000, 256, 10, None) == N.EINVAL
    assert lib.ragraph_topk_cosine_filtered_sharded_speculates(16, 100000, 256, 10, 0) == 0
    assert lib.ragraph_topk_cosine_filtered_workspace_bytes(16, 100000, 100, 10) == 0
    assert lib.ragraph_topk_cosine_filtered_sharded_workspace_bytes(16, 100000, 100, 10, 2) == 0
