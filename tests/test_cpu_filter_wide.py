"""The filtered exact top-k for lists of 33 .. 128 keys, host side (no GPU): the one entry family of the C ABI takes every k (the
per-width entries are gone), what its plan, size and int8 queries and the call accept and refuse, the floor rule of the size
query, the plans' level rule, a table of plans and sizes recorded from the builds that introduced each width, the dispatch rules
kernels.filter_wide_helps / filter_wide128_helps, and KeyIndex's routing of such a k."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = ("ragraph_topk_cosine_filtered_f32", "ragraph_topk_cosine_filtered_plan", "ragraph_topk_cosine_filtered_workspace_bytes",
          "ragraph_topk_cosine_filtered_i8_levels")
REMOVED = ("ragraph_topk_cosine_filtered_wide_f32", "ragraph_topk_cosine_filtered_wide_plan",
           "ragraph_topk_cosine_filtered_wide_workspace_bytes", "ragraph_topk_cosine_filtered_wide128_f32",
           "ragraph_topk_cosine_filtered_wide128_plan", "ragraph_topk_cosine_filtered_wide128_workspace_bytes",
           "ragraph_topk_cosine_filtered_wide128_i8_levels")
SHAPES = ((100_000, 1_000_000, 256), (65_536, 4_000_000, 64), (20_000, 300_000, 128), (4096, 1_000_000, 256), (300, 70_000, 256))


@pytest.fixture()
def lib(monkeypatch):
    from ragraph_amd import _native as N

    for name in ("RAGRAPH_TOPK_CUS", "RAGRAPH_FILTER_I8", "RAGRAPH_FILTER_SCORED", "RAGRAPH_EXACT_FP32", "RAGRAPH_FILTER_FRACS",
                 "RAGRAPH_FILTER_TIGHT_LEVELS"):
        monkeypatch.delenv(name, raising=False)
    return N.lib()


def _header_define(name):
    header = open(os.path.join(ROOT, "include", "ragraph_hip.h")).read()
    return int(re.search(r"^#define %s (\d+)" % name, header, re.M).group(1))


def test_the_per_width_entries_are_gone_and_the_one_family_is_typed(lib):
    from ragraph_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ragraph_hip.h")).read()
    for name in REMOVED:   # (hasattr on a CDLL is a dlsym: the library's exports)
        assert name not in header and name not in N.SIGNATURES and not hasattr(lib, name), name
    for name in FAMILY:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    i64, i32 = ctypes.c_int64, ctypes.c_int
    assert lib.ragraph_topk_cosine_filtered_plan.argtypes == [i64, i64, i32, i32, ctypes.c_void_p]
    assert lib.ragraph_topk_cosine_filtered_workspace_bytes.argtypes == lib.ragraph_topk_cosine_filtered_i8_levels.argtypes == \
        [i64, i64, i32, i32]
    assert lib.ragraph_topk_cosine_filtered_workspace_bytes.restype is ctypes.c_size_t
    assert len(lib.ragraph_topk_cosine_filtered_f32.argtypes) == 16
    assert _header_define("RAGRAPH_TOPK_FILTER_MAX") == N.TOPK_FILTER_MAX == 128
    assert _header_define("RAGRAPH_TOPK_MAX") == N.TOPK_MAX == 64
    assert _header_define("RAGRAPH_ABI_VERSION") == lib.ragraph_abi_version() == 1


@pytest.mark.parametrize("D", (64, 128, 256))
@pytest.mark.parametrize("B,N", ((9, 70_000), (256, 70_000), (300, 70_000), (2100, 40_000), (4096, 1_000_000), (100_000, 1_000_000)))
def test_plan_and_size_queries_accept_33_to_64(lib, B, N, D):
    plan = (ctypes.c_int64 * 7)()
    for k in (33, 48, 64):
        L = lib.ragraph_topk_cosine_filtered_plan(B, N, D, k, plan)
        w = list(plan)
        assert 1 <= L <= 3 and w[2] == L, (k, w)
        ends = w[3:3 + L]
        assert ends == sorted(set(ends)) and ends[-1] == N and all(e % 256 == 0 for e in ends[:-1]), (k, w)
        assert w[1] in (0, 1, 2) and 0 <= w[6] <= N // 2 and w[0] >= 1, (k, w)
        assert all(x == 0 for x in w[3 + L:6]), (k, w)
        assert lib.ragraph_topk_cosine_filtered_workspace_bytes(B, N, D, k) > 0
    # a list of 33 needs no less room than a list of 32 does
    assert lib.ragraph_topk_cosine_filtered_workspace_bytes(B, N, D, 33) >= \
        lib.ragraph_topk_cosine_filtered_workspace_bytes(B, N, D, 32)


def _aligned16(nbytes=64):
    buf = ctypes.create_string_buffer(nbytes + 16)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_one_entry_family_takes_every_k(lib):
    """_plan, _workspace_bytes, _i8_levels and _f32 accept k = 1, 32, 33, 64, 65, 128 and refuse k = 0 and 129, k > N (the size
    query for k <= 32 excepted: it never looked at N), another D and a null plan; the call checks k and D before it touches a
    pointer, and insists on exactly the size its query reports; the sharded entry says why it refuses k = 33."""
    from ragraph_amd import _native as N

    plan = (ctypes.c_int64 * 7)()
    shape = (300, 70_000, 256)
    keep, a = _aligned16()
    one = ctypes.c_int64(0)
    p = ctypes.addressof(one)   # (8-byte aligned only: a call that got past its shape checks would refuse the alignment)

    def call(ptr, B, Nk, D, k, ws_bytes):
        return lib.ragraph_topk_cosine_filtered_f32(ptr, B, ptr, None, ptr, Nk, D, k, 0, ptr, ptr, ptr, None, ptr, ws_bytes, None)

    for k in (1, 32, 33, 64, 65, 128):
        assert 1 <= lib.ragraph_topk_cosine_filtered_plan(*shape, k, plan) <= 3 and plan[2] >= 1, k
        size = lib.ragraph_topk_cosine_filtered_workspace_bytes(*shape, k)
        assert size > 0, k
        assert 0 <= lib.ragraph_topk_cosine_filtered_i8_levels(*shape, k) <= plan[2], k
        # accepted by the call: it gets as far as the size, and insists on what the query reports -- not a byte less
        assert call(a, *shape, k, size - 1) == N.EWORKSPACE, k
        assert N.last_error() == "topk_cosine_filtered: workspace %d < %d" % (size - 1, size), k
    for k in (0, 129):
        assert lib.ragraph_topk_cosine_filtered_plan(*shape, k, plan) == N.EINVAL, k
        assert lib.ragraph_topk_cosine_filtered_workspace_bytes(*shape, k) == 0, k
        assert lib.ragraph_topk_cosine_filtered_i8_levels(*shape, k) == 0, k
        assert call(p, *shape, k, 1 << 30) == N.EINVAL and N.last_error() == "topk_cosine_filtered: bad B/N/k", k
    for Nk, k in ((20, 32), (40, 48), (80, 96)):                      # k > N, at every width
        assert lib.ragraph_topk_cosine_filtered_plan(300, Nk, 256, k, plan) == N.EINVAL, k
        assert lib.ragraph_topk_cosine_filtered_i8_levels(300, Nk, 256, k) == 0, k
        assert call(p, 300, Nk, 256, k, 1 << 30) == N.EINVAL and N.last_error() == "topk_cosine_filtered: bad B/N/k", k
        if k > 32:
            assert lib.ragraph_topk_cosine_filtered_workspace_bytes(300, Nk, 256, k) == 0, k
    for k in (48, 96):
        assert lib.ragraph_topk_cosine_filtered_workspace_bytes(0, 70_000, 256, k) == 0, k       # B < 1
        assert lib.ragraph_topk_cosine_filtered_plan(0, 70_000, 256, k, plan) == N.EINVAL, k
    for k in (10, 48, 96):
        assert lib.ragraph_topk_cosine_filtered_plan(300, 70_000, 256, k, None) == N.EINVAL, k
        assert lib.ragraph_topk_cosine_filtered_plan(300, 70_000, 100, k, plan) == N.EUNSUPPORTED, k
        assert lib.ragraph_topk_cosine_filtered_workspace_bytes(300, 70_000, 100, k) == 0, k
        assert lib.ragraph_topk_cosine_filtered_i8_levels(300, 70_000, 100, k) == 0, k
        assert call(p, 300, 70_000, 100, k, 1 << 30) == N.EUNSUPPORTED, k
    # no exchange for lists of more than 32 keys: the sharded entry names the reason, whatever else it was given
    rc = lib.ragraph_topk_cosine_filtered_sharded_f32(p, 300, p, None, p, 70_000, 256, 33, 0, p, p, p, None, p, 1 << 30, None,
                                                      70_000, None, None, None, 1)
    assert rc == N.EINVAL and "an exchange takes lists of up to 32 keys" in N.last_error(), N.last_error()
    del keep


def test_plans_of_wide_lists_stay_under_the_list_capacity(lib):
    """The cost model's rule -- a level is planned for at most half the list capacity, 1.3 k (end / previous end) candidates,
    twice that on int8 -- also where the schedule is the fixed fractions of a large batch."""
    plan = (ctypes.c_int64 * 7)()
    for B, N, D in ((100_000, 1_000_000, 256), (65_536, 4_000_000, 64), (20_000, 300_000, 128), (4096, 1_000_000, 256)):
        L = lib.ragraph_topk_cosine_filtered_plan(B, N, D, 64, plan)
        w = list(plan)
        prev = w[0]
        for l in range(L):
            assert 1.3 * 64 * w[3 + l] / prev <= 1024 * 1.01, (B, N, D, w)
            prev = w[3 + l]


@pytest.mark.parametrize("k", (33, 48, 64, 65, 128))
@pytest.mark.parametrize("B,N,D", SHAPES)
def test_plans_keep_every_level_to_half_a_list(lib, B, N, D, k):
    """1 <= L <= 3 levels, strictly increasing ends that finish at N, inner ends whole pads of 256 keys, a bound prefix of at
    most half the bank, and per level 1.3 k (end / previous end) <= 1024 (1 % for the rounding of the ends), half that where
    the plan marks the level int8 (its last ragraph_topk_cosine_filtered_i8_levels levels)."""
    plan = (ctypes.c_int64 * 7)()
    L = lib.ragraph_topk_cosine_filtered_plan(B, N, D, k, plan)
    w = list(plan)
    assert 1 <= L <= 3 and w[2] == L, w
    ends = w[3:3 + L]
    assert ends == sorted(set(ends)) and ends[-1] == N and all(e % 256 == 0 for e in ends[:-1]), w
    assert all(x == 0 for x in w[3 + L:6]), w
    assert w[1] in (0, 1, 2) and 0 <= w[6] <= N // 2 and w[0] >= 1, w
    n_i8 = lib.ragraph_topk_cosine_filtered_i8_levels(B, N, D, k)
    assert 0 <= n_i8 <= L
    prev = w[0]
    for l in range(L):
        cands = 1.3 * k * w[3 + l] / prev
        assert cands <= 1024 * 1.01, (l, w)
        if l >= L - n_i8:
            assert 2 * cands <= 1024 * 1.01, (l, w)
        prev = w[3 + l]
    assert lib.ragraph_topk_cosine_filtered_workspace_bytes(B, N, D, k) > 0
    if k == 65:   # a list of 65 needs no less room than a list of 64 does
        assert lib.ragraph_topk_cosine_filtered_workspace_bytes(B, N, D, 65) >= \
            lib.ragraph_topk_cosine_filtered_workspace_bytes(B, N, D, 64)


# ((B, N, D, k), levels, the seven plan words, workspace bytes, int8 levels): k = 10 .. 64 recorded from a build of the commit
# before lists of 65 .. 128 keys existed, k = 65 .. 128 and the int8 levels (None: no query answered for 33 .. 64 then) from the
# last build with one set of entries per list width.  Nothing planned may move.
PLANS_RECORDED = (
    ((100000, 1000000, 256, 10), 3, (15625, 2, 3, 62720, 250880, 1000000, 18944), 2008796672, 3),
    ((100000, 1000000, 256, 32), 3, (15625, 2, 3, 62720, 250880, 1000000, 18944), 1211996672, 2),
    ((100000, 1000000, 256, 33), 3, (15625, 2, 3, 62720, 250880, 1000000, 18944), 2234484224, None),
    ((100000, 1000000, 256, 64), 3, (15625, 2, 3, 62720, 250880, 1000000, 18944), 2234484224, None),
    ((100000, 1000000, 256, 65), 3, (15625, 2, 3, 62720, 250112, 1000000, 19968), 2285684224, 2),
    ((100000, 1000000, 256, 96), 3, (15625, 2, 3, 62720, 250112, 1000000, 21760), 2285684224, 2),
    ((100000, 1000000, 256, 128), 3, (15625, 2, 3, 62720, 250112, 1000000, 24064), 2285684224, 0),
    ((65536, 4000000, 64, 10), 3, (62500, 2, 3, 249856, 1000448, 4000000, 75008), 606671104, 2),
    ((65536, 4000000, 64, 32), 3, (62500, 2, 3, 249856, 1000448, 4000000, 75008), 641274112, 2),
    ((65536, 4000000, 64, 33), 3, (62500, 2, 3, 249856, 1000448, 4000000, 75008), 1697997056, None),
    ((65536, 4000000, 64, 64), 3, (62500, 2, 3, 249856, 1000448, 4000000, 75008), 1697997056, None),
    ((65536, 4000000, 64, 65), 3, (62500, 2, 3, 249856, 999936, 4000000, 79360), 1731551488, 2),
    ((65536, 4000000, 64, 96), 3, (62500, 2, 3, 249856, 999936, 4000000, 86272), 1731551488, 2),
    ((65536, 4000000, 64, 128), 3, (62500, 2, 3, 249856, 999936, 4000000, 95488), 1731551488, 0),
    ((20000, 300000, 128, 10), 3, (4687, 2, 3, 18944, 75776, 300000, 5632), 206796800, 2),
    ((20000, 300000, 128, 32), 3, (4687, 2, 3, 18944, 75776, 300000, 18944), 224396800, 2),
    ((20000, 300000, 128, 33), 3, (4687, 2, 3, 18944, 75776, 300000, 18944), 583996928, None),
    ((20000, 300000, 128, 64), 3, (4687, 2, 3, 18944, 75776, 300000, 18944), 583996928, None),
    ((20000, 300000, 128, 65), 3, (4687, 2, 3, 18944, 75008, 300000, 10496), 594236928, 2),
    ((20000, 300000, 128, 96), 3, (4687, 2, 3, 18944, 75008, 300000, 13568), 594236928, 2),
    ((20000, 300000, 128, 128), 3, (4687, 2, 3, 18944, 75008, 300000, 17152), 594236928, 0),
    ((4096, 1000000, 256, 10), 2, (32768, 2, 2, 181248, 1000000, 0, 39424), 618373376, 2),
    ((4096, 1000000, 256, 32), 2, (131072, 2, 2, 362240, 1000000, 0, 157440), 2196873472, 2),
    ((4096, 1000000, 256, 33), 2, (131072, 2, 2, 362240, 1000000, 0, 157440), 2196873472, None),
    ((4096, 1000000, 256, 64), 2, (131072, 2, 2, 362240, 1000000, 0, 157440), 2196873472, None),
    ((4096, 1000000, 256, 65), 2, (131072, 2, 2, 362240, 1000000, 0, 166400), 2196873472, 2),
    ((4096, 1000000, 256, 96), 2, (131072, 2, 2, 362240, 1000000, 0, 180736), 2196873472, 1),
    ((4096, 1000000, 256, 128), 2, (131072, 2, 2, 362240, 1000000, 0, 199936), 2196873472, 1),
    ((300, 70000, 256, 10), 1, (8192, 2, 1, 70000, 0, 0, 9984), 21687808, 0),
    ((300, 70000, 256, 32), 1, (8192, 2, 1, 70000, 0, 0, 9984), 19335680, 0),
    ((300, 70000, 256, 33), 1, (16384, 2, 1, 70000, 0, 0, 19712), 29611520, None),
    ((300, 70000, 256, 64), 1, (16384, 2, 1, 70000, 0, 0, 19712), 29706752, None),
    ((300, 70000, 256, 65), 1, (16384, 2, 1, 70000, 0, 0, 20992), 30170624, 0),
    ((300, 70000, 256, 96), 1, (16384, 2, 1, 70000, 0, 0, 22784), 30265856, 0),
    ((300, 70000, 256, 128), 1, (16384, 2, 1, 70000, 0, 0, 25088), 30364160, 0),
)


def test_recorded_plans_and_sizes_are_what_they_were(lib):
    assert {r[0][:3] for r in PLANS_RECORDED} == set(SHAPES)
    assert {r[0][3] for r in PLANS_RECORDED} == {10, 32, 33, 64, 65, 96, 128}
    plan = (ctypes.c_int64 * 7)()
    for (B, N, D, k), L, words, size, i8 in PLANS_RECORDED:
        assert lib.ragraph_topk_cosine_filtered_plan(B, N, D, k, plan) == L, (B, N, D, k)
        assert tuple(plan) == words, (B, N, D, k, tuple(plan))
        assert lib.ragraph_topk_cosine_filtered_workspace_bytes(B, N, D, k) == size, (B, N, D, k)
        if i8 is not None:
            assert lib.ragraph_topk_cosine_filtered_i8_levels(B, N, D, k) == i8, (B, N, D, k)


def test_scored_lists_are_refused_beyond_64(lib, monkeypatch):
    """RAGRAPH_FILTER_SCORED=1 cannot reach a scored kernel at this width: the plan keeps plain lists.  The switch moves neither
    the plan words nor the int8 levels, and the call's own size stays that of 4-byte slots -- the size query moves only through
    its floor, the size of a list of 64, whose slots the same switch doubles."""
    shape = (2100, 40_000, 256)
    plan, plan1 = (ctypes.c_int64 * 7)(), (ctypes.c_int64 * 7)()
    L = lib.ragraph_topk_cosine_filtered_plan(*shape, 96, plan)
    i8 = lib.ragraph_topk_cosine_filtered_i8_levels(*shape, 96)
    plain = lib.ragraph_topk_cosine_filtered_workspace_bytes(*shape, 96)
    plain64 = lib.ragraph_topk_cosine_filtered_workspace_bytes(*shape, 64)
    monkeypatch.setenv("RAGRAPH_FILTER_SCORED", "1")
    assert lib.ragraph_topk_cosine_filtered_plan(*shape, 96, plan1) == L and tuple(plan1) == tuple(plan)
    assert lib.ragraph_topk_cosine_filtered_i8_levels(*shape, 96) == i8
    scored64 = lib.ragraph_topk_cosine_filtered_workspace_bytes(*shape, 64)
    assert scored64 > plain64
    assert lib.ragraph_topk_cosine_filtered_workspace_bytes(*shape, 96) == max(plain, scored64)


def test_filter_wide_helps_truth_table(monkeypatch):
    from ragraph_amd import kernels as K

    monkeypatch.delenv("RAGRAPH_EXACT_FP32", raising=False)
    for k in (1, 10, 32, 65, 100):                                  # one rule per k: not this one's
        assert not K.filter_wide_helps(4096, 1_000_000, 256, k)
    for D in (32, 100, 512):
        assert not K.filter_wide_helps(4096, 1_000_000, D, 41)
    for B, N, D, k, want in WIDE_HELPS_TABLE:
        assert K.filter_wide_helps(B, N, D, k) is want, (B, N, D, k)
    assert not K.filter_helps(4096, 1_000_000, 256, 33)             # (unchanged: the rule for k <= 32 refuses 33)
    monkeypatch.setenv("RAGRAPH_EXACT_FP32", "1")
    for B, N, D, k, _ in WIDE_HELPS_TABLE:
        assert not K.filter_wide_helps(B, N, D, k)


# (B, n_keys, D, k, filtered?): the classes kernels.filter_wide_helps keeps, and their neighbours
WIDE_HELPS_TABLE = [
    (4096, 1_000_000, 256, 41, True), (4096, 1_000_000, 256, 33, True), (4096, 1_000_000, 256, 64, True),
    (100_000, 1_000_000, 256, 41, True), (256, 1_000_000, 256, 41, True), (4096, 4_000_000, 64, 64, True),
    (600, 70_000, 256, 41, True), (169_343, 169_343, 256, 41, True),
    (1, 1_000_000, 256, 41, True), (16, 70_000, 64, 64, True), (128, 40_000, 256, 64, True), (64, 40_000, 256, 41, False),
    (700, 20_000, 128, 41, True), (700, 20_000, 128, 64, False), (511, 20_000, 128, 41, False), (1024, 10_000, 256, 41, False),
    (2048, 20_000, 64, 33, True), (2047, 20_000, 64, 33, False), (8192, 10_000, 64, 41, False),
    (600, 5000, 256, 41, False), (16, 20_000, 128, 48, False),
]


def test_filter_wide128_helps_truth_table(monkeypatch):
    from ragraph_amd import kernels as K

    monkeypatch.delenv("RAGRAPH_EXACT_FP32", raising=False)
    for k in (1, 32, 64, 129):                                      # one rule per k: not this one's
        assert not K.filter_wide128_helps(4096, 1_000_000, 256, k)
    for D in (32, 100, 512):
        assert not K.filter_wide128_helps(4096, 1_000_000, D, 96)
    for B, N, D, k, want in WIDE128_HELPS_TABLE:
        assert K.filter_wide128_helps(B, N, D, k) is want, (B, N, D, k)
    for k in (65, 100):                                             # (unchanged: the rules for shorter lists refuse these)
        assert not K.filter_wide_helps(4096, 1_000_000, 256, k) and not K.filter_helps(4096, 1_000_000, 256, k)
    monkeypatch.setenv("RAGRAPH_EXACT_FP32", "1")
    for B, N, D, k, _ in WIDE128_HELPS_TABLE:
        assert not K.filter_wide128_helps(B, N, D, k)


# (B, n_keys, D, k, filtered?): the classes kernels.filter_wide128_helps keeps (profiles/filter_wide128.txt), and their neighbours
WIDE128_HELPS_TABLE = [
    (100_000, 1_000_000, 256, 65, True), (100_000, 1_000_000, 256, 128, True), (4096, 1_000_000, 256, 96, True),
    (256, 1_000_000, 256, 96, True), (1, 1_000_000, 256, 128, True), (16, 1_000_000, 128, 65, True), (64, 2_000_000, 256, 96, True),
    (4096, 200_000, 128, 96, True), (600, 70_000, 256, 82, True), (256, 70_000, 256, 128, True), (255, 70_000, 256, 96, False),
    (16, 999_999, 256, 96, False), (600, 65_536, 128, 100, True), (600, 65_535, 128, 100, False),
    (4096, 4_000_000, 64, 128, True), (4095, 4_000_000, 64, 96, False), (4096, 3_999_999, 64, 96, False), (16, 70_000, 64, 65, False),
    (2100, 40_000, 256, 96, True), (2048, 32_768, 256, 65, True), (2047, 40_000, 256, 96, False), (2100, 40_000, 128, 96, False),
    (2100, 32_767, 256, 96, False), (128, 40_000, 256, 65, False), (64, 40_000, 256, 96, False),
    (700, 20_000, 128, 65, False), (1024, 10_000, 256, 96, False), (2048, 20_000, 64, 65, False), (8192, 10_000, 64, 128, False),
    (169_343, 169_343, 256, 82, True),
]


class RecordingOps:
    """Just enough of ragraph_amd.kernels for KeyIndex.topk's dispatch: every call is recorded, nothing is computed."""

    def __init__(self, wide_rule=True, rule128=False):
        self.calls = []
        if wide_rule:
            self.filter_wide_helps = lambda B, N, D, k: self.calls.append(("filter_wide_helps", B, N, D, k)) or True
        if rule128:
            self.filter_wide128_helps = lambda B, N, D, k: self.calls.append(("filter_wide128_helps", B, N, D, k)) or True

    def filter_helps(self, B, N, D, k):
        self.calls.append(("filter_helps", B, N, D, k))
        return k <= 32

    def keys_to_bf16(self, kn):
        return torch.zeros(1, dtype=torch.int16)

    def normalize_rows(self, x):
        return x

    def _out(self, q, k):
        return torch.zeros(q.shape[0], k), torch.zeros(q.shape[0], k, dtype=torch.int64)

    def topk_cosine(self, q, kn, k, idx_base=0, keys_packed=None):
        self.calls.append(("topk_cosine", k))
        return self._out(q, k)

    def topk_cosine_filtered(self, q, kn, kb, k, idx_base=0, keys_packed=None):
        self.calls.append(("topk_cosine_filtered", k))
        return self._out(q, k) + (torch.zeros(1, dtype=torch.int32),)


def _router(ops, index):
    q = torch.zeros(7, 64)

    def route(k):
        del ops.calls[:]
        s, i = index.topk(q, k)
        assert s.shape == (7, k) and i.shape == (7, k)
        return [c[0] for c in ops.calls]
    return route


@pytest.mark.parametrize("wide_rule", (True, False))
def test_key_index_routes_a_wide_k_by_the_ops_own_rule(wide_rule):
    from ragraph_amd.kernels_index import KeyIndex

    ops = RecordingOps(wide_rule)
    index = KeyIndex(torch.zeros(100, 64), ops=ops, dedup=False)
    route = _router(ops, index)
    assert route(10) == ["filter_helps", "topk_cosine_filtered"]
    assert route(32) == ["filter_helps", "topk_cosine_filtered"]
    if wide_rule:
        assert route(41) == ["filter_wide_helps", "topk_cosine_filtered"] and ops.calls[0] == ("filter_wide_helps", 7, 100, 64, 41)
        assert route(33) == ["filter_wide_helps", "topk_cosine_filtered"]
        assert route(64) == ["filter_wide_helps", "topk_cosine_filtered"]
    else:                                           # an ops object without the rule keeps the fp32 score slabs
        assert route(41) == ["topk_cosine"]
        assert route(64) == ["topk_cosine"]
    assert route(100) == ["topk_cosine"]            # beyond the list limit: ordered large k, as ever
    index._filter_off = True                        # a bank that defeated the filter: no filtered call at any k
    assert route(41) == ["topk_cosine"]
    assert route(10) == ["topk_cosine"]


def test_key_index_routes_65_to_128_by_the_ops_own_rule():
    from ragraph_amd.kernels_index import KeyIndex

    ops = RecordingOps(rule128=True)
    index = KeyIndex(torch.zeros(200, 64), ops=ops, dedup=False)
    route = _router(ops, index)
    for k in (65, 100, 128):
        assert route(k) == ["filter_wide128_helps", "topk_cosine_filtered"], k
        assert ops.calls[0] == ("filter_wide128_helps", 7, 200, 64, k)
    assert route(129) == ["topk_cosine"]                       # beyond the longest filtered list: ordered large k, as ever
    assert route(41) == ["filter_wide_helps", "topk_cosine_filtered"]
    assert route(10) == ["filter_helps", "topk_cosine_filtered"]
    index._filter_off = True                                   # a bank that defeated the filter: no filtered call at any k
    assert route(100) == ["topk_cosine"]
    index._filter_off = False
    assert route(100) == ["filter_wide128_helps", "topk_cosine_filtered"]
    index._collapsed = (index, None, None)                     # searched through its unique rows: the expansion stops at 64
    assert route(100) == ["topk_cosine"]


def test_a_bank_with_a_tail_keeps_the_fp32_slabs_beyond_64():
    from ragraph_amd.kernels_index import KeyIndex

    ops = RecordingOps(rule128=True)
    ops.topk_cosine_tail = lambda q, kt, s, i, base: ops.calls.append(("topk_cosine_tail", s.shape[1])) or (s, i)
    index = KeyIndex(torch.zeros(200, 64), ops=ops, dedup=False)
    route = _router(ops, index)
    assert route(100) == ["filter_wide128_helps", "topk_cosine_filtered"]
    index.extend(torch.zeros(201, 64))                          # one appended row behind the sealed ones
    assert index.tail_rows == 1 and index.sealed_rows == 200
    assert route(100) == ["topk_cosine"] and index.tail_rows == 1
    assert route(41) == ["filter_wide_helps", "topk_cosine_filtered", "topk_cosine_tail"]   # (up to 64: sealed rows + tail pass)


def test_an_ops_object_without_the_rule_keeps_the_fp32_slabs():
    from ragraph_amd.kernels_index import KeyIndex

    ops = RecordingOps(rule128=False)
    route = _router(ops, KeyIndex(torch.zeros(200, 64), ops=ops, dedup=False))
    assert route(100) == ["topk_cosine"] and route(65) == ["topk_cosine"] and route(128) == ["topk_cosine"]
    assert route(41) == ["filter_wide_helps", "topk_cosine_filtered"]
