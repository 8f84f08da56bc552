"""The filtered exact top-k for lists of 65 .. 128 keys, host side (no GPU): the three wide128 entries of the C ABI, what their
plan and size queries accept and refuse, the plans' level rule, the plans of every shorter list (unchanged: a table recorded
from the commit before this entry existed), the dispatch rule kernels.filter_wide128_helps, and KeyIndex's routing of such a k."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE128 = ("ragraph_topk_cosine_filtered_wide128_f32", "ragraph_topk_cosine_filtered_wide128_workspace_bytes",
           "ragraph_topk_cosine_filtered_wide128_plan")
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


def test_the_wide128_entries_exist_in_the_header_and_in_the_loader(lib):
    from ragraph_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ragraph_hip.h")).read()
    for name in WIDE128:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(lib, name), name
    for part in ("f32", "plan", "workspace_bytes"):   # each has the argument list of its _wide_ counterpart
        a, b = (getattr(lib, "ragraph_topk_cosine_filtered_%s_%s" % (w, part)) for w in ("wide128", "wide"))
        assert a.argtypes == b.argtypes and a.restype == b.restype, part
    assert _header_define("RAGRAPH_TOPK_FILTER_MAX") == N.TOPK_FILTER_MAX == 128
    assert _header_define("RAGRAPH_TOPK_MAX") == N.TOPK_MAX == 64


def test_one_path_per_k(lib):
    from ragraph_amd import _native as N

    plan = (ctypes.c_int64 * 7)()
    for k in (65, 96, 128):
        assert 1 <= lib.ragraph_topk_cosine_filtered_wide128_plan(300, 70_000, 256, k, plan) <= 3, k
        assert lib.ragraph_topk_cosine_filtered_wide128_workspace_bytes(300, 70_000, 256, k) > 0, k
    for k in (64, 129, 0):
        assert lib.ragraph_topk_cosine_filtered_wide128_plan(300, 70_000, 256, k, plan) == N.EINVAL, k
        assert lib.ragraph_topk_cosine_filtered_wide128_workspace_bytes(300, 70_000, 256, k) == 0, k
    assert lib.ragraph_topk_cosine_filtered_wide128_plan(300, 80, 256, 96, plan) == N.EINVAL          # k > N
    assert lib.ragraph_topk_cosine_filtered_wide128_workspace_bytes(300, 80, 256, 96) == 0
    assert lib.ragraph_topk_cosine_filtered_wide128_plan(300, 70_000, 256, 96, None) == N.EINVAL
    assert lib.ragraph_topk_cosine_filtered_wide128_plan(300, 70_000, 100, 96, plan) == N.EUNSUPPORTED
    assert lib.ragraph_topk_cosine_filtered_wide128_workspace_bytes(300, 70_000, 100, 96) == 0
    # the call itself checks its k before it touches a pointer it was given
    one = ctypes.c_int64(0)
    p = ctypes.addressof(one)
    for k in (64, 129):
        assert lib.ragraph_topk_cosine_filtered_wide128_f32(p, 300, p, None, p, 70_000, 256, k, 0, p, p, p, None, p, 1 << 30, None) == N.EINVAL
    assert lib.ragraph_topk_cosine_filtered_wide128_f32(p, 300, p, None, p, 70_000, 100, 96, 0, p, p, p, None, p, 1 << 30, None) == N.EUNSUPPORTED
    # the two existing entries refuse 65 as before
    assert lib.ragraph_topk_cosine_filtered_plan(300, 70_000, 256, 65, plan) == N.EINVAL
    assert lib.ragraph_topk_cosine_filtered_wide_plan(300, 70_000, 256, 65, plan) == N.EINVAL
    assert lib.ragraph_topk_cosine_filtered_wide_workspace_bytes(300, 70_000, 256, 65) == 0
    assert lib.ragraph_topk_cosine_filtered_f32(p, 300, p, None, p, 70_000, 256, 65, 0, p, p, p, None, p, 1 << 30, None) == N.EINVAL
    assert lib.ragraph_topk_cosine_filtered_wide_f32(p, 300, p, None, p, 70_000, 256, 65, 0, p, p, p, None, p, 1 << 30, None) == N.EINVAL


@pytest.mark.parametrize("k", (65, 128))
@pytest.mark.parametrize("B,N,D", SHAPES)
def test_plans_keep_every_level_to_half_a_list(lib, B, N, D, k):
    """1 <= L <= 3 levels, strictly increasing ends that finish at N, inner ends whole pads of 256 keys, a bound prefix of at
    most half the bank, and per level 1.3 k (end / previous end) <= 1024 (1 % for the rounding of the ends), half that where
    the plan marks the level int8 (its last ragraph_topk_cosine_filtered_wide128_i8_levels levels)."""
    plan = (ctypes.c_int64 * 7)()
    L = lib.ragraph_topk_cosine_filtered_wide128_plan(B, N, D, k, plan)
    w = list(plan)
    assert 1 <= L <= 3 and w[2] == L, w
    ends = w[3:3 + L]
    assert ends == sorted(set(ends)) and ends[-1] == N and all(e % 256 == 0 for e in ends[:-1]), w
    assert all(x == 0 for x in w[3 + L:6]), w
    assert w[1] in (0, 1, 2) and 0 <= w[6] <= N // 2 and w[0] >= 1, w
    n_i8 = lib.ragraph_topk_cosine_filtered_wide128_i8_levels(B, N, D, k)
    assert 0 <= n_i8 <= L
    prev = w[0]
    for l in range(L):
        cands = 1.3 * k * w[3 + l] / prev
        assert cands <= 1024 * 1.01, (l, w)
        if l >= L - n_i8:
            assert 2 * cands <= 1024 * 1.01, (l, w)
        prev = w[3 + l]
    assert lib.ragraph_topk_cosine_filtered_wide128_workspace_bytes(B, N, D, k) > 0
    if k == 65:
        assert lib.ragraph_topk_cosine_filtered_wide128_workspace_bytes(B, N, D, 65) >= \
            lib.ragraph_topk_cosine_filtered_wide_workspace_bytes(B, N, D, 64)


# ((B, N, D, k), levels, the seven plan words, workspace bytes) of the entries for k <= 32 (k = 10, 32) and 33 .. 64 (k = 33, 64),
# recorded from a build of the commit before the wide128 entry existed: nothing planned for a shorter list may move.
PLANS_UP_TO_64 = (
    ((100000, 1000000, 256, 10), 3, (15625, 2, 3, 62720, 250880, 1000000, 18944), 2008796672),
    ((100000, 1000000, 256, 32), 3, (15625, 2, 3, 62720, 250880, 1000000, 18944), 1211996672),
    ((100000, 1000000, 256, 33), 3, (15625, 2, 3, 62720, 250880, 1000000, 18944), 2234484224),
    ((100000, 1000000, 256, 64), 3, (15625, 2, 3, 62720, 250880, 1000000, 18944), 2234484224),
    ((65536, 4000000, 64, 10), 3, (62500, 2, 3, 249856, 1000448, 4000000, 75008), 606671104),
    ((65536, 4000000, 64, 32), 3, (62500, 2, 3, 249856, 1000448, 4000000, 75008), 641274112),
    ((65536, 4000000, 64, 33), 3, (62500, 2, 3, 249856, 1000448, 4000000, 75008), 1697997056),
    ((65536, 4000000, 64, 64), 3, (62500, 2, 3, 249856, 1000448, 4000000, 75008), 1697997056),
    ((20000, 300000, 128, 10), 3, (4687, 2, 3, 18944, 75776, 300000, 5632), 206796800),
    ((20000, 300000, 128, 32), 3, (4687, 2, 3, 18944, 75776, 300000, 18944), 224396800),
    ((20000, 300000, 128, 33), 3, (4687, 2, 3, 18944, 75776, 300000, 18944), 583996928),
    ((20000, 300000, 128, 64), 3, (4687, 2, 3, 18944, 75776, 300000, 18944), 583996928),
    ((4096, 1000000, 256, 10), 2, (32768, 2, 2, 181248, 1000000, 0, 39424), 618373376),
    ((4096, 1000000, 256, 32), 2, (131072, 2, 2, 362240, 1000000, 0, 157440), 2196873472),
    ((4096, 1000000, 256, 33), 2, (131072, 2, 2, 362240, 1000000, 0, 157440), 2196873472),
    ((4096, 1000000, 256, 64), 2, (131072, 2, 2, 362240, 1000000, 0, 157440), 2196873472),
    ((300, 70000, 256, 10), 1, (8192, 2, 1, 70000, 0, 0, 9984), 21687808),
    ((300, 70000, 256, 32), 1, (8192, 2, 1, 70000, 0, 0, 9984), 19335680),
    ((300, 70000, 256, 33), 1, (16384, 2, 1, 70000, 0, 0, 19712), 29611520),
    ((300, 70000, 256, 64), 1, (16384, 2, 1, 70000, 0, 0, 19712), 29706752),
)


def test_plans_and_sizes_of_shorter_lists_are_what_they_were(lib):
    assert {r[0][:3] for r in PLANS_UP_TO_64} == set(SHAPES)
    plan = (ctypes.c_int64 * 7)()
    for (B, N, D, k), L, words, size in PLANS_UP_TO_64:
        w = "wide_" if k > 32 else ""
        assert getattr(lib, "ragraph_topk_cosine_filtered_%splan" % w)(B, N, D, k, plan) == L, (B, N, D, k)
        assert tuple(plan) == words, (B, N, D, k, tuple(plan))
        assert getattr(lib, "ragraph_topk_cosine_filtered_%sworkspace_bytes" % w)(B, N, D, k) == size, (B, N, D, k)


def test_scored_lists_are_refused_beyond_64(lib, monkeypatch):
    """RAGRAPH_FILTER_SCORED=1 cannot reach a scored kernel at this width: the plan keeps plain lists.  The switch moves neither
    the plan words nor the int8 levels, and the call's own size stays that of 4-byte slots -- the size query moves only through
    its floor, the size of a list of 64, whose slots the same switch doubles."""
    shape = (2100, 40_000, 256)
    plan, plan1 = (ctypes.c_int64 * 7)(), (ctypes.c_int64 * 7)()
    L = lib.ragraph_topk_cosine_filtered_wide128_plan(*shape, 96, plan)
    i8 = lib.ragraph_topk_cosine_filtered_wide128_i8_levels(*shape, 96)
    plain = lib.ragraph_topk_cosine_filtered_wide128_workspace_bytes(*shape, 96)
    plain64 = lib.ragraph_topk_cosine_filtered_wide_workspace_bytes(*shape, 64)
    monkeypatch.setenv("RAGRAPH_FILTER_SCORED", "1")
    assert lib.ragraph_topk_cosine_filtered_wide128_plan(*shape, 96, plan1) == L and tuple(plan1) == tuple(plan)
    assert lib.ragraph_topk_cosine_filtered_wide128_i8_levels(*shape, 96) == i8
    scored64 = lib.ragraph_topk_cosine_filtered_wide_workspace_bytes(*shape, 64)
    assert scored64 > plain64
    assert lib.ragraph_topk_cosine_filtered_wide128_workspace_bytes(*shape, 96) == max(plain, scored64)


def test_filter_wide128_helps_truth_table(monkeypatch):
    from ragraph_amd import kernels as K

    monkeypatch.delenv("RAGRAPH_EXACT_FP32", raising=False)
    for k in (1, 32, 64, 129):                                      # one path per k: not this one's
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

    def __init__(self, rule128, wide_rule=True):
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


def test_key_index_routes_65_to_128_by_the_ops_own_rule():
    from ragraph_amd.kernels_index import KeyIndex

    ops = RecordingOps(True)
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

    ops = RecordingOps(True)
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

    ops = RecordingOps(False)
    route = _router(ops, KeyIndex(torch.zeros(200, 64), ops=ops, dedup=False))
    assert route(100) == ["topk_cosine"] and route(65) == ["topk_cosine"] and route(128) == ["topk_cosine"]
    assert route(41) == ["filter_wide_helps", "topk_cosine_filtered"]
