"""The filtered exact top-k for lists of 33 .. 64 keys, host side (no GPU): the three wide entries of the C ABI, what their
plan and size queries accept and refuse, the dispatch rule kernels.filter_wide_helps, and KeyIndex's routing of such a k."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = ("ragraph_topk_cosine_filtered_wide_f32", "ragraph_topk_cosine_filtered_wide_workspace_bytes",
        "ragraph_topk_cosine_filtered_wide_plan")


@pytest.fixture()
def lib(monkeypatch):
    from ragraph_amd import _native as N

    for name in ("RAGRAPH_TOPK_CUS", "RAGRAPH_FILTER_I8", "RAGRAPH_FILTER_SCORED", "RAGRAPH_EXACT_FP32"):
        monkeypatch.delenv(name, raising=False)
    return N.lib()


def test_the_wide_entries_exist_in_the_header_and_in_the_loader(lib):
    from ragraph_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ragraph_hip.h")).read()
    for name in WIDE:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    # the argument list of the entry for k <= 32
    assert lib.ragraph_topk_cosine_filtered_wide_f32.argtypes == lib.ragraph_topk_cosine_filtered_f32.argtypes
    assert lib.ragraph_topk_cosine_filtered_wide_plan.argtypes == lib.ragraph_topk_cosine_filtered_plan.argtypes


@pytest.mark.parametrize("D", (64, 128, 256))
@pytest.mark.parametrize("B,N", ((9, 70_000), (256, 70_000), (300, 70_000), (2100, 40_000), (4096, 1_000_000), (100_000, 1_000_000)))
def test_plan_and_size_queries_accept_33_to_64(lib, B, N, D):
    plan = (ctypes.c_int64 * 7)()
    for k in (33, 48, 64):
        L = lib.ragraph_topk_cosine_filtered_wide_plan(B, N, D, k, plan)
        w = list(plan)
        assert 1 <= L <= 3 and w[2] == L, (k, w)
        ends = w[3:3 + L]
        assert ends == sorted(set(ends)) and ends[-1] == N and all(e % 256 == 0 for e in ends[:-1]), (k, w)
        assert w[1] in (0, 1, 2) and 0 <= w[6] <= N // 2 and w[0] >= 1, (k, w)
        assert all(x == 0 for x in w[3 + L:6]), (k, w)
        assert lib.ragraph_topk_cosine_filtered_wide_workspace_bytes(B, N, D, k) > 0
    # a list of 33 needs no less room than a list of 32 does
    assert lib.ragraph_topk_cosine_filtered_wide_workspace_bytes(B, N, D, 33) >= \
        lib.ragraph_topk_cosine_filtered_workspace_bytes(B, N, D, 32)


def test_one_path_per_k(lib):
    from ragraph_amd import _native as N

    plan = (ctypes.c_int64 * 7)()
    for k in (32, 65, 0, 10):
        assert lib.ragraph_topk_cosine_filtered_wide_plan(300, 70_000, 256, k, plan) == N.EINVAL, k
        assert lib.ragraph_topk_cosine_filtered_wide_workspace_bytes(300, 70_000, 256, k) == 0, k
    assert lib.ragraph_topk_cosine_filtered_wide_plan(300, 40, 256, 48, plan) == N.EINVAL          # k > N
    assert lib.ragraph_topk_cosine_filtered_wide_plan(300, 70_000, 256, 48, None) == N.EINVAL
    assert lib.ragraph_topk_cosine_filtered_wide_plan(300, 70_000, 100, 48, plan) == N.EUNSUPPORTED
    assert lib.ragraph_topk_cosine_filtered_wide_workspace_bytes(300, 70_000, 100, 48) == 0
    # the entries for k <= 32 refuse what they refused
    assert lib.ragraph_topk_cosine_filtered_plan(300, 70_000, 256, 33, plan) == N.EINVAL
    assert lib.ragraph_topk_cosine_filtered_plan(300, 70_000, 256, 32, plan) >= 1
    # the call itself checks its k before it touches a pointer it was given
    one = ctypes.c_int64(0)
    p = ctypes.addressof(one)
    for k, code in ((32, N.EINVAL), (65, N.EINVAL)):
        assert lib.ragraph_topk_cosine_filtered_wide_f32(p, 300, p, None, p, 70_000, 256, k, 0, p, p, p, None, p, 1 << 30, None) == code
    assert lib.ragraph_topk_cosine_filtered_wide_f32(p, 300, p, None, p, 70_000, 100, 48, 0, p, p, p, None, p, 1 << 30, None) == N.EUNSUPPORTED
    assert lib.ragraph_topk_cosine_filtered_f32(p, 300, p, None, p, 70_000, 256, 33, 0, p, p, p, None, p, 1 << 30, None) == N.EINVAL


def test_plans_of_wide_lists_stay_under_the_list_capacity(lib):
    """The cost model's rule -- a level is planned for at most half the list capacity, 1.3 k (end / previous end) candidates,
    twice that on int8 -- also where the schedule is the fixed fractions of a large batch."""
    plan = (ctypes.c_int64 * 7)()
    for B, N, D in ((100_000, 1_000_000, 256), (65_536, 4_000_000, 64), (20_000, 300_000, 128), (4096, 1_000_000, 256)):
        L = lib.ragraph_topk_cosine_filtered_wide_plan(B, N, D, 64, plan)
        w = list(plan)
        prev = w[0]
        for l in range(L):
            assert 1.3 * 64 * w[3 + l] / prev <= 1024 * 1.01, (B, N, D, w)
            prev = w[3 + l]


def test_filter_wide_helps_truth_table(monkeypatch):
    from ragraph_amd import kernels as K

    monkeypatch.delenv("RAGRAPH_EXACT_FP32", raising=False)
    for k in (1, 10, 32, 65, 100):                                  # one path per k: not this one's
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


class RecordingOps:
    """Just enough of ragraph_amd.kernels for KeyIndex.topk's dispatch: every call is recorded, nothing is computed."""

    def __init__(self, wide_rule):
        self.calls = []
        if wide_rule:
            self.filter_wide_helps = lambda B, N, D, k: self.calls.append(("filter_wide_helps", B, N, D, k)) or True

    def filter_helps(self, B, N, D, k):
        self.calls.append(("filter_helps", B, N, D, k))
        return k <= 32

    def keys_to_bf16(self, kn):
        return torch.zeros(1, dtype=torch.int16)

    def _out(self, q, k):
        return torch.zeros(q.shape[0], k), torch.zeros(q.shape[0], k, dtype=torch.int64)

    def topk_cosine(self, q, kn, k, idx_base=0, keys_packed=None):
        self.calls.append(("topk_cosine", k))
        return self._out(q, k)

    def topk_cosine_filtered(self, q, kn, kb, k, idx_base=0, keys_packed=None):
        self.calls.append(("topk_cosine_filtered", k))
        return self._out(q, k) + (torch.zeros(1, dtype=torch.int32),)


@pytest.mark.parametrize("wide_rule", (True, False))
def test_key_index_routes_a_wide_k_by_the_ops_own_rule(wide_rule):
    from ragraph_amd.kernels_index import KeyIndex

    ops = RecordingOps(wide_rule)
    index = KeyIndex(torch.zeros(100, 64), ops=ops, dedup=False)
    q = torch.zeros(7, 64)

    def route(k):
        del ops.calls[:]
        s, i = index.topk(q, k)
        assert s.shape == (7, k) and i.shape == (7, k)
        return [c[0] for c in ops.calls]

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
