"""The filtered exact top-k for lists of 33 .. 64 keys (ragraph_topk_cosine_filtered_f32 at its list width of 64, behind
kernels.topk_cosine_filtered): every result is held, bit for bit, to K.topk_cosine on the same tensors -- the fp32 score
slabs, which existing tests hold to the oracle.  No tolerance anywhere."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the smallest shapes that reach each kernel form
RING = [(300, 70_000, 256),    # int8 ring, one ragged tile
        (2100, 40_000, 256),   # from 2048 queries: the one-wave-per-query rescoring (scored lists when they are switched on)
        (700, 20_000, 128),    # a bf16 level
        (1100, 70_000, 64)]    # the eight-group D = 64 form
DIRECT = [(9, 70_000, 256),    # direct kernel, sliced lists for <= 64 queries
          (100, 70_000, 128),
          (256, 70_000, 256)]
KS = (33, 48, 64)
_BANK, _REF = {}, {}


def _bank(dev, B, N, D):
    from ragraph_amd import kernels as K

    if (B, N, D) not in _BANK:
        g = torch.Generator(device=dev).manual_seed(2000 + B + D)
        kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
        _BANK[(B, N, D)] = (kn, K.keys_to_bf16(kn), torch.randn(B, D, device=dev, generator=g))
    return _BANK[(B, N, D)]


def _case(dev, B, N, D, k):
    """Bank, queries and the fp32 reference of a shape and k, computed once and shared (read-only) by the tests."""
    from ragraph_amd import kernels as K

    kn, kb, q = _bank(dev, B, N, D)
    if (B, N, D, k) not in _REF:
        _REF[(B, N, D, k)] = K.topk_cosine(q, kn, k)
    return (kn, kb, q) + tuple(_REF[(B, N, D, k)])


def _call(K, q, kn, kb, k, prior=None, tight=None):
    K.set_filter_prior(prior)
    K.set_filter_tight_prior(tight)
    try:
        s, i, over, st = K.topk_cosine_filtered(q, kn, kb, k, return_stats=True)
        w = st.cpu().tolist()
    finally:
        K.set_filter_prior(None)
        K.set_filter_tight_prior(None)
    return s, i, int(over), w


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("B,N,D", RING + DIRECT)
def test_no_prior_every_shape_matches_the_fp32_path(dev, B, N, D, k):
    from ragraph_amd import kernels as K

    kn, kb, q, s32, i32 = _case(dev, B, N, D, k)
    s, i, over, w = _call(K, q, kn, kb, k)
    assert w[0] == K.FILTER_STATS_MAGIC and w[14] == B and w[16] == 0, w[:24]
    assert torch.equal(i, i32) and torch.equal(s, s32)
    assert over == 0 and w[20] == 0, (over, w[:24])


@pytest.mark.parametrize("k", (33, 64))
@pytest.mark.parametrize("B,N,D", (DIRECT[0], RING[0]))
def test_the_int8_level_query_answers_what_the_call_runs(dev, B, N, D, k):
    """ragraph_topk_cosine_filtered_i8_levels for 33 .. 64 keys (no such query existed per list width): without a prior it is
    the number of trailing int8 levels in the call's own statistics words, in both launch families."""
    from ragraph_amd import kernels as K

    kn, kb, q = _bank(dev, B, N, D)
    s, i, over, w = _call(K, q, kn, kb, k)
    ran = [dt for dt, _, _ in K.filter_stats_levels(w)]
    assert len(ran) == w[1] >= 1, w[:24]
    trailing = 0
    while trailing < len(ran) and ran[len(ran) - 1 - trailing] == "int8":
        trailing += 1
    assert K.filtered_i8_levels(B, N, D, k) == trailing, (ran, w[:24])


@pytest.mark.parametrize("k", KS)
def test_scored_lists_switched_on(dev, k, monkeypatch):
    """Lists of more than 16 keys are plain by rule; RAGRAPH_FILTER_SCORED=1 (read per call) sends the int8 levels of this shape
    through the scored rescoring in its form for 64 winners -- without a running result, and merging one under a tight bound."""
    from ragraph_amd import kernels as K

    B, N, D = RING[1]
    kn, kb, q, s32, i32 = _case(dev, B, N, D, k)
    kth = torch.sort(s32[:, k - 1]).values
    monkeypatch.setenv("RAGRAPH_FILTER_SCORED", "1")
    s, i, over, w = _call(K, q, kn, kb, k)
    assert torch.equal(i, i32) and torch.equal(s, s32) and over == 0
    assert any(w[8 + l] for l in range(w[1])), w[:24]          # an int8 level ran: its lists were scored
    s, i, over, w = _call(K, q, kn, kb, k, float(kth[0]) - 0.01, float(kth[100]))
    assert torch.equal(i, i32) and torch.equal(s, s32) and over == 0
    assert w[21] == 1 and w[22] == int((s32[:, k - 1] < float(kth[100])).sum()) and w[23] == 1, w[14:24]


@pytest.mark.parametrize("B,N,D", RING)
def test_forced_priors_are_exact(dev, B, N, D):
    from ragraph_amd import kernels as K

    k = 48
    kn, kb, q, s32, i32 = _case(dev, B, N, D, k)
    kth = s32[:, k - 1]
    for what, p in (("below every k-th best", float(kth.min()) - 0.01), ("the median", float(kth.median())),
                    ("above every score", 1.5)):
        s, i, over, w = _call(K, q, kn, kb, k, p)
        assert torch.equal(i, i32) and torch.equal(s, s32), what
        missed = int((kth < p).sum())
        assert w[16] == 1 and w[17] == missed and over == missed and w[20] == missed, (what, missed, over, w[14:24])


@pytest.mark.parametrize("B,N,D", [RING[0], RING[1]])
def test_forced_tight_bounds_are_exact(dev, B, N, D):
    from ragraph_amd import kernels as K

    k = 64
    kn, kb, q, s32, i32 = _case(dev, B, N, D, k)
    kth = s32[:, k - 1]
    srt = torch.sort(kth).values
    lo, hi = float(srt[0]), float(srt[-1])
    safe = lo - 0.01
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    cases = [("no soft miss", safe, f32(lo - 0.005)),
             ("one soft miss", safe, float((srt[0] + srt[1]) * 0.5)),
             ("about 100 soft misses", safe, float(srt[100])),
             ("more than 256 soft misses", safe, float(srt[B - 10])),
             ("above every score: every list empty", safe, 1.5),
             ("hard and soft misses in one call", float(srt[B // 10]), float(srt[B // 2]))]
    for what, p, t in cases:
        s, i, over, w = _call(K, q, kn, kb, k, p, t)
        assert torch.equal(i, i32) and torch.equal(s, s32), what
        soft, hard = int((kth < t).sum()), int((kth < p).sum())
        assert w[0] == K.FILTER_STATS_MAGIC and w[16] == 1 and w[21] == 1 and w[1] == 1, (what, w[14:24])
        assert w[22] == soft and w[17] == hard and over == hard, (what, soft, hard, w[14:24], over)
        assert w[23] == (0 if soft == 0 else (1 if soft <= 256 else 2)), (what, soft, w[21:24])
        if hard == 0:
            assert abs(K.ord2f(w[18]) - lo) < 1e-6 and abs(K.ord2f(w[19]) - hi) < 1e-6, (what, w[18:20])


@pytest.mark.parametrize("B", (9, 300))
def test_ties_come_back_in_index_order(dev, B):
    """200 rows of the bank are copies of one row; queries equal to that row and near it: equal scores, ascending indices."""
    from ragraph_amd import kernels as K

    k = 64
    g = torch.Generator(device=dev).manual_seed(31 + B)
    kn = K.normalize_rows(torch.randn(70_000, 256, device=dev, generator=g))
    rows = torch.randperm(70_000, device=dev, generator=g)[:200]
    kn[rows] = kn[rows[0]].clone()
    q = torch.randn(B, 256, device=dev, generator=g)
    q[0] = kn[rows[0]]
    q[B - 1] = kn[rows[0]] * 3.0
    for r in range(1, min(B - 1, 6)):
        q[r] = kn[rows[0]] + 0.02 * r * torch.randn(256, device=dev, generator=g)
    s32, i32 = K.topk_cosine(q, kn, k)
    s, i, over, w = _call(K, q, kn, K.keys_to_bf16(kn), k)
    assert torch.equal(i, i32) and torch.equal(s, s32) and over == 0
    first = torch.sort(rows).values[:k]
    assert torch.equal(i[0], first) and torch.equal(i[B - 1], first)        # the copies, lowest rows first
    assert bool((s[0] == s[0, 0]).all())
    for r in range(B):                                                     # canonical order in every row
        ties = s[r, 1:] == s[r, :-1]
        assert bool((s[r, 1:] <= s[r, :-1]).all()) and bool((i[r, 1:][ties] > i[r, :-1][ties]).all()), r


def test_zero_queries_and_an_overflowing_cluster(dev):
    """Zero queries (answered without work, never counted) and a query next to 3000 near-duplicate keys, whose list overflows
    (the exact scan, in its form for 64 winners): without a bound, under a prior, and under tight bounds with either repair."""
    from ragraph_amd import kernels as K

    k = 48
    g = torch.Generator(device=dev).manual_seed(77)
    kn = K.normalize_rows(torch.randn(70_000, 256, device=dev, generator=g))
    kn[5000:8000] = K.normalize_rows(kn[7] + 0.0005 * torch.randn(3000, 256, device=dev, generator=g))
    q = torch.randn(600, 256, device=dev, generator=g)
    q[3] = 0.0
    q[599] = 0.0
    q[100] = kn[7] + 0.001 * torch.randn(256, device=dev, generator=g)
    kb = K.keys_to_bf16(kn)
    s32, i32 = K.topk_cosine(q, kn, k)
    kth = s32[:, k - 1]
    live = torch.ones(600, dtype=torch.bool, device=dev)
    live[[3, 100, 599]] = False
    srt = torch.sort(kth[live]).values
    s, i, over, w = _call(K, q, kn, kb, k)
    assert torch.equal(i, i32) and torch.equal(s, s32) and over == 1 and w[15] == 2, (over, w[14:24])
    assert torch.equal(i[3], i32[3]) and torch.equal(s[599], s32[599]) and bool((s[3] == 0).all())
    for t in (float(srt[0]) - 0.005, float(srt[60]), float(srt[300])):
        s, i, over, w = _call(K, q, kn, kb, k, float(srt[0]) - 0.01, t)
        assert torch.equal(i, i32) and torch.equal(s, s32), t
        assert w[21] == 1 and over == 1 and w[17] == 0, (t, w[14:24], over)
        assert w[22] == int((kth[live] < t).sum()), (t, w[14:24])


def test_a_captured_call_replays_exactly(dev):
    """One call captured into a HIP graph on one stream: no read-back, and each replay answers the queries copied into its
    static input."""
    from ragraph_amd import kernels as K
    from ragraph_amd.capture import CapturedForward

    B, N, D, k = 600, 70_000, 256, 41
    g = torch.Generator(device=dev).manual_seed(4141)
    kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
    kb = K.keys_to_bf16(kn)
    cap = CapturedForward(lambda x: K.topk_cosine_filtered(x, kn, kb, k), torch.randn(B, D, device=dev, generator=g))
    for _ in range(2):
        q = torch.randn(B, D, device=dev, generator=g)
        s, i, over = cap(q)
        s, i, over = s.clone(), i.clone(), int(over)
        s32, i32 = K.topk_cosine(q, kn, k)
        assert torch.equal(i, i32) and torch.equal(s, s32) and over == 0


_CHILD = """
import sys, torch
sys.path.insert(0, sys.argv[1])
from ragraph_amd import kernels as K
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(515)
kn = K.normalize_rows(torch.randn(70_000, 256, device=dev, generator=g))
q = torch.randn(600, 256, device=dev, generator=g)
index = K.KeyIndex(kn, dedup=False)
s, i = index.topk(q, 41)
s32, i32 = K.topk_cosine(q, kn, 41)
assert torch.equal(i, i32) and torch.equal(s, s32)
assert index.last_stats is None and index._bf16 is None, "a filtered call ran"
print("child ok")
"""


def test_key_index_and_the_bank_take_the_wide_call(dev):
    from ragraph_amd import kernels as K
    from ragraph_amd.ragraph_utils import ToyGraphBase

    N, D, k, B = 70_000, 256, 41, 600
    g = torch.Generator(device=dev).manual_seed(515)
    kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
    q = torch.randn(B, D, device=dev, generator=g)
    s32, i32 = K.topk_cosine(q, kn, k)
    assert K.filter_wide_helps(B, N, D, k)
    index = K.KeyIndex(kn, dedup=False)
    s, i = index.topk(q, k)
    w = index.last_stats.cpu().tolist()
    assert w[0] == K.FILTER_STATS_MAGIC and w[14] == B and w[20] == 0, w[:24]      # a filtered call ran
    assert torch.equal(i, i32) and torch.equal(s, s32)
    base = ToyGraphBase(None, 2, D, 3, device=dev, flavour="node")
    base.add_resources(kn, torch.zeros(N, D, device=dev), torch.zeros(N, 2, device=dev))
    sb, ib = base.topk(q, k)[:2]
    sr, ir = K.topk_cosine(q, base.keys_normalized, k)           # (the bank normalises what it is given)
    assert torch.equal(ib, ir) and torch.equal(sb, sr)
    assert base._index.last_stats is not None and int(base._index.last_stats[0]) == K.FILTER_STATS_MAGIC
    # RAGRAPH_EXACT_FP32=1 (read when the rule is asked): the same bits with no filtered call, in a process of its own
    env = dict(os.environ, RAGRAPH_EXACT_FP32="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stdout + out.stderr
