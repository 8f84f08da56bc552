"""The TIGHT speculative bound of the filtered top-k (ragraph_topk_cosine_filtered_set_tight_prior): a call under a prior p
that also starts every query from t > p runs ONE level, proves the queries whose k-th best found reaches t and repairs the
others on the device from max(p, what they found) -- up to 256 of them by a compact call of the direct kernel, more by one
more level for everybody -- so the result has the bits of the fp32 kernel for ANY t.  Forced bounds through the C ABI against
K.topk_cosine, the statistics words [21] (tight in force), [22] (soft misses), [23] (the repair that ran), and the product
dispatch (KeyIndex) that derives t from its calls' statistics."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# the smallest shapes that reach each kernel form: int8 ring with one ragged tile; int8 from 2048 queries (the schedule's scored
# lists); a bf16 level; the D = 64 eight-group form
SHAPES = [(300, 70_000, 256, 10), (2100, 40_000, 256, 10), (700, 20_000, 128, 5), (1100, 70_000, 64, 8)]
_REF = {}


def _case(dev, B, N, D, k):
    """Bank, queries and the fp32 reference of a shape, computed once and shared (read-only) by the tests."""
    from ragraph_amd import kernels as K

    key = (B, N, D, k)
    if key not in _REF:
        g = torch.Generator(device=dev).manual_seed(1000 + B + D)
        kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
        q = torch.randn(B, D, device=dev, generator=g)
        s32, i32 = K.topk_cosine(q, kn, k)
        _REF[key] = (kn, K.keys_to_bf16(kn), q, s32, i32)
    return _REF[key]


def _call(K, q, kn, kb, k, prior, tight):
    K.set_filter_prior(prior)
    old = K.set_filter_tight_prior(tight)
    assert old != old                                    # (NaN: no tight bound was set on this thread)
    try:
        s, i, over, st = K.topk_cosine_filtered(q, kn, kb, k, return_stats=True)
        w = st.cpu().tolist()
    finally:
        K.set_filter_prior(None)
        K.set_filter_tight_prior(None)
    return s, i, int(over), w


@pytest.mark.parametrize("B,N,D,k", SHAPES)
def test_forced_tight_bounds_are_exact(dev, B, N, D, k):
    from ragraph_amd import kernels as K

    kn, kb, q, s32, i32 = _case(dev, B, N, D, k)
    kth = s32[:, k - 1]
    srt = torch.sort(kth).values
    lo, hi = float(srt[0]), float(srt[-1])
    safe = lo - 0.01
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    cases = [("below every k-th best", safe, f32(lo - 0.005)),
             ("between the lowest and the second lowest", safe, float((srt[0] + srt[1]) * 0.5)),
             ("a quantile: about 100 soft misses", safe, float(srt[100])),
             ("the median", safe, float(srt[B // 2])),
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
    for what, p, t in (("t at most p", safe, safe - 0.01), ("t = p", safe, safe), ("NaN", safe, None)):
        s, i, over, w = _call(K, q, kn, kb, k, p, t)
        assert torch.equal(i, i32) and torch.equal(s, s32), what
        assert w[16] == 1 and w[21] == 0 and w[22] == 0 and w[23] == 0 and w[17] == 0, (what, w[14:24])
    s, i, over, w = _call(K, q, kn, kb, k, None, float(srt[B // 2]))     # no prior: the bound pass, t ignored
    assert torch.equal(i, i32) and torch.equal(s, s32) and w[16] == 0 and w[21] == 0


def test_a_shape_below_the_workspace_rule_ignores_the_tight_bound(dev):
    """260 queries: the idle candidate lists and gmax cannot hold the 256-query repair's buffers (filter_call_plan)."""
    from ragraph_amd import kernels as K

    kn, kb, q, s32, i32 = _case(dev, 260, 70_000, 256, 10)
    kth = s32[:, 9]
    s, i, over, w = _call(K, q, kn, kb, 10, float(kth.min()) - 0.01, float(kth.median()))
    assert torch.equal(i, i32) and torch.equal(s, s32)
    assert w[16] == 1 and w[21] == 0 and w[22] == 0 and w[17] == 0 and over == 0


def test_tight_bound_with_zero_queries_and_an_overflowing_cluster(dev):
    """Zero queries (flag 2: answered without work, never judged) and a query next to 3000 near-duplicate keys whose list
    overflows (flag 1: the exact scan) under a tight bound, with the 256-query repair and with the all-queries level."""
    from ragraph_amd import kernels as K

    g = torch.Generator(device=dev).manual_seed(77)
    kn = K.normalize_rows(torch.randn(70_000, 256, device=dev, generator=g))
    kn[5000:8000] = K.normalize_rows(kn[7] + 0.0005 * torch.randn(3000, 256, device=dev, generator=g))
    q = torch.randn(600, 256, device=dev, generator=g)
    q[3] = 0.0
    q[599] = 0.0
    q[100] = kn[7] + 0.001 * torch.randn(256, device=dev, generator=g)
    kb = K.keys_to_bf16(kn)
    s32, i32 = K.topk_cosine(q, kn, 10)
    kth = s32[:, 9]
    live = torch.ones(600, dtype=torch.bool, device=dev)
    live[[3, 100, 599]] = False
    srt = torch.sort(kth[live]).values
    for t in (float(srt[0]) - 0.005, float(srt[60]), float(srt[300])):
        s, i, over, w = _call(K, q, kn, kb, 10, float(srt[0]) - 0.01, t)
        assert torch.equal(i, i32) and torch.equal(s, s32), t
        assert w[21] == 1 and over == 1 and w[17] == 0, (t, w[14:24], over)
        assert w[22] == int((kth[live] < t).sum()), (t, w[14:24])


def test_a_capture_after_warm_up_sets_no_tight_bound(dev):
    """A warm index (prior and tight bound in force for eager calls) captures calls with their bound pass and neither bound."""
    from ragraph_amd import kernels as K
    from ragraph_amd.capture import CapturedForward

    N, D, k, B = 100_000, 256, 10, 2048
    g = torch.Generator(device=dev).manual_seed(4243)
    kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
    index = K.KeyIndex(kn, dedup=False)
    batch = lambda: torch.randn(B, D, device=dev, generator=g)
    for _ in range(5):
        index.topk(batch(), k)
        torch.cuda.synchronize()
    assert index.last_prior is not None and index.last_tight is not None
    stats = torch.zeros(32, dtype=torch.int32, device=dev)

    def fwd(q):
        s, i = index.topk(q, k)
        stats.copy_(index.last_stats[:32])
        return i

    cap = CapturedForward(fwd, batch())
    assert index.last_prior is None and index.last_tight is None
    q = batch()
    i_rep = cap(q).clone()
    torch.cuda.synchronize()
    w = stats.cpu().tolist()
    assert torch.equal(i_rep, K.topk_cosine(q, kn, k)[1])
    assert w[0] == K.FILTER_STATS_MAGIC and w[16] == 0 and w[21] == 0 and w[20] == 0, w[14:24]


def test_key_index_derives_the_tight_bound_and_repairs_a_drifted_batch(dev):
    from ragraph_amd import kernels as K

    N, D, k, B = 200_000, 256, 10, 2048
    g = torch.Generator(device=dev).manual_seed(99)
    kn = torch.randn(N, D, device=dev, generator=g)
    kn[:, 128:] = 0.0                                     # the bank spans half of the space, and so do the queries it knows
    kn = K.normalize_rows(kn)
    index = K.KeyIndex(kn, dedup=False)

    def batch():
        q = torch.randn(B, D, device=dev, generator=g)
        q[:, 128:] = 0.0
        return q

    for c in range(5):
        q = batch()
        s, i = index.topk(q, k)
        torch.cuda.synchronize()
        s32, i32 = K.topk_cosine(q, kn, k)
        assert torch.equal(i, i32) and torch.equal(s, s32)
    assert index.last_prior is not None and index.last_tight is not None and index.last_tight > index.last_prior
    w = index.last_stats.cpu().tolist()
    assert w[16] == 1 and w[21] == 1 and w[1] == 1 and w[17] == 0, w[14:24]
    # a drifted batch: a tenth of the mass of 24 queries lies outside the bank's span -- their scores shrink by 5 %, which
    # takes the lower ones below the tight bound and none below the prior (lowest seen - half the spread)
    q = batch()
    q[:24, 128:] = 0.33 * torch.randn(24, 128, device=dev, generator=g)
    s32, i32 = K.topk_cosine(q, kn, k)
    s, i = index.topk(q, k)
    torch.cuda.synchronize()
    assert index.last_tight is not None
    t, p = index.last_tight, index.last_prior
    w = index.last_stats.cpu().tolist()
    assert torch.equal(i, i32) and torch.equal(s, s32)
    kth = s32[:, k - 1]
    assert w[21] == 1 and w[22] == int((kth < t).sum()) and w[22] >= 1 and w[17] == int((kth < p).sum()), (w[14:24], t, p)
    index.topk(batch()[:300].contiguous(), k)            # (polls the drifted call's words)
    torch.cuda.synchronize()
    assert index._spec[k].get("soft", 0) >= w[22]
