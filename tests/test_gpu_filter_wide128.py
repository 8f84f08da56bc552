"""The filtered exact top-k for lists of 65 .. 128 keys (ragraph_topk_cosine_filtered_f32 at its list width of 128, behind
kernels.topk_cosine_filtered): every result is held, bit for bit, to K.topk_cosine on the same tensors -- the ordered large-k
path over fp32 score slabs, which existing tests hold to the oracle.  No tolerance anywhere."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# the smallest shapes that reach each kernel form (those of the test for lists of 33 .. 64 keys)
RING = [(300, 70_000, 256),    # ring kernel, one ragged tile; the workgroup-per-query rescoring
        (2100, 40_000, 256),   # from 2048 queries: the one-wave-per-query rescoring
        (700, 20_000, 128),    # a bf16 level
        (1100, 70_000, 64)]    # the eight-group D = 64 form
DIRECT = [(9, 70_000, 256),    # direct kernel, sliced lists for <= 64 queries
          (100, 70_000, 128),
          (256, 70_000, 256)]
KS = (65, 96, 128)
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
    print("candidates per query and level:", K.filter_stats_levels(w), "overflow", over)
    assert w[0] == K.FILTER_STATS_MAGIC and w[14] == B and w[16] == 0, w[:24]
    assert torch.equal(i, i32) and torch.equal(s, s32)
    assert over == 0 and w[20] == 0, (over, w[:24])


def test_the_scored_switch_changes_nothing(dev, monkeypatch):
    """The plan refuses scored lists beyond k = 64 (tests/test_cpu_filter_wide.py): with RAGRAPH_FILTER_SCORED=1 the call of
    the shape whose int8 levels would keep them runs on plain lists and is as exact."""
    from ragraph_amd import kernels as K

    B, N, D = RING[1]
    kn, kb, q, s32, i32 = _case(dev, B, N, D, 96)
    monkeypatch.setenv("RAGRAPH_FILTER_SCORED", "1")
    s, i, over, w = _call(K, q, kn, kb, 96)
    assert torch.equal(i, i32) and torch.equal(s, s32) and over == 0


@pytest.mark.parametrize("B,N,D", RING)
def test_forced_priors_are_exact(dev, B, N, D):
    from ragraph_amd import kernels as K

    k = 96
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

    k = 128
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

    k = 128
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
    assert bool((s[0] == s[0, 0]).all()) and bool((s[B - 1] == s[B - 1, 0]).all())
    ties = s[:, 1:] == s[:, :-1]                                            # canonical order in every row
    assert bool((s[:, 1:] <= s[:, :-1]).all()) and bool((i[:, 1:][ties] > i[:, :-1][ties]).all())


def test_zero_queries_and_an_overflowing_cluster(dev):
    """Zero queries (answered without work, never counted) and a query next to 3000 near-duplicate keys, whose list overflows
    (the exact scan, in its form for 128 winners): without a bound, and under tight bounds with either repair.
    Every other query is made orthogonal to the cluster's centre.  A level's threshold for a list of 96 of 70 000 keys lies
    where a Gaussian query scores above it against a given key with probability ~1 %: of 600 untouched Gaussian queries five
    were within their bound of all 3000 copies and overflowed too (measured: 6 overflowed lists, every row exact), which is
    the filter's contract and not this test's subject -- one query next to the cluster, and one overflow."""
    from ragraph_amd import kernels as K

    k = 96
    g = torch.Generator(device=dev).manual_seed(77)
    kn = K.normalize_rows(torch.randn(70_000, 256, device=dev, generator=g))
    kn[5000:8000] = K.normalize_rows(kn[7] + 0.0005 * torch.randn(3000, 256, device=dev, generator=g))
    q = torch.randn(600, 256, device=dev, generator=g)
    q -= (q @ kn[7])[:, None] * kn[7][None, :]       # (orthogonal to the cluster's centre: nowhere near their k-th best)
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
    print("overflowed lists:", over, "zero queries:", w[15])
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

    B, N, D, k = 600, 70_000, 256, 96
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


def test_key_index_and_the_bank_take_the_wide128_call(dev, monkeypatch):
    from ragraph_amd import kernels as K
    from ragraph_amd.ragraph_utils import ToyGraphBase

    monkeypatch.delenv("RAGRAPH_EXACT_FP32", raising=False)
    N, D, k, B, C = 70_000, 256, 100, 600, 40
    g = torch.Generator(device=dev).manual_seed(515)
    kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
    q = torch.randn(B, D, device=dev, generator=g)
    s32, i32 = K.topk_cosine(q, kn, k)
    assert K.filter_wide128_helps(B, N, D, k) and K.filter_wide128_helps(B, N, D, 2 * (C + 1))
    index = K.KeyIndex(kn, dedup=False)
    s, i = index.topk(q, k)
    w = index.last_stats.cpu().tolist()
    assert w[0] == K.FILTER_STATS_MAGIC and w[14] == B and w[20] == 0, w[:24]      # a filtered call ran
    assert torch.equal(i, i32) and torch.equal(s, s32)
    # noisy fine-tuning over 40 classes retrieves 2 (40 + 1) = 82 keys: the same rows with the rule on and under RAGRAPH_EXACT_FP32=1
    vals = torch.randn(N, D, device=dev, generator=g)
    labs = torch.nn.functional.one_hot(torch.randint(0, C, (N,), device=dev, generator=g), C).float()

    def noisy():
        base = ToyGraphBase(None, C, D, 3, device=dev, flavour="node")
        base.noise_rng = "device"
        base.add_resources(kn, vals, labs)
        torch.manual_seed(99)
        emb, lab = base.retrieve(q, None, add_noise=True)
        return emb, lab, base._index.last_stats

    emb, lab, stats = noisy()
    assert emb.shape == (B, 2 * (C + 1) + 1, D) and stats is not None and int(stats[0]) == K.FILTER_STATS_MAGIC
    monkeypatch.setenv("RAGRAPH_EXACT_FP32", "1")
    emb32, lab32, stats32 = noisy()
    assert stats32 is None                                                         # no filtered call ran
    assert torch.equal(emb, emb32) and torch.equal(lab, lab32)
