"""The low-tail counts of a call under a TIGHT bound t (csrc/filter_verify_fixup.h: filter_verify_prior_kernel): statistics
word [24] = delta = (t - p) / 16 as float bits, words [25..28] = the judged queries (flag 0, proven against the prior p) whose
final k-th best is below t + m delta, m = 1, 2, 4, 8.  Forced bounds through the C ABI at the smallest shapes that take the ring
kernel and honour t, against counts made from the fp32 kernel's k-th best scores with the edges formed in fp32 the same way.
Each bank holds one zero query (flag 2) and one query whose list overflows (flag 1) with a final k-th best INSIDE the edges:
neither may be counted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, K_ = 600, 20_000, 10
ZERO_Q, CLUSTER = 3, slice(5000, 8000)
SEED = {256: 4356, 64: 4164}     # (checked with the oracle on the CPU: no reference k-th best within 1e-6 of an edge)
_CASES = {}


def build_case(D, normalize, topk):
    """Bank, queries and reference of width D from a fixed seed (CPU generator: the same numbers everywhere).  `normalize` and
    `topk(q, kn, k) -> (scores, idx)` are the fp32 kernels (or, for a check without a GPU, the oracle's).
    The cluster query sees 3000 near-duplicate keys at about the 20th lowest k-th best of the plain bank: its list overflows under
    any t below that, and its final k-th best lies a little above such a t.  The other queries are made orthogonal to the
    cluster's direction, so the cluster overflows nobody else's list."""
    g = torch.Generator().manual_seed(SEED[D])
    keys = torch.randn(N, D, generator=g)
    q = torch.randn(B, D, generator=g)
    u = torch.randn(D, generator=g)
    noise = 0.0005 * torch.randn(CLUSTER.stop - CLUSTER.start, D, generator=g)
    q[ZERO_Q] = 0.0
    kn0, q0 = normalize(keys), q
    kth = topk(q, kn0, K_)[0][:, K_ - 1].clone()
    kth[ZERO_Q] = 2.0
    cq = int(torch.argmin(kth))          # the query with the lowest k-th best of the plain bank: the cluster RAISES its k-th best
    live = torch.ones(B, dtype=torch.bool)
    live[[ZERO_Q, cq]] = False
    qn = q[cq] / q[cq].norm()
    u = u - (u @ qn) * qn
    u = u / u.norm()
    kn = kn0
    for _ in range(2):   # (the cluster replaces 3000 keys and lowers every k-th best a little: placed again from the bank that has it)
        a = float(torch.sort(topk(q, kn, K_)[0][live, K_ - 1]).values[20])
        c = a * qn + (1.0 - a * a) ** 0.5 * u
        q = q0.clone()
        q[live] -= (q[live] @ c)[:, None] * c[None, :]
        keys = kn0.clone()
        keys[CLUSTER] = c[None, :] + noise
        kn = normalize(keys)
    s32, i32 = topk(q, kn, K_)
    assert float(s32[cq, K_ - 1]) > a - 0.002 and bool(((i32[cq] >= CLUSTER.start) & (i32[cq] < CLUSTER.stop)).any())   # (cluster rows among its winners)
    return kn, q, s32, i32, live, cq


def bounds(s32, live, cq):
    """(what, prior, t) of the forced calls, as fp32 values: t sits 0.004 below the cluster query's final k-th best."""
    f32 = lambda x: float(np.float32(x))
    kth = s32[:, K_ - 1]
    srt = torch.sort(kth[live]).values
    t = f32(float(kth[cq]) - 0.004)
    return [("soft misses only", f32(min(float(srt[0]), t) - 0.02), t),
            ("three hard misses: failed queries are not counted", f32(0.5 * (float(srt[2]) + float(srt[3]))), t)]


def expected_words(s32, live, p, t):
    """([24], [25..28], [22], [17]) from the reference k-th best scores; asserts that no judged score is within 1e-6 of an edge."""
    kth = s32[:, K_ - 1].numpy().astype(np.float32)
    p32, t32 = np.float32(p), np.float32(t)
    delta = np.float32((t32 - p32) / np.float32(16.0))
    judged = live.numpy() & (kth >= p32)
    edges = [t32] + [np.float32(t32 + np.float32(m) * delta) for m in (1, 2, 4, 8)]
    for e in edges + [p32]:
        assert np.abs(kth[live.numpy()].astype(np.float64) - float(e)).min() > 1e-6, ("a k-th best too close to an edge", float(e))
    counts = [int((kth[judged] < e).sum()) for e in edges[1:]]
    soft = int((kth[live.numpy()] < t32).sum())              # (word [22] counts every unflagged query the level left below t)
    hard = int((kth[live.numpy()] < p32).sum())
    return int(delta.view(np.int32)), counts, soft, hard, edges


def _case(dev, D):
    from ragraph_amd import kernels as K

    if D not in _CASES:
        on_dev = lambda f: (lambda *a: tuple(o.cpu() for o in f(*[x.to(dev) if torch.is_tensor(x) else x for x in a])))
        kn, q, s32, i32, live, cq = build_case(D, lambda x: K.normalize_rows(x.to(dev)).cpu(), on_dev(K.topk_cosine))
        knd = kn.to(dev)
        _CASES[D] = (knd, K.keys_to_bf16(knd), q.to(dev), s32, i32, live, cq)
    return _CASES[D]


def _call(K, q, kn, kb, prior, tight):
    K.set_filter_prior(prior)
    K.set_filter_tight_prior(tight)
    try:
        s, i, over, st = K.topk_cosine_filtered(q, kn, kb, K_, return_stats=True)
        w = st.cpu().tolist()
    finally:
        K.set_filter_prior(None)
        K.set_filter_tight_prior(None)
    return s.cpu(), i.cpu(), int(over), w


@pytest.mark.parametrize("D", [256, 64])
def test_tail_counts_match_the_reference(dev, D):
    from ragraph_amd import kernels as K

    kn, kb, q, s32, i32, live, cq = _case(dev, D)
    kth = s32[:, K_ - 1]
    for what, p, t in bounds(s32, live, cq):
        delta_bits, counts, soft, hard, edges = expected_words(s32, live, p, t)
        s, i, over, w = _call(K, q, kn, kb, p, t)
        print(D, what, "p", p, "t", t, "words[17:29]", w[17:29], "expected", delta_bits, counts, soft, hard, "over", over)
        assert torch.equal(i, i32) and torch.equal(s, s32), what
        assert w[21] == 1 and w[22] == soft and w[17] == hard and over == hard + 1, (what, w[14:29], over)   # (+ 1: the cluster query)
        assert w[24] == delta_bits and w[25:29] == counts and w[29:32] == [0, 0, 0], (what, w[22:32], delta_bits, counts)
        # the two special queries lie where a kernel that ignored their flags would have counted them
        assert float(kth[ZERO_Q]) == 0.0 and 0.0 < float(edges[1])
        if hard == 0:
            assert float(edges[0]) < float(kth[cq]) < float(edges[4]), (what, float(kth[cq]), edges)
            assert len(set([soft] + counts)) >= 2, (what, soft, counts)            # at least two of the five points differ


@pytest.mark.parametrize("D", [256, 64])
def test_calls_without_a_tight_bound_report_no_tail(dev, D):
    from ragraph_amd import kernels as K

    kn, kb, q, s32, i32, live, cq = _case(dev, D)
    _, p, t = bounds(s32, live, cq)[0]
    for prior, tight in ((p, None), (p, p - 0.01), (None, t)):     # the prior alone; t below p (ignored); no prior at all
        s, i, over, w = _call(K, q, kn, kb, prior, tight)
        assert torch.equal(i, i32) and torch.equal(s, s32)
        assert w[21] == 0 and w[24:32] == [0] * 8, w[20:32]
