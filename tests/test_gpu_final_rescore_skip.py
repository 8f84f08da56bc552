"""The FINAL rescoring launch of a call under a tight bound returns, for an unflagged query with an empty list and no index base,
before it reads the query row (csrc/filter_rescore.h: SKIP; run_tight_repair): such a query's merge would rewrite the row it read.
Forced bounds through the C ABI: indices and score bits against the fp32 kernel, the overflow count and every statistics word
against the launch that skips nothing (RAGRAPH_FILTER_FINAL_SKIP=0, the path before the change), with no soft miss, with 1 .. 256
(the compact repair), with more (the all-queries level fills the lists the final launch merges), with an index base (never
skipped) -- over banks that hold one zero query and one query next to an overflowing near-duplicate cluster.  600 queries take the
workgroup-per-query kernel, 2100 the wave-per-query one."""
import numpy as np
import pytest
import torch

import test_gpu_tight_tail_counts as T

pytestmark = pytest.mark.gpu

K_ = T.K_
_BIG = {}


def _call(K, monkeypatch, skip, q, kn, kb, prior, tight, idx_base):
    monkeypatch.setenv("RAGRAPH_FILTER_FINAL_SKIP", "1" if skip else "0")
    K.set_filter_prior(prior)
    K.set_filter_tight_prior(tight)
    try:
        s, i, over, st = K.topk_cosine_filtered(q, kn, kb, K_, idx_base=idx_base, return_stats=True)
        w = st.cpu().tolist()
    finally:
        K.set_filter_prior(None)
        K.set_filter_tight_prior(None)
    return s.cpu(), i.cpu(), int(over), w


def _check(K, monkeypatch, q, kn, kb, s32, i32, kth_live, cases, n_flagged, kth_cluster=None):
    """kth_cluster: the final k-th best of the cluster query.  Under a t ABOVE it the cluster may stay below the level's threshold:
    the query is then a soft miss like any other (and overflows in the repair) instead of being flagged by the level -- which of the
    two depends on the level's eps, and both are right, so word [22] may count it."""
    for what, p, t, base, repair in cases:
        soft = int((kth_live < np.float32(t)).sum())
        maybe = 1 if kth_cluster is not None and kth_cluster < np.float32(t) else 0
        assert (soft == 0, 1 <= soft <= 256, soft > 256) == (repair == 0, repair == 1, repair == 2), (what, soft)
        got = [_call(K, monkeypatch, skip, q, kn, kb, p, t, base) for skip in (True, False)]
        print(what, "soft", soft, "words[14:29]", got[0][3][14:29], "over", got[0][2])
        for s, i, over, w in got:
            assert torch.equal(i, i32 + base) and torch.equal(s, s32), what
            assert w[21] == 1 and w[22] in (soft, soft + maybe) and w[23] == repair and w[17] == 0 and over == n_flagged, (what, w[14:29], over)
        assert got[0][2] == got[1][2] and got[0][3] == got[1][3], (what, got[0][3], got[1][3])


@pytest.mark.parametrize("D", [256, 64])
def test_skipping_changes_nothing(dev, monkeypatch, D):
    from ragraph_amd import kernels as K

    kn, kb, q, s32, i32, live, cq = T._case(dev, D)
    kth_live = s32[live, K_ - 1].numpy()
    srt = np.sort(kth_live)
    _, p, t_some = T.bounds(s32, live, cq)[0]
    f32 = lambda x: float(np.float32(x))
    cases = [("no soft miss", p, f32(srt[0] - 0.005), 0, 0),
             ("1 .. 256 soft misses", p, t_some, 0, 1),
             ("more than 256 soft misses", p, f32(0.5 * (srt[300] + srt[301])), 0, 2),
             ("an index base: no row is skipped", p, t_some, 7, 1),
             ("an index base, no soft miss", p, f32(srt[0] - 0.005), 7, 0)]
    # (n_flagged: the cluster query; zero queries are not counted)
    _check(K, monkeypatch, q, kn, kb, s32, i32, kth_live, cases, n_flagged=1, kth_cluster=s32[cq, K_ - 1].numpy())


def test_skipping_changes_nothing_in_the_wave_per_query_kernels(dev, monkeypatch):
    """2100 queries: the final launch is the one-wave-per-query kernel (scored lists on the int8 level of this shape)."""
    from ragraph_amd import kernels as K

    if not _BIG:
        g = torch.Generator().manual_seed(977)
        kn = K.normalize_rows(torch.randn(40_000, 256, generator=g).to(dev))
        q = torch.randn(2100, 256, generator=g)
        q[11] = 0.0
        q = q.to(dev)
        s32, i32 = K.topk_cosine(q, kn, K_)
        _BIG["case"] = (kn, K.keys_to_bf16(kn), q, s32.cpu(), i32.cpu())
    kn, kb, q, s32, i32 = _BIG["case"]
    live = torch.ones(2100, dtype=torch.bool)
    live[11] = False
    kth_live = s32[live, K_ - 1].numpy()
    srt = np.sort(kth_live)
    f32 = lambda x: float(np.float32(x))
    p = f32(srt[0] - 0.02)
    cases = [("no soft miss", p, f32(srt[0] - 0.005), 0, 0),
             ("1 .. 256 soft misses", p, f32(0.5 * (srt[40] + srt[41])), 0, 1),
             ("more than 256 soft misses", p, f32(0.5 * (srt[700] + srt[701])), 0, 2),
             ("an index base: no row is skipped", p, f32(0.5 * (srt[40] + srt[41])), 7, 1)]
    _check(K, monkeypatch, q, kn, kb, s32, i32, kth_live, cases, n_flagged=0)
