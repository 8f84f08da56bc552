"""Edge evaluation (RAGraph_edge/utils/metrics.py Metric) without a GPU: golden g17 -- produced by the reference's own
Metric.eval / eval_grouped (tools/make_golden_metric.py) -- against the C oracle's ranking and a numpy restatement of the
metrics, and edge_eval.Metric's host planning."""
import os

import numpy as np
import pytest

from oracle import pipeline

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUPS = ("eval", "tuned", "untuned")


def gold():
    return dict(np.load(os.path.join(GOLD, "g17_metric_eval.npz")))


def rows(rowptr, items):
    return [items[rowptr[u]:rowptr[u + 1]].tolist() for u in range(len(rowptr) - 1)]


def ref_metrics(ranked, gt, ks, batch):
    """metrics.py:12-46, 60-80, 131-133 restated: per batch of `batch` users, result += batch_result / n_users."""
    n = len(gt)
    out = {m: np.zeros(len(ks)) for m in ("recall", "ndcg", "precision")}
    for s in range(0, n, batch):
        rk, g = ranked[s:s + batch], gt[s:s + batch]
        r = np.array([[float(x in gg) for x in row] for row, gg in zip(rk, g)])
        rn = np.array([len(gg) for gg in g])
        for t, k in enumerate(ks):
            right = r[:, :k].sum(1)
            tm = np.zeros((len(r), k))
            for i, gg in enumerate(g):
                tm[i, :min(k, len(gg))] = 1
            idcg = np.sum(tm * 1. / np.log2(np.arange(2, k + 2)), axis=1)
            dcg = np.sum(r[:, :k] * (1. / np.log2(np.arange(2, k + 2))), axis=1)
            idcg[idcg == 0.] = 1.
            out["recall"][t] += np.sum(right / rn) / n
            out["ndcg"][t] += np.sum(dcg / idcg) / n
            out["precision"][t] += np.sum(right) / k / n
    return out


class Loader:
    """The three dicts the reference's Metric reads (EdgeListData carries the same)."""

    def __init__(self, g):
        users = g["eval_users"].tolist()
        hist = rows(g["eval_hist_rowptr"], g["eval_hist_items"])
        gt = rows(g["eval_gt_rowptr"], g["eval_gt_items"])
        self.test_user_dict = {u: gt[i] for i, u in enumerate(users)}
        self.user_hist_dict = {u: hist[i] for i, u in enumerate(users)}
        self.train_user_dict = {int(u): self.user_hist_dict.get(int(u), []) for u in g["train_users"]}


def test_g17_oracle_ranking_and_numpy_metrics_match_reference():
    g = gold()
    ks = g["ks"].tolist()
    for name in GROUPS:
        users = g[f"{name}_users"]
        hist = rows(g[f"{name}_hist_rowptr"], g[f"{name}_hist_items"])
        ranked = pipeline.edge_topk_items(g["user_emb"], g["item_emb"], users, hist, int(max(ks)))
        assert np.array_equal(ranked, g[f"{name}_ranked"]), name
        gt = rows(g[f"{name}_gt_rowptr"], g[f"{name}_gt_items"])
        res = ref_metrics(ranked, gt, ks, int(g["eval_batch_size"]))
        for m, v in res.items():
            assert np.allclose(v, g[f"{name}_{m}_raw"], rtol=0, atol=1e-12), (name, m)
            assert np.array_equal(np.round(v, 6), g[f"{name}_{m}"]), (name, m)
    # the fixture covers what it claims to
    assert (np.diff(g["eval_hist_rowptr"]) == 0).any() and g["untuned_users"].size > 0
    assert any(len(h) != len(set(h)) for h in rows(g["eval_hist_rowptr"], g["eval_hist_items"]))
    assert any(len(t) != len(set(t)) for t in rows(g["eval_gt_rowptr"], g["eval_gt_items"]))


def test_metric_host_planning():
    from ragraph_amd.edge_eval import Metric

    g = gold()
    dl = Loader(g)
    m = Metric("recall;ndcg;precision", "10;20;50", int(g["eval_batch_size"]))
    assert m.metrics == ["recall", "ndcg", "precision"] and m.k == [10, 20, 50]
    for name, group in (("eval", None), ("tuned", "tuned"), ("untuned", "untuned")):
        p = m.plan(dl, group)
        assert np.array_equal(p.users, g[f"{name}_users"]), name          # the reference's user order
        for a in ("hist_rowptr", "hist_items", "gt_rowptr", "gt_items"):   # raw CSRs: duplicates and order kept
            assert np.array_equal(getattr(p, a), g[f"{name}_{a}"]), (name, a)
        assert m.plan(dl, group) is p                                      # built once per dataloader
    tuned, untuned = set(g["tuned_users"].tolist()), set(g["untuned_users"].tolist())
    assert not tuned & untuned and tuned | untuned == set(g["eval_users"].tolist())
    assert tuned <= set(g["train_users"].tolist()) and not untuned & set(g["train_users"].tolist())


def test_metric_arguments():
    from ragraph_amd.edge_eval import Metric
    from ragraph_amd._native import RagraphNativeError

    m = Metric()
    assert m.metrics == ["recall", "ndcg"] and m.k == [20] and m.eval_batch_size == 512
    assert Metric(metrics_k="5;64").k == [5, 64]
    with pytest.raises(NotImplementedError, match="mrr"):
        Metric(metrics="recall;mrr")
    with pytest.raises(ValueError, match="hit_ratio"):
        Metric(metrics="hit_ratio")
    with pytest.raises(RagraphNativeError, match="64"):
        Metric(metrics_k="20;65")


def test_topk_dot_masked_workspace_is_slab_free_on_fused_shapes():
    from ragraph_amd import _native as N

    L = N.lib()
    ws = L.ragraph_topk_dot_masked_workspace_bytes(20000, 107028, 64, 20, 200000)
    assert 0 < ws < 64 << 20                                     # a [B, N] slab alone would be 8.6 GB
    assert L.ragraph_topk_dot_masked_workspace_bytes(33, 2000, 48, 20, 10) >= 33 * 2000 * 4   # slab path: width 48
    assert L.ragraph_topk_dot_masked_workspace_bytes(10, 10, 0, 3, 0) == 0
    assert L.ragraph_rank_metrics_workspace_bytes(257, 3, 128) >= 257 * 9 * 8
    assert L.ragraph_rank_metrics_workspace_bytes(257, 17, 128) == 0
