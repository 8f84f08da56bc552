"""Top-k recommendation evaluation of RAGraph_edge (RAGraph_edge/utils/metrics.py:83-214): generate() once, then
rating = user_emb @ item_emb.T, history items scored -1e8, top-max(k), recall / ndcg / precision at every k.

The reference builds a [512, I] rating slab per batch of test users, moves it to the CPU for the mask loop and
torch.topk, and computes the metrics in a host loop per user.  Here ONE call ranks all test users on the device
(kernels.topk_dot_masked: the fused kernels score, mask and select without a [B, I] matrix) and one more computes every
metric at every k (kernels.rank_metrics); the host reads back 3 x len(ks) doubles."""
from __future__ import annotations

import time

import numpy as np
import torch

from . import kernels as K
from ._native import TOPK_MAX, RagraphNativeError

MASK_VALUE = -1e8   # metrics.py:214


@torch.no_grad()
def topk_items(model, users: torch.Tensor, hist_rowptr: torch.Tensor, hist_items: torch.Tensor, k: int = 20,
               eval_batch_size: int = 512, embeddings=None):
    """-> idx [len(users), k] item ids ranked by rating.  hist_rowptr/hist_items: CSR over `users` (in that order) of
    the training-history item ids to exclude (metrics.py:210-214).  eval_batch_size is kept for callers; the ranking is
    one call whatever the batch (the result does not depend on it)."""
    user_emb, item_emb = embeddings if embeddings is not None else model.generate()
    return K.topk_dot_masked(user_emb, item_emb, k, hist_rowptr, hist_items, users=users, mask_value=MASK_VALUE)[1]


def recall_ndcg(rank_idx: np.ndarray, ground_truth: list, k: int = 20):
    """metrics.py:12-46 (recall@k, ndcg@k), host side on the [U,k] index matrix."""
    hits = np.zeros(rank_idx.shape, dtype=np.float64)
    for u, items in enumerate(ground_truth):
        hits[u] = np.isin(rank_idx[u], list(items))
    n_rel = np.array([len(g) for g in ground_truth], dtype=np.float64)
    recall = float(np.sum(hits[:, :k].sum(1) / n_rel))
    disc = 1.0 / np.log2(np.arange(2, k + 2))
    ideal = np.array([disc[:min(k, int(n))].sum() for n in n_rel])
    ideal[ideal == 0] = 1.0
    ndcg = float(np.sum((hits[:, :k] * disc).sum(1) / ideal))
    return recall / len(ground_truth), ndcg / len(ground_truth)


def _csr(lists):
    """Raw lists (duplicates and order kept) -> (rowptr int64 [n+1], items int64)."""
    lens = np.fromiter((len(x) for x in lists), dtype=np.int64, count=len(lists))
    rowptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    items = np.fromiter((int(i) for x in lists for i in x), dtype=np.int64, count=int(rowptr[-1]))
    return rowptr, items


class EvalPlan:
    """Host planning of one evaluation (no device work): the test users in the reference's order, their training
    histories (the mask) and ground-truth lists as raw CSRs."""

    def __init__(self, users, hist_rowptr, hist_items, gt_rowptr, gt_items):
        self.users, self.hist_rowptr, self.hist_items = users, hist_rowptr, hist_items
        self.gt_rowptr, self.gt_items = gt_rowptr, gt_items
        self._dev = {}

    def on(self, device):
        """The five arrays as device tensors (copied once per device)."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(device) for a in
                                   (self.users, self.hist_rowptr, self.hist_items, self.gt_rowptr, self.gt_items))
        return self._dev[key]


class Metric:
    """RAGraph_edge/utils/metrics.py:7-10 Metric, with the reference's arguments as constructor parameters
    (--metrics, --metrics_k, --eval_batch_size).  eval / eval_grouped return the reference's dict: metric -> np.ndarray
    over metrics_k rounded to 6 places, plus 'eval_time'.  eval_batch_size only fixes the order the metric sums are added
    in (per batch of that many users, then batch by batch); the device work is one ranking call and one metrics call."""

    def __init__(self, metrics: str = "recall;ndcg", metrics_k: str = "20", eval_batch_size: int = 512):
        self.metrics = metrics.split(";")
        self.k = [int(k) for k in str(metrics_k).split(";")]
        self.eval_batch_size = int(eval_batch_size)
        for m in self.metrics:
            if m == "mrr":
                raise NotImplementedError(
                    "metric 'mrr': the reference's formula (metrics.py:24-29) divides by log2(1/1) = 0 at rank 1 and returns "
                    "inf / nan; it is not reproduced")
            if m not in K.RANK_METRICS:
                raise ValueError(f"unknown metric {m!r} (supported: {', '.join(K.RANK_METRICS)})")
        if not self.k or min(self.k) < 1:
            raise ValueError(f"metrics_k {metrics_k!r}: every k must be >= 1")
        if max(self.k) > TOPK_MAX:
            raise RagraphNativeError(f"metrics_k: max(k) = {max(self.k)} exceeds the ranking kernels' limit of {TOPK_MAX}")
        if self.eval_batch_size < 1:
            raise ValueError("eval_batch_size must be >= 1")
        self._plans = {}
        self.last_ranked = None     # [U, max(k)] item ids of the last evaluation (device tensor)
        self.last_values = None     # its unrounded results: metric -> np.ndarray over k

    # ---- host planning ---------------------------------------------------------------------------------------------
    @staticmethod
    def group_users(dataloader, group=None):
        """The test users in the reference's order: dict order (metrics.py:94) or, for a group, the order of the
        reference's own set expression (metrics.py:150-151)."""
        test = dataloader.test_user_dict
        if group is None:
            return list(test.keys())
        tune = dataloader.train_user_dict
        if group == "tuned":
            return list(set(tune.keys()).intersection(set(test.keys())))
        return list(set(test.keys()).difference(set(tune.keys())))

    def plan(self, dataloader, group=None) -> EvalPlan:
        """The users, history CSR and ground-truth CSR of one evaluation, built once per (dataloader, group)."""
        key = (id(dataloader), group)
        hit = self._plans.get(key)
        if hit is not None and hit[0] is dataloader:
            return hit[1]
        users = self.group_users(dataloader, group)
        hist = dataloader.user_hist_dict
        test = dataloader.test_user_dict
        hrp, hit_ = _csr([hist.get(u, []) for u in users])
        grp, git = _csr([test[u] for u in users])
        p = EvalPlan(np.asarray(users, dtype=np.int64).reshape(-1), hrp, hit_, grp, git)
        self._plans[key] = (dataloader, p)
        return p

    # ---- evaluation ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _run(self, model, dataloader, group):
        t0 = time.time()
        p = self.plan(dataloader, group)
        if p.users.size == 0:
            raise ValueError(f"no test users in group {group!r}")
        user_emb, item_emb = model.generate()                                      # metrics.py:99-100
        users, hrp, hitems, grp, gitems = p.on(user_emb.device)
        _, idx = K.topk_dot_masked(user_emb, item_emb, max(self.k), hrp, hitems, users=users,
                                   mask_value=MASK_VALUE)                          # metrics.py:104-116
        vals = K.rank_metrics(idx, grp, gitems, self.k, self.eval_batch_size)      # metrics.py:126-133
        self.last_ranked = idx
        self.last_values = {m: vals[K.RANK_METRICS.index(m)].copy() for m in self.metrics}
        result = {m: np.round(self.last_values[m], 6) for m in self.metrics}
        result["eval_time"] = np.round(round(time.time() - t0, 2), 6)
        return result

    def eval(self, model, dataloader):
        """metrics.py:83-141."""
        return self._run(model, dataloader, None)

    def eval_grouped(self, model, dataloader, group="tuned"):
        """metrics.py:143-200: group 'tuned' = test users with training interactions, anything else = those without."""
        return self._run(model, dataloader, "tuned" if group == "tuned" else "untuned")
