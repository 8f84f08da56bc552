#!/usr/bin/env python3
"""Generate tests/golden/g17_metric_eval.npz by running the REFERENCE's own evaluation (RAGraph_edge/utils/metrics.py
Metric.eval and Metric.eval_grouped, CPU) on fixed embeddings -- the pinned fixture of edge_eval.Metric.

Uses oracle/make_golden.py's import context unchanged.  The model and dataloader are stand-ins: generate() returns fixed
embeddings, rating() is u @ i.T (RAGraph_edge/modules/RAGraph.py:362-364), the dataloader carries the three dicts
Metric reads.  A Metric subclass records every eval_batch input (the ranked lists) and output (the unrounded per-batch
sums) before the reference rounds them.

Data conditions (asserted): users with empty histories, duplicates in histories and ground truths, test users without
training interactions (so 'untuned' is non-empty), ground truth drawn partly from each user's unmasked top 50; every
test user keeps >= 50 unmasked items, and the masked ratings are tie-free through place 51 (torch.topk's tie order
never enters the fixture).

Usage:  python tools/make_golden_metric.py   (writes tests/golden/g17_metric_eval.npz)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.make_golden import _install_shims, min_topk_gap, ref_project, save  # noqa: E402

U, I, D, N_TEST, KMAX, BATCH = 300, 2000, 64, 257, 50, 128
METRICS, KS = "recall;ndcg;precision", "10;20;50"


def _csr(lists):
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    items = np.array([i for x in lists for i in x], dtype=np.int64)
    return rowptr, items


def main():
    _install_shims()
    rng = np.random.default_rng(17)
    g = torch.Generator().manual_seed(1717)
    ue = torch.randn(U, D, generator=g)
    ie = torch.randn(I, D, generator=g)
    rating = ue @ ie.t()

    # training interactions: users 0..219 have some (a few with duplicates), 220..299 none (test-only: 'untuned')
    train = {}
    for u in range(220):
        n = int(rng.integers(1, 25))
        items = rng.choice(I, size=n, replace=False).tolist()
        if u % 7 == 0:
            items += items[: 1 + n // 3]          # duplicates in a history (the mask is a set anyway)
        train[u] = items
    hist = {u: train.get(u, []) for u in range(U)}
    # test users in a shuffled dict order, tuned and untuned mixed; each ground truth partly from the unmasked top 50
    test_users = rng.permutation(U)[:N_TEST].tolist()
    # a test user whose masked top 51 holds a near-tie draws its embedding again (fp32 summation-order noise at these
    # magnitudes is ~1e-6; the gap asked for is 1e-4)
    for u in test_users:
        while True:
            masked = ue[u] @ ie.t()
            masked[hist[u]] = -1e8
            if min_topk_gap(masked[None], KMAX) >= 1e-4:
                break
            ue[u] = torch.randn(D, generator=g)
    rating = ue @ ie.t()
    test = {}
    for u in test_users:
        masked = rating[u].clone()
        masked[hist[u]] = -1e8
        top = torch.topk(masked, KMAX).indices.numpy()
        picks = rng.choice(top, size=int(rng.integers(0, 6)), replace=False).tolist()
        rest = rng.choice(I, size=int(rng.integers(1, 8)), replace=False).tolist()
        gt = picks + rest
        if u % 5 == 0:
            gt = gt + gt[:2]                      # duplicates in a ground truth (raw length counts them)
        test[int(u)] = [int(x) for x in gt]

    masked = rating.clone()
    for u in range(U):
        masked[u, hist[u]] = -1e8
    sel = masked[test_users]
    assert all(I - len(set(hist[u])) >= KMAX for u in test_users)
    gap = min_topk_gap(sel, KMAX)
    print(f"  masked ratings: min top-{KMAX + 1} gap {gap:.3e}")
    assert gap >= 1e-4, gap
    assert any(len(hist[u]) == 0 for u in test_users) and any(u not in train for u in test_users)

    class Model:
        def generate(self):
            return ue.clone(), ie.clone()

        def rating(self, u, i):
            return u @ i.t()

    class Loader:
        test_user_dict = test
        train_user_dict = train
        user_hist_dict = hist

    argv = ["x", "--device", "cpu", "--metrics", METRICS, "--metrics_k", KS, "--eval_batch_size", str(BATCH)]
    out = {}
    with ref_project("RAGraph_edge", argv=argv):
        from utils.metrics import Metric

        class Recording(Metric):
            def __init__(self):
                super().__init__()
                self.ranked, self.batches = [], []

            def eval_batch(self, data, topks):
                self.ranked.append(data[0].numpy().copy())
                r = super().eval_batch(data, topks)
                self.batches.append({m: np.array(v, dtype=np.float64) for m, v in r.items()})
                return r

        for name, group in (("eval", None), ("tuned", "tuned"), ("untuned", "untuned")):
            m = Recording()
            res = m.eval(Model(), Loader()) if group is None else m.eval_grouped(Model(), Loader(), group=group)
            ranked = np.concatenate([r.reshape(-1, KMAX) for r in m.ranked], 0).astype(np.int64)
            n = ranked.shape[0]
            raw = {mm: np.zeros(3) for mm in METRICS.split(";")}
            for b in m.batches:                   # metrics.py:131-133 / 196-198, unrounded
                for mm in raw:
                    raw[mm] += b[mm] / n
            if group is None:
                users = list(test.keys())
            elif group == "tuned":
                users = list(set(train.keys()).intersection(set(test.keys())))
            else:
                users = list(set(test.keys()).difference(set(train.keys())))
            assert len(users) == n
            hrp, hit = _csr([hist[u] for u in users])
            grp, git = _csr([test[u] for u in users])
            out[f"{name}_users"] = np.array(users, dtype=np.int64)
            out[f"{name}_hist_rowptr"], out[f"{name}_hist_items"] = hrp, hit
            out[f"{name}_gt_rowptr"], out[f"{name}_gt_items"] = grp, git
            out[f"{name}_ranked"] = ranked
            for mm in raw:
                out[f"{name}_{mm}"] = np.asarray(res[mm], dtype=np.float64)
                out[f"{name}_{mm}_raw"] = raw[mm]
            print(f"  {name}: {n} users, " + ", ".join(f"{mm} {np.asarray(res[mm])}" for mm in raw))
    assert out["untuned_users"].size > 0 and out["tuned_users"].size > 0
    save("g17_metric_eval", user_emb=ue, item_emb=ie, ks=np.array([10, 20, 50], dtype=np.int64),
         train_users=np.array(list(train.keys()), dtype=np.int64),
         eval_batch_size=np.int64(BATCH), **out)


if __name__ == "__main__":
    main()
