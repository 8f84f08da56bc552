#!/usr/bin/env python3
"""Edge evaluation at the amazon shape (131 707 users x 107 028 items x D = 64, ~10 history items per user), on one GPU:
  (a) the per-batch slab path (eval_batch_size 512: gather + linear -> scatter_fill -> topk_rows) plus host recall_ndcg;
  (a') its device part alone (the masked slab path);
  (b) one kernels.topk_dot_masked call;
  (c) the whole edge_eval.Metric.eval.
Device-event times after warm-up, A/B alternated; the share of the fp32 MFMA peak is 2 U I D / 157.3 TF.

Usage:  python tools/edge_eval_probe.py [--only b] [--reps 3]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragraph_amd import kernels as K  # noqa: E402
from ragraph_amd import edge_eval  # noqa: E402

U, I, D, PEAK = 131707, 107028, 64, 157.3e12


def ev_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    g = torch.Generator(device=dev).manual_seed(0)
    ue = torch.randn(U, D, generator=g, device=dev)
    ie = torch.randn(I, D, generator=g, device=dev)
    lens = rng.poisson(10, U)
    hist = np.concatenate([rng.integers(0, I, n) for n in lens]).astype(np.int64)
    hrp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    glen = 1 + rng.poisson(4, U)
    gt = np.concatenate([rng.integers(0, I, n) for n in glen]).astype(np.int64)
    grp = np.concatenate([[0], np.cumsum(glen)]).astype(np.int64)
    users = torch.arange(U, device=dev)
    hrp_d, hist_d = torch.from_numpy(hrp).to(dev), torch.from_numpy(hist).to(dev)
    floor_ms = 2.0 * U * I * D / PEAK * 1e3
    print(f"shape {U} x {I} x {D}, history nnz {hist.size}, compute floor {floor_ms:.2f} ms")

    class DL:
        test_user_dict = {u: gt[grp[u]:grp[u + 1]].tolist() for u in range(U)}
        user_hist_dict = {u: hist[hrp[u]:hrp[u + 1]].tolist() for u in range(U)}
        train_user_dict = user_hist_dict

    class Model:
        def generate(self):
            return ue, ie

    def slab_path(k, bs=512):
        out = []
        for s in range(0, U, bs):
            ub = users[s:s + bs]
            rating = K.linear(K.gather_rows(ue, ub), ie)
            rp = hrp_d[s:s + ub.numel() + 1] - hrp_d[s]
            cols = hist_d[int(hrp[s]):int(hrp[s + ub.numel()])]
            K.scatter_fill_(rating, rp.contiguous(), cols.contiguous(), -1e8)
            out.append(K.topk_rows(rating, k)[1])
        return torch.cat(out)

    def fused(k):
        return K.topk_dot_masked(ue, ie, k, hrp_d, hist_d)[1]

    def share(ms):
        return f"{ms:9.2f} ms  ({100 * floor_ms / ms:5.1f} % of fp32 MFMA peak)"

    for k in (20, 50):
        m = edge_eval.Metric("recall;ndcg;precision", f"10;{k}" if k != 10 else "10", 512)
        dl = DL()
        if args.only == "b":
            fused(k)
            for _ in range(args.reps):
                t, _ = ev_time(lambda: fused(k))
                print(f"k={k} (b) topk_dot_masked: {share(t)}")
            continue
        m.eval(Model(), dl)   # warm-up (plans the CSRs once)
        a_idx = slab_path(k)
        b_idx = fused(k)
        assert torch.equal(a_idx, b_idx), "slab and fused paths differ"
        ta, tb, tc = [], [], []
        for _ in range(args.reps):
            t, _ = ev_time(lambda: slab_path(k))
            ta.append(t)
            t, _ = ev_time(lambda: fused(k))
            tb.append(t)
            t, _ = ev_time(lambda: m.eval(Model(), dl))
            tc.append(t)
        t0 = time.time()
        idx = slab_path(k).cpu().numpy()
        truth = [set(DL.test_user_dict[u]) for u in range(U)]
        edge_eval.recall_ndcg(idx, truth, k)
        t_a_full = (time.time() - t0) * 1e3
        print(f"k={k} (a)  slab loop + host recall_ndcg: {share(t_a_full)}  (wall, one run)")
        print(f"k={k} (a') slab loop, device only:       {share(min(ta))}  (min of {args.reps}; all {[round(x, 2) for x in ta]})")
        print(f"k={k} (b)  topk_dot_masked, one call:    {share(min(tb))}  (min of {args.reps}; all {[round(x, 2) for x in tb]})")
        print(f"k={k} (c)  Metric.eval:                  {share(min(tc))}  (min of {args.reps}; all {[round(x, 2) for x in tc]})")


if __name__ == "__main__":
    main()
