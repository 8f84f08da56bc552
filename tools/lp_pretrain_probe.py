#!/usr/bin/env python3
"""Link-prediction pre-training (csrc/pretrain.hip), on one GPU.  Device-event times after warm-up, medians of --reps:
  * sampler: prompt_pretrain_sample on the device, and the reference's numpy algorithm (setdiff1d + two shuffles per
    node, restated here) at the sizes where it finishes (528, 10 k; host wall time);
  * compare loss forward and backward (ragraph_amd.preprompt.compareloss) against the reference's op chain run as torch
    ops on the same GPU (gather to [n, 1 + n_neg, D] twice, F.cosine_similarity, exp / log chain, autograd).
Shapes: n = 528 (an ENZYMES batch of 16 graphs), 10 k and 100 k nodes of a random graph with mean degree 8, D = 256,
100 negatives.

Usage:  python tools/lp_pretrain_probe.py [--reps 5] [--sizes 528,10000,100000]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragraph_amd.graph import CSRGraph  # noqa: E402
from ragraph_amd.preprompt import compareloss, prompt_pretrain_sample  # noqa: E402


def ev_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def torch_chain(feature, tuples, temperature=1.5):
    n, S = tuples.shape
    D = feature.shape[1]
    h_t = torch.gather(feature, 0, tuples.reshape(-1, 1).expand(-1, D)).reshape(n, S, D)
    own = torch.arange(n, device=feature.device).reshape(-1, 1).expand(n, S)
    h_i = torch.gather(feature, 0, own.reshape(-1, 1).expand(-1, D)).reshape(n, S, D)
    sim = F.cosine_similarity(h_i, h_t, dim=2)
    e = (torch.exp(sim) / temperature).permute(1, 0)
    return (-1 * torch.log(e[0].reshape(-1, 1) / e[1:].permute(1, 0).sum(dim=1, keepdim=True))).mean()


def numpy_sampler(indptr, indices, n_neg):
    """The reference's per-node algorithm: the complement by setdiff1d, both lists shuffled, the heads taken."""
    nodenum = len(indptr) - 1
    n_neg = min(n_neg, nodenum)
    res = np.zeros((nodenum, 1 + n_neg))
    whole = np.arange(nodenum)
    for i in range(nodenum):
        nb = indices[indptr[i]:indptr[i + 1]].copy()
        comp = np.setdiff1d(whole, nb)
        np.random.shuffle(nb)
        np.random.shuffle(comp)
        res[i, 0] = i if nb.size == 0 else nb[0]
        res[i, 1:] = comp[:n_neg]
    return res.astype(int)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="528,10000,100000")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--neg", type=int, default=100)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    D, n_neg = args.dim, args.neg
    print(f"# {torch.cuda.get_device_name(dev)}; D = {D}, {n_neg} negatives, medians of {args.reps} (ms)")
    print(f"{'n':>7} {'sample':>9} {'np_sample':>10} {'fwd':>8} {'bwd':>8} {'torch_fwd':>10} {'torch_bwd':>10} "
          f"{'fwd_x':>6} {'bwd_x':>6} {'step_x':>6}")
    for n in [int(s) for s in args.sizes.split(",")]:
        g = torch.Generator(device=dev).manual_seed(n)
        m = 4 * n
        ei = torch.randint(0, n, (2, m), device=dev, generator=g)
        ei = torch.cat([ei, ei.flip(0)], 1)
        adj = CSRGraph.from_edge_index_sym_normalized(ei, n)
        t_samp = ev_ms(lambda: prompt_pretrain_sample(adj, n_neg, generator=g), args.reps)
        t = prompt_pretrain_sample(adj, n_neg, generator=g)
        np_ms = float("nan")
        if n <= 10000:
            a = sp.csr_matrix((np.ones(adj.nnz), adj.col.cpu().numpy(), adj.rowptr.cpu().numpy()), shape=(n, n))
            a.setdiag(0)                                                # the raw A has no self loops
            a.eliminate_zeros()
            t0 = time.perf_counter()
            numpy_sampler(a.indptr, a.indices, n_neg)
            np_ms = (time.perf_counter() - t0) * 1e3
        h = torch.randn(n, D, device=dev, requires_grad=True)
        go = torch.ones((), device=dev)

        def ours_fwd():
            with torch.no_grad():
                compareloss(h, t, 1.5)

        def ours_step():
            loss = compareloss(h, t, 1.5)
            loss.backward(go)

        def ref_fwd():
            with torch.no_grad():
                torch_chain(h, t)

        def ref_step():
            loss = torch_chain(h, t)
            loss.backward(go)

        f_ours, s_ours = ev_ms(ours_fwd, args.reps), ev_ms(ours_step, args.reps)
        f_ref, s_ref = ev_ms(ref_fwd, args.reps), ev_ms(ref_step, args.reps)
        b_ours, b_ref = s_ours - f_ours, s_ref - f_ref
        print(f"{n:>7} {t_samp:>9.3f} {np_ms:>10.1f} {f_ours:>8.3f} {b_ours:>8.3f} {f_ref:>10.3f} {b_ref:>10.3f} "
              f"{f_ref / f_ours:>6.1f} {b_ref / max(b_ours, 1e-6):>6.1f} {s_ref / s_ours:>6.1f}")
        del h
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
