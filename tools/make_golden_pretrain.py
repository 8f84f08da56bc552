#!/usr/bin/env python3
"""Generate tests/golden/g18_lp_pretrain.npz by running the REFERENCE's own link-prediction pre-training step on CPU:
preprompt.prompt_pretrain_sample (numpy, seeded), PrePrompt.forward (GcnLayers in LP mode -> ELU -> compareloss) and
.backward(), for a node-flavour batch (RAGraph_node: 100 negatives) and a graph-flavour batch (RAGraph_graph: 50).

Uses oracle/make_golden.py's import context unchanged.  Dropout p = 0, so the step is deterministic; BatchNorm runs in
train mode (batch statistics, running statistics updated once).  The bias, PReLU slope and BatchNorm affine parameters
are set to non-default values so that every gradient is exercised.  Each graph has an isolated node (its positive is
itself) and the raw adjacency has no self loops, as process_tu returns it; the encoder takes A_hat = D^-1/2 (A + I) D^-1/2
(utils/process.py normalize_adj), recorded in CSR form.

Recorded per flavour (prefix node_ / graph_): X, adj_rowptr / adj_col / adj_val (A_hat), raw_rowptr / raw_col (A),
W, bias, alpha, bn_weight, bn_bias (the parameters before the step), sample, elu, loss, the gradients g_W, g_bias,
g_alpha, g_bn_weight, g_bn_bias, and bn_running_mean / bn_running_var after the step.

Usage:  python tools/make_golden_pretrain.py   (writes tests/golden/g18_lp_pretrain.npz)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.make_golden import _install_shims, gen, ref_project, save  # noqa: E402

F_IN, D = 18, 256
FLAVOURS = (("node", "RAGraph_node", 300, 100, 18), ("graph", "RAGraph_graph", 160, 50, 28))


def _raw_graph(n, mean_deg, seed):
    """Symmetric 0/1 adjacency without self loops; node n - 1 is isolated."""
    rng = np.random.default_rng(seed)
    m = int(n * mean_deg / 2)
    r, c = rng.integers(0, n - 1, m), rng.integers(0, n - 1, m)
    keep = r != c
    a = sp.coo_matrix((np.ones(keep.sum()), (r[keep], c[keep])), shape=(n, n)).tocsr()
    a = ((a + a.T) > 0).astype(np.float64).tocsr()
    a.sort_indices()
    return a


def _flavour(tag, project, n, n_neg, seed):
    with ref_project(project):
        import preprompt
        from preprompt import PrePrompt
        from utils import process

        raw = _raw_graph(n, 3.7, seed)
        adj_hat = process.normalize_adj(raw + sp.eye(n)).tocsr()
        adj_hat.sort_indices()
        adj_dense = torch.FloatTensor(np.asarray(adj_hat.todense())[np.newaxis])
        X = torch.rand(1, n, F_IN, generator=gen(seed + 1))

        torch.manual_seed(seed + 2)
        model = PrePrompt(F_IN, D, "prelu", 1, 0.0)
        conv, bn = model.gcn.convs[0], model.gcn.bns[0]
        with torch.no_grad():
            conv.bias.copy_(0.1 * torch.randn(D, generator=gen(seed + 3)))
            conv.act.weight.fill_(0.2)
            bn.weight.copy_(1.0 + 0.1 * torch.randn(D, generator=gen(seed + 4)))
            bn.bias.copy_(0.1 * torch.randn(D, generator=gen(seed + 5)))
        params = {"W": conv.fc.weight.detach().clone(), "bias": conv.bias.detach().clone(),
                  "alpha": conv.act.weight.detach().clone(), "bn_weight": bn.weight.detach().clone(),
                  "bn_bias": bn.bias.detach().clone()}

        np.random.seed(seed + 6)
        sample = preprompt.prompt_pretrain_sample(raw.copy(), n_neg)   # (shuffles its indices in place: a copy)
        model.train()
        elu = model.lp(model.gcn, X.squeeze(0), adj_dense, False)
        bn.reset_running_stats()                                        # (the probe above stepped them once)
        bn.num_batches_tracked.zero_()
        loss = model(X, X, X, X, adj_dense, None, None, False, None, None, None, lbl=None, sample=sample)
        loss.backward()

    out = {"X": X.squeeze(0), "adj_rowptr": adj_hat.indptr.astype(np.int64), "adj_col": adj_hat.indices.astype(np.int32),
           "adj_val": adj_hat.data.astype(np.float32), "raw_rowptr": raw.indptr.astype(np.int64),
           "raw_col": raw.indices.astype(np.int32), "sample": sample.astype(np.int32), "elu": elu.detach(),
           "loss": np.float32(loss.item()), "n_neg": np.int64(n_neg),
           "g_W": conv.fc.weight.grad, "g_bias": conv.bias.grad, "g_alpha": conv.act.weight.grad,
           "g_bn_weight": bn.weight.grad, "g_bn_bias": bn.bias.grad,
           "bn_running_mean": bn.running_mean, "bn_running_var": bn.running_var}
    out.update(params)
    return {f"{tag}_{k}": v for k, v in out.items()}


def main():
    _install_shims()
    torch.set_num_threads(4)
    arrays = {}
    for tag, project, n, n_neg, seed in FLAVOURS:
        arrays.update(_flavour(tag, project, n, n_neg, seed))
    save("g18_lp_pretrain", **arrays)


if __name__ == "__main__":
    main()
