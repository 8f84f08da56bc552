"""Mirror of RAGraph_*/preprompt.py :: PrePrompt -- the encoder stack and its link-prediction pre-training objective
(prompt_pretrain_sample, compareloss, PrePrompt.forward); DGI / GraphCL are out of scope
(dead code in the reference's own pre-training: forward returns only the LP loss)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import autograd as A
from . import kernels as K
from .gcnlayers import GcnLayers
from .graph import CSRGraph, as_csr
from .layers.gcn import sparse_features

LP_TEMPERATURE = 1.5   # preprompt.py:52


def _sample_pattern(adj, device):
    """(rowptr, col) of A on the device, columns strictly ascending per row."""
    if isinstance(adj, CSRGraph):
        return adj.rowptr.to(device), adj.col.to(device)
    if hasattr(adj, "tocsr") and not isinstance(adj, torch.Tensor):   # scipy sparse (the reference passes adj.indices/indptr)
        a = adj.tocsr(copy=True)
        a.sum_duplicates()
        a.sort_indices()
        return (torch.as_tensor(a.indptr.astype(np.int64), device=device),
                torch.as_tensor(a.indices.astype(np.int32), device=device))
    t = torch.as_tensor(np.asarray(adj)) if not isinstance(adj, torch.Tensor) else adj
    if t.layout == torch.sparse_csr:
        t = t.to_dense()
    g = as_csr(t.to(device))
    return g.rowptr, g.col


def prompt_pretrain_sample(adj, n, generator=None):
    """preprompt.py:106-126 on the device: int64 [nodenum, 1 + n'] with n' = min(n, nodenum).  Column 0 is a uniformly random
    neighbour of i (i itself when i has none); columns 1.. are n' distinct nodes drawn uniformly from the complement of i's
    neighbour set (i may be drawn), in unspecified order.  adj: a CSRGraph, a dense tensor / array or a scipy matrix; a
    diagonal entry is ignored, so process_tu_dataset's A_hat can be passed as it is.  The seed is drawn on the device from
    `generator` (default: torch's CUDA generator), so torch.manual_seed reproduces a sample.  A row with neighbours and
    fewer than n' non-neighbours raises ValueError (the reference fails there too)."""
    device = adj.device if isinstance(adj, (CSRGraph, torch.Tensor)) and adj.device.type == "cuda" else torch.device("cuda")
    if generator is not None and generator.device.type == "cuda":
        device = generator.device
    rowptr, col = _sample_pattern(adj, device)
    nodenum = rowptr.numel() - 1
    seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=device, generator=generator)
    return K.lp_sample(rowptr, col, min(int(n), nodenum), seed)


def compareloss(feature, tuples, temperature):
    """preprompt.py:80-103 without the [n, 1 + n_neg, D] gathers (autograd.compare_loss): differentiable in feature."""
    if not isinstance(tuples, torch.Tensor):
        tuples = torch.as_tensor(np.asarray(tuples), dtype=torch.int64)
    return A.compare_loss(feature, tuples.to(device=feature.device, dtype=torch.int64), float(temperature))


class PrePrompt(nn.Module):
    def __init__(self, n_in, n_h, activation, num_layers_num, p):
        super().__init__()
        self.gcn = GcnLayers(n_in, n_h, num_layers_num, p)

    def forward(self, seq1, seq2, seq3, seq4, adj, aug_adj1edge, aug_adj2edge, sparse, msk, samp_bias1, samp_bias2, lbl,
                sample):
        """preprompt.py:42-55: the LP loss of the ELU of the encoder in LP mode (models/LP.py: Lp.prompt is never read).
        seq2..seq4, the augmented adjacencies, msk, the sampling biases and lbl feed DGI / GraphCL, whose losses the reference
        computes nowhere: accepted and ignored.  `sample` is prompt_pretrain_sample's result -- a numpy array from the
        reference's sampler or a device tensor."""
        t = sample if isinstance(sample, torch.Tensor) else torch.as_tensor(np.asarray(sample), dtype=torch.int64)
        seq1 = torch.squeeze(seq1, 0)
        logits3 = F.elu(self.gcn(seq1, adj, sparse, True).squeeze(dim=0))   # LP.py:14-17
        return compareloss(logits3, t.to(device=logits3.device, dtype=torch.int64), temperature=LP_TEMPERATURE)

    @torch.no_grad()   # (the reference detaches the result: nothing upstream of it can train through this call)
    def embed(self, seq, adj, sparse, msk, LP):
        """preprompt.py:57-62.  Returns (h, c).  The node flavour's c is the 3-hop subgraph readout that a Python loop
        over nnz(A^3) computes (preprompt.py:8-27) and inference() throws away; here c is the plain mean readout of h
        (the graph flavour's AvgReadout, RAGraph_graph/preprompt.py:48-54)."""
        sparse_features(seq)  # (bag-of-words features are judged here, once per tensor version: layers/gcn.py)
        h = self.gcn(seq, adj, sparse, LP).squeeze(0)
        return h.detach(), h.mean(dim=0, keepdim=True).detach()

    @torch.no_grad()   # (detached by the reference: always the inference kernels, whatever the caller's grad mode)
    def inference(self, features, adj):
        """preprompt.py:64-66: L GCN layers, detached."""
        sparse_features(features)
        return self.gcn(features, adj, False, False).squeeze(0).detach()

    @torch.no_grad()
    def inference_rows(self, features, adj, lo: int, hi: int):
        """Rows [lo, hi) of inference(features, adj), bit for bit, at the cost of those rows (+ the earlier layers): what a rank
        that answers a slice of the queries needs before its retrieval can start (None: take the whole-graph call)."""
        sparse_features(features)
        h = self.gcn.forward_rows(features, adj, lo, hi)
        return None if h is None else h.detach()

    def encode(self, features, adj):  # RAGraph_node_fewshot/preprompt.py:74-75
        sparse_features(features)
        return self.gcn.encode(features, adj)

    def decode(self, features, adj):  # RAGraph_node_fewshot/preprompt.py:77-78
        return self.gcn.decode(features, adj)

    def load_reference_state_dict(self, state_dict):
        """Load a reference checkpoint (modelset/model_*.pkl): keeps gcn.convs.* / gcn.bns.*, ignores the duplicated
        gcn.g_net.* aliases and the pre-training heads (dgi, graphcledge, graphclmask, lp)."""
        own = self.state_dict()
        picked = {k: v for k, v in state_dict.items() if k in own}
        missing = [k for k in own if k not in picked and not k.startswith("gcn.g_net.") and "bns" not in k]
        if missing:
            raise KeyError(f"reference checkpoint lacks {missing}")
        return self.load_state_dict(picked, strict=False)
