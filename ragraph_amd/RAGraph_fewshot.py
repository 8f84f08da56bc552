"""Mirror of RAGraph_node_fewshot: retrieval mixes a STRUCTURAL similarity (position-aware codes from all-pairs
shortest paths to random anchors) with the semantic cosine, the decoder is the encoder's second GCN layer, and the
label term is a prototype-logit lookup.

Retrieval is one call of the mixed top-k (K.topk_cosine_mix): small score matrices (B ~ 40 query nodes x a few thousand
bank rows) are materialised inside it exactly as the reference does (ToyGraphBase.py:47-61: two cosine matrices on the
HIP linear kernel, the uncontracted mix, the HIP top-k over rows), banks too large for that stream through the fused
kernels -- the same bits.  `similarity_scores` keeps the materialised matrix for callers that want it.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import kernels as K
from .graph import CSRGraph, as_csr
from .ragraph_utils.Propagation import Propagation
from .ragraph_utils.ToyGraphBase import ToyGraphBase, _Bank


def _dense(adj) -> torch.Tensor:
    if isinstance(adj, torch.Tensor) and adj.layout == torch.strided:
        return adj.squeeze(0) if adj.dim() == 3 else adj
    g: CSRGraph = as_csr(adj)
    a = torch.zeros(g.n, g.n, device=g.device)
    rows = torch.repeat_interleave(torch.arange(g.n, device=g.device), g.rowptr[1:] - g.rowptr[:-1])
    a[rows, g.col.long()] = g.val
    return a


class PositionAwareEncoder:
    """ragraph_utils/PositionAwareEncoder.py: distance-to-anchor codes.  The reference runs an all-pairs Floyd-Warshall as
    n dense torch.min broadcasts and fills the code matrix in a Python double loop -- to use 10 columns of the n x n
    matrix.  The codes here come from the distances to the anchors ONLY, relaxed on the CSR of the (block-diagonal)
    batch in one launch (K.position_codes_csr: no n x n allocation, no n dependent launches); `floyd_warshall` keeps the
    reference's all-pairs entry for callers that want the matrix."""

    @staticmethod
    def floyd_warshall(adj) -> torch.Tensor:
        return K.floyd_warshall(_dense(adj))

    @staticmethod
    def encode_position_aware_code(adj, num_anchors: int, dis_q: int = 10, anchors: torch.Tensor | None = None,
                                   rounds: int | None = None):
        """`rounds`: a fixed number of relaxation rounds (K.position_codes_csr: the capturable form for graphs of more
        than 40000 nodes); the result is then (codes, converged word on the device)."""
        g: CSRGraph = as_csr(adj.squeeze(0) if isinstance(adj, torch.Tensor) and adj.layout == torch.strided
                             and adj.dim() == 3 else adj)
        if anchors is None:  # PositionAwareEncoder.py:11 draws them from torch's global CPU generator
            anchors = torch.randint(low=0, high=g.n, size=(int(num_anchors),))
        if rounds is None:
            return K.position_codes_csr(g.rowptr, g.col, g.val, anchors.to(g.device), float(dis_q))
        return K.position_codes_csr(g.rowptr, g.col, g.val, anchors.to(g.device), float(dis_q), rounds=rounds,
                                    return_converged=True)


class ToyGraphBaseFewShot(ToyGraphBase):
    """RAGraph_node_fewshot/ragraph_utils/ToyGraphBase.py."""

    def __init__(self, pretrain_model, num_class, emb_size, query_graph_hop, retrieve_num, device="cuda"):
        super().__init__(pretrain_model, num_class, emb_size, query_graph_hop, device=device, flavour="node")
        self.retrieve_num = retrieve_num
        self.num_anchors = 10
        self.dis_q = 10
        self.structure_weight = 0.001   # :28-29
        self.semantic_weight = 0.999
        self._positions = _Bank(self.num_anchors, self.device)

    @property
    def resource_positions(self):
        return self._positions.view()

    def add_resources(self, keys, values, labels, positions=None):
        if positions is None:
            positions = torch.zeros(keys.shape[0], self.num_anchors, device=self.device)
        super().add_resources(keys, values, labels, positions)   # (one path: the normalised caches grow with the bank)

    def similarity_scores(self, search_keys, search_adj, anchors=None):
        """ToyGraphBase.py:49-61: structure_weight * cos(position codes) + semantic_weight * cos(embeddings)."""
        pos = PositionAwareEncoder.encode_position_aware_code(search_adj, self.num_anchors, self.dis_q, anchors)
        s_struct = K.linear(K.normalize_rows(pos), K.normalize_rows(self.resource_positions))
        s_sem = K.linear(K.normalize_rows(search_keys), self.keys_normalized)
        return K.axpby(s_struct, self.structure_weight, s_sem, self.semantic_weight)

    def retrieve(self, search_keys, search_adj, add_noise: bool, anchors=None, row_ids=None, row_base: int = 0):
        """`row_ids` / `row_base`: the keys of the noise rows with noise_rng = "device" (ToyGraphBase.retrieve_indices)."""
        retrieve_num = 2 * self.retrieve_num if add_noise else self.retrieve_num
        if add_noise or self.structure_weight == 0:   # (uniform draws, or scores over every physical row: live rows only)
            self._compact_before_uniform_draws()
        if self.structure_weight != 0:   # :49-64 in one call, no [B, N] matrix in this module
            pos = self.search_positions(search_adj, None, anchors)
            _, idx = self.topk(search_keys, retrieve_num, pos)
        else:   # (a caller that zeroed the structural weight: the reference still scales the scores, :61)
            _, idx = K.topk_rows(self.similarity_scores(search_keys, search_adj, anchors), retrieve_num)
        rag_embeddings = K.gather_rows(self.resource_values, idx)
        rag_labels = K.gather_rows(self.resource_labels, idx)
        if add_noise:                                                                # :70-76
            if self.noise_rng == "device":
                noise_idx = K.noise_rows(self._draw_noise_seed(), idx.shape[0], self.noise_retrieve_num,
                                         self.resource_values.shape[0], row_ids, row_base)
            else:
                noise_idx = torch.randint(0, self.resource_values.shape[0], (idx.shape[0], self.noise_retrieve_num),
                                          device=idx.device)
            rag_embeddings = torch.cat([rag_embeddings, K.gather_rows(self.resource_values, noise_idx)], dim=1)
            rag_labels = torch.cat([rag_labels, K.gather_rows(self.resource_labels, noise_idx)], dim=1)
        return rag_embeddings, rag_labels


def _reject_noise_under_capture(add_noise: bool, noise_rng: str = "host"):
    """noise_rng = "device" (ToyGraphBase.noise_rng): the noise is made inside the kernels from a seed drawn on the device
    generator, which a capture records -- nothing to reject."""
    if add_noise and noise_rng != "device" and torch.cuda.is_current_stream_capturing():
        raise K.RagraphNativeError("noisy fine-tuning draws new noise rows every step (on the host generator in the graph "
                                   "flavour, as the reference does): its step is not captured in a HIP graph (train it eagerly)")


class RAGraph(nn.Module):
    """RAGraph_node_fewshot/RAGraph.py:7-83.  In training mode the second GCN layer trains through decode()
    (autograd.spmm_csr, slope on the device) and the label mix (:77): a whole step can be captured
    (ragraph_amd.capture.CapturedTrainStep) when the anchors of the position codes are passed in (the reference draws
    them from the host generator every forward)."""

    def __init__(self, pretrain_model, resource_dataset, mean_fewshot_logits, emb_size, finetune=True,
                 noise_finetune=False, query_graph_hop=3, retrieve_num=5, device="cuda", dataset_name=None, build_rng="host"):
        super().__init__()
        self.emb_size = emb_size
        self.pretrain_model = pretrain_model
        name = dataset_name or getattr(resource_dataset, "name", "ENZYMES")
        if name == "PROTEINS":                       # RAGraph.py:25-32
            self.retrieve_weight, self.label_weight = 0.3, 0.8
        else:
            self.retrieve_weight, self.label_weight = 0.5, 0.5
        self.finetune, self.noise_finetune = finetune, noise_finetune
        self.query_graph_hop = query_graph_hop
        self.toy_graph_base = ToyGraphBaseFewShot(pretrain_model, len(mean_fewshot_logits), emb_size, query_graph_hop,
                                                  retrieve_num, device=device)
        self.toy_graph_base.build_rng = build_rng   # (ToyGraphBase.build_rng: read when the bank is built)

    def forward(self, features, adj, mean_fewshot_logits, anchors=None):
        g = as_csr(adj)
        emb = self.pretrain_model.encode(features, g)                                           # :48
        add_noise = self.training and self.noise_finetune
        _reject_noise_under_capture(add_noise, self.toy_graph_base.noise_rng)
        if anchors is None and torch.cuda.is_current_stream_capturing():
            raise K.RagraphNativeError("RAGraph_fewshot.RAGraph: pass `anchors` to a captured forward (drawn on the host "
                                       "generator otherwise: PositionAwareEncoder.py:11)")
        rag_embeddings, rag_labels = self.toy_graph_base.retrieve(emb, g, add_noise, anchors)    # :51
        label_ids = torch.argmax(rag_labels, dim=-1)                                             # :54 (integer lookup)
        k = label_ids.shape[1]
        rag_logits, _ = K.gather_reduce(mean_fewshot_logits, None, label_ids, v_scale=1.0 / k)   # :55,62 mean over k
        if not self.finetune:
            return rag_logits
        # :63 torch.sum(rag_embeddings, dim=1): rank-order fp32 adds over the gathered [B,k,D] rows
        flat = rag_embeddings.reshape(-1, rag_embeddings.shape[-1])
        rows = torch.arange(flat.shape[0], device=emb.device).reshape(-1, k)
        rag_embedding, _ = K.gather_reduce(flat, None, rows)
        query = Propagation.aggregate_k_hop_features(g, emb, self.query_graph_hop)               # :65
        hidden = K.axpby(query, 1 - self.retrieve_weight, rag_embedding, self.retrieve_weight)   # :67
        decode_logits = self.pretrain_model.decode(hidden, g)                                    # :69
        from . import autograd as A   # (differentiable when decode() trains; the same kernel otherwise)
        return A.axpby(decode_logits, 1 - self.label_weight, rag_logits, self.label_weight)      # :77


class RAGraphGraphFewShot(nn.Module):
    """RAGraph_graph_fewshot/RAGraph.py:7-91: graph classification, few-shot.  EVERY node of the one query graph is a query
    against a bank that holds every node of every resource graph with its graph's label
    (ragraph_utils/ToyGraphBase.py:118-126); the label term is a prototype-logit lookup, the decoder is the encoder's
    second GCN layer (trained through decode(): ragraph_amd.autograd.spmm_csr), and the node logits are averaged into one
    row (:86).  FewShotBase (RAGraph.py:43) only loads blobs that forward never reads and is not reproduced."""

    def __init__(self, pretrain_model, resource_dataset, feture_size, num_class, emb_size, finetune=True,
                 noise_finetune=False, device="cuda", dataset_name=None, build_rng="host"):
        super().__init__()
        self.emb_size, self.num_class, self.pretrain_model = emb_size, num_class, pretrain_model
        name = dataset_name or getattr(resource_dataset, "name", "PROTEINS")
        weights = {"ENZYMES": (0.3, 0.8), "PROTEINS": (0.5, 0.5), "COX2": (0.3, 0.6), "BZR": (0.1, 0.5)}   # RAGraph.py:16-30
        if name not in weights:
            raise NotImplementedError(name)
        self.retrieve_weight, self.label_weight = weights[name]
        self.finetune, self.noise_finetune = finetune, noise_finetune
        if noise_finetune:
            assert finetune
        self.query_graph_hop = 1                                                               # :38
        self.toy_graph_base = ToyGraphBase(pretrain_model, num_class, emb_size, self.query_graph_hop, device=device,
                                           flavour="graph_fewshot")
        self.toy_graph_base.build_rng = build_rng   # (no draw in this flavour's build: accepted for a uniform interface)
        if resource_dataset is not None:
            self.toy_graph_base.build_toy_graph(resource_dataset)
        self.to(device)

    def forward(self, features, adj, mean_fewshot_logits):
        from . import autograd as A
        g = as_csr(adj)
        tgb = self.toy_graph_base
        emb = self.pretrain_model.encode(features, g)                                            # :47
        add_noise = self.training and self.noise_finetune
        _reject_noise_under_capture(add_noise, self.toy_graph_base.noise_rng)
        idx = tgb.retrieve_indices(emb, add_noise)                                               # :51 (k' = 2k with noise)
        k = idx.shape[1]
        label_ids = torch.argmax(K.gather_rows(tgb.resource_labels, idx), dim=-1)                # :55 (integer lookup)
        rag_logits, _ = K.gather_reduce(mean_fewshot_logits, None, label_ids, v_scale=1.0 / k)   # :56,68 mean over k
        if not self.finetune:
            return rag_logits                                                                    # :88-91
        if add_noise:                                                                            # graph noise: on the embeddings
            rag_embedding, _ = tgb.retrieve_reduced_noisy(emb, idx=idx, want_labels=False)
        else:
            rag_embedding, _ = K.gather_reduce(tgb.resource_values, None, idx)                   # :69 sum over k
        query = Propagation.aggregate_k_hop_features(g, emb, self.query_graph_hop)               # :71
        hidden = K.axpby(query, 1 - self.retrieve_weight, rag_embedding, self.retrieve_weight)   # :75
        decode_logits = self.pretrain_model.decode(hidden, g)                                    # :79
        label_logits = A.axpby(decode_logits, 1 - self.label_weight, rag_logits, self.label_weight)   # :82
        if label_logits.requires_grad:   # training: the mean over the nodes through torch (one reduction of [n, D])
            return label_logits.mean(dim=0).unsqueeze(0)                                         # :84
        seg = torch.tensor([0, label_logits.shape[0]], dtype=torch.int64, device=label_logits.device)
        return K.segment_reduce(label_logits, seg, mean_mode=True)                               # :84
