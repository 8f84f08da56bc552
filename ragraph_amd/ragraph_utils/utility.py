"""Mirror of RAGraph_*/ragraph_utils/utility.py: seeding and TU-batch preprocessing, emitting CSR instead of a dense
block-diagonal adjacency (the numpy row_stack loop of utility.py:43-58 is quadratic in the batch's node count)."""
import os
import random

import numpy as np
import torch

from ..graph import CSRGraph


def seed_everything(seed: int):
    """utility.py:5-16."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)


def process_tu_dataset(data, num_node_attributes, device="cuda"):
    """utility.py:30-72 (node flavour): a PyG-style batch -> (features [n,F], adj CSRGraph, node_labels [n,C]).
    `data` needs .x [n, F + C] (attributes then one-hot node labels) and .edge_index [2,E] with batch-global node ids
    (what torch_geometric's Batch holds; block-diagonal structure is implicit)."""
    x = data.x.to(device)
    features = x[:, :num_node_attributes].float().contiguous()
    node_labels = x[:, num_node_attributes:].float().contiguous()
    adj = CSRGraph.from_edge_index_sym_normalized(data.edge_index.to(device), x.shape[0])
    return features, adj, node_labels


# ---- few-shot prototypes (RAGraph_node_fewshot/ragraph_utils/utility.py:114-162, same in RAGraph_graph_fewshot) -------
# The reference builds them with one unique() and a .item() per class: a read-back per class per training step
# (finetune-rag.py:96-101), which a HIP graph cannot hold.  Here the rows are ordered by label with the library's stable
# COO -> CSR sort (one call: the class pointer and the row order), summed per class by segment_sum and divided by the
# class sizes on the device; only the reference's missing-label check reads labels back, and not under capture.
def fewshot_mean_logits(fewshot_logits: torch.Tensor, fewshot_labels: torch.Tensor, num_class: int | None = None):
    """[C, D]: row c = the mean of the rows of `fewshot_logits` labelled c, c = 0..C-1.  num_class=None: C is the number of
    distinct labels and a label of range(C) that no row carries raises KeyError, as the reference does (one read-back).
    Under HIP graph capture pass num_class: nothing is read back, a class without rows gives a zero row and labels outside
    [0, num_class) are ignored.  Differentiable in fewshot_logits."""
    from .. import autograd as A
    from .. import kernels as K

    labels = fewshot_labels.reshape(-1)
    n = labels.numel()
    if fewshot_logits.dim() != 2 or fewshot_logits.shape[0] != n:
        raise ValueError(f"fewshot_mean_logits: logits {tuple(fewshot_logits.shape)} for {n} labels")
    if num_class is None:
        if torch.cuda.is_current_stream_capturing():
            raise K.RagraphNativeError("fewshot_mean_logits: pass num_class under HIP graph capture (the class count is "
                                       "otherwise read back from the labels)")
        present = set(int(v) for v in torch.unique(labels).tolist())
        num_class = len(present)
        for c in range(num_class):
            if c not in present:
                raise KeyError(c)   # (the reference's label_to_logit[label] for label in range(len(label_to_logit)))
    C = int(num_class)
    if C < 1:
        raise ValueError("fewshot_mean_logits: no class")
    lab = labels.to(torch.int64)
    lab = torch.where((lab >= 0) & (lab < C), lab, torch.full_like(lab, C))   # (other labels: a slot nobody reads)
    ptr, _, perm = K.coo_to_csr(lab, torch.arange(n, dtype=torch.int64, device=lab.device), C + 1)
    sums = A.segment_sum(A.gather_rows(fewshot_logits.contiguous(), perm), ptr)[:C]
    counts = (ptr[1:C + 1] - ptr[:C]).clamp(min=1).to(sums.dtype)
    return sums / counts.unsqueeze(1)


def fewshot_predict_logits(mean_fewshot_logits: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
    """[B, C] cosine of every row of `logits` with every class mean (torch.cosine_similarity, eps = 1e-8) on the
    proto_cosine kernel; differentiable in logits (and in the means when they require a gradient).  C <= 64."""
    from .. import autograd as A

    return A.proto_cosine(logits, mean_fewshot_logits.contiguous(), 0)


def fewshot_predict_labels_by_mean(mean_fewshot_logits: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
    """[B] int64: the class whose mean is the most similar (the first of equal cosines, as Tensor.max(dim=1))."""
    with torch.no_grad():
        _, predicted = fewshot_predict_logits(mean_fewshot_logits, logits).max(dim=1)
    return predicted
