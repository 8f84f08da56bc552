"""Device dense -> CSR, the parts a machine without a GPU can check: both entries are declared in the header and bound in
_native (the export test of tests/test_cpu_abi_and_host.py then covers the library itself), CSRGraph.from_dense on host
tensors is the torch construction it always was, and a padded graph refuses what enumerates its slots."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ragraph_dense_to_csr_workspace_bytes", "ragraph_dense_to_csr_f32")


def test_entries_declared_in_the_header_and_bound():
    from ragraph_amd import _native

    header = open(os.path.join(ROOT, "include", "ragraph_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/ragraph_hip.h"
        assert name in _native.SIGNATURES, f"{name} is not bound in ragraph_amd/_native.py"
    res, args = _native.SIGNATURES["ragraph_dense_to_csr_f32"]
    decl = re.search(r"int\s+ragraph_dense_to_csr_f32\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(args) == len(decl.split(",")) == 12
    # the comment names the reference code that builds and consumes the dense form
    assert "RAGraph_node/layers/gcn.py:26-40" in header and "ragraph_utils/utility.py:43-66" in header


def test_workspace_query_without_a_device():
    """The size query is host arithmetic: 4 (rows + 1) bytes of counts and the scan's scratch; 0 outside the limits."""
    from ragraph_amd import _native

    L = _native.lib()
    f = L.ragraph_dense_to_csr_workspace_bytes
    assert f(0, 5) >= 4 and f(5, 0) >= 24
    assert 4 * 4097 <= f(4096, 4096) < 4 * 4097 + 4096
    assert f(-1, 3) == 0 and f(3, -1) == 0
    assert f(46341, 46341) == 0 and f(1 << 16, 1 << 15) == 0      # 2^31 elements or more
    assert f(46340, 46340) > 0 and f((1 << 16) - 1, 1 << 15) > 0


def _torch_from_dense(a):
    nz = torch.nonzero(a, as_tuple=False)
    rows, cols = nz[:, 0], nz[:, 1]
    rowptr = torch.zeros(a.shape[0] + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=a.shape[0]), 0)
    return rowptr, cols.to(torch.int32), a[rows, cols].float()


@pytest.mark.parametrize("batched", [False, True])
def test_from_dense_on_host_tensors_is_unchanged(batched):
    from ragraph_amd.graph import CSRGraph, as_csr

    g0 = torch.Generator().manual_seed(3)
    a = torch.rand(37, 37, generator=g0)
    a = torch.where(a < 0.2, a, torch.zeros_like(a))
    a[5] = 0                                       # an isolated node
    a[:, 9] = 0
    a[3, 4] = -0.0
    rowptr, col, val = _torch_from_dense(a)
    for g in (CSRGraph.from_dense(a[None] if batched else a), as_csr(a[None] if batched else a)):
        assert g.n == 37 and not g.padded and g.status is None
        assert g.rowptr.dtype == torch.int64 and g.col.dtype == torch.int32 and g.val.dtype == torch.float32
        assert torch.equal(g.rowptr, rowptr) and torch.equal(g.col, col) and torch.equal(g.val, val)
        assert g._has_long_rows is None            # (host tensors: looked up lazily, as before)
    with pytest.raises(ValueError):
        CSRGraph.from_dense(a, capacity=10)        # a capacity is for device tensors


def test_padded_graph_refuses_what_enumerates_its_slots():
    from ragraph_amd._native import RagraphNativeError
    from ragraph_amd.graph import CSRGraph

    rowptr = torch.tensor([0, 2, 2, 3], dtype=torch.int64)
    col = torch.tensor([0, 2, 1, 7, 7, 7, 7, 7, 7], dtype=torch.int32)       # 3 entries, 9 slots
    val = torch.tensor([1.0, 2.0, 3.0, 9, 9, 9, 9, 9, 9])
    g = CSRGraph(rowptr, col, val, 3, padded=True)
    for call in (g.row_ids, g.transposed, lambda: g.permuted(torch.tensor([2, 0, 1])), lambda: g.tile_plan(8),
                 lambda: g.tiled_values(None, val)):
        with pytest.raises(RagraphNativeError, match="padded graph is inference-only"):
            call()
    plain = CSRGraph(rowptr, col[:3], val[:3], 3)
    assert plain.padded is False
    assert plain.row_ids().tolist() == [0, 0, 2]
    assert plain.tile_plan(8) is None              # (host tensors are not tiled: no error)
