"""Row-subset SpMM: the header declares the entries, the library exports them, and the workspace size is what the kernels
assume (host code only: no device needed)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ragraph_spmm_csr_rows_f32", "ragraph_spmm_csr_rows_workspace_bytes")


def _lib():
    from ragraph_amd import _native as N

    return N.lib()


def test_header_declares_and_library_exports_the_entries():
    header = open(os.path.join(ROOT, "include", "ragraph_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(_lib(), name), name
    assert "RAGraph_edge/modules/RAGraph.py:232-240,327,343-345" in header


@pytest.mark.parametrize("nnz,R,D", [(0, 1, 4), (4096, 1, 8), (4097, 7, 64), (123_457, 6144, 64), (44_000_000, 6144, 64),
                                     (44_000_000, 4_000_000, 256)])
def test_workspace_bytes(nnz, R, D):
    f = _lib().ragraph_spmm_csr_rows_workspace_bytes
    b = f(nnz, R, D)
    assert b > 0 and b % 16 == 0
    assert b >= (R + nnz // 4096) * D * 4
    assert f(nnz + 1, R, D) >= b and f(nnz + 4096, R, D) >= b and f(nnz * 2 + 5, R, D) >= b
    assert f(nnz, R + 1, D) >= b and f(nnz, 2 * R + 3, D) >= b
    assert f(nnz, R, D + 4) >= b and f(nnz, R, 2 * D) >= b
