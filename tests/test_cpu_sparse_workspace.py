"""The two hub-row workspace sizes of csrc/sparse.hip pinned to their closed forms (host code only: no device needed).
Both areas come from one layout function fed by two capacity rules; every piece is rounded up to 256 bytes, so the total
does not depend on the order of the pieces."""
import itertools

import pytest

ROW_BLOCK = 4096
NNZ = (0, 4095, 4096, 4097, 123_457, 44_000_000)
DS = (0, 4, 64, 256)
RS = (0, 1, 7, 6144, 4_000_000)


def _lib():
    from ragraph_amd import _native as N

    return N.lib()


def a(x):
    return (x + 255) // 256 * 256


def sparse_closed_form(nnz, D):
    mr, mt = nnz // ROW_BLOCK + 1, 2 * (nnz // ROW_BLOCK) + 2
    return a(8) + a(8 * mr) + a(4 * mr) + a(8 * mt) + a(4 * mt) + a(4 * mt * max(D, 1))


def rows_closed_form(nnz, R, D):
    mt = R + nnz // ROW_BLOCK + 1
    mr = mt // 2 + 1
    return a(8) + a(4 * max(R, 1)) + a(8 * mr) + a(4 * mr) + a(8 * mt) + a(4 * mt) + a(4 * mt * D)


def test_python_constant_is_the_block_size():
    from ragraph_amd import kernels as K

    assert K.ROW_BLOCK == ROW_BLOCK


@pytest.mark.parametrize("nnz,D", list(itertools.product(NNZ, DS)))
def test_sparse_workspace_bytes_closed_form(nnz, D):
    assert _lib().ragraph_sparse_workspace_bytes(nnz, D) == sparse_closed_form(nnz, D)


@pytest.mark.parametrize("nnz", NNZ)
def test_rows_workspace_bytes_closed_form(nnz):
    f = _lib().ragraph_spmm_csr_rows_workspace_bytes
    for R, D in itertools.product(RS, [d for d in DS if d >= 1]):
        assert f(nnz, R, D) == rows_closed_form(nnz, R, D), (nnz, R, D)


def test_zero_on_bad_arguments():
    L = _lib()
    assert L.ragraph_sparse_workspace_bytes(-1, 64) == 0
    assert L.ragraph_sparse_workspace_bytes(4097, -1) == 0
    f = L.ragraph_spmm_csr_rows_workspace_bytes
    assert f(-1, 7, 64) == 0 and f(4097, -1, 64) == 0
    assert f(4097, 7, 0) == 0 and f(4097, 7, -4) == 0
    # R + nnz // 4096 + 1 >= 2**31 - 1: the task counter is an int
    assert f(0, 2**31 - 2, 4) == 0 and f(4096 * 5, 2**31 - 7, 4) == 0 and f(0, 2**31, 4) == 0
    assert f(0, 2**31 - 3, 4) == rows_closed_form(0, 2**31 - 3, 4)
