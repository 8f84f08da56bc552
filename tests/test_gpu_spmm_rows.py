"""Row-subset SpMM (ragraph_spmm_csr_rows_f32, csrc/sparse.hip): Y[r] = (A X)[rows[r]] bit for bit against the full product
and the oracle at every row length around the 16-edge chunk and the 4096-edge block, with and without the hub-row workspace,
when the requested hubs overflow the partial-sum area, through autograd, and captured into a HIP graph."""
import numpy as np
import pytest
import torch

from oracle import cref

pytestmark = pytest.mark.gpu

N_ROWS = 10_000
LENGTHS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 5)     # the chunk (16) and block (4096) edges of row_chain
AT = (9001, 17, 4242, 0, 9999, 311, 5000, 7777, 2600)            # where those rows sit
ROWS = [7777, 17, 2600, 9001, 0, 2600, 311, 5000, 9999, 4242]    # scrambled, the longest row twice


def close(a, b, tol=1e-4):   # (tests/test_gpu_backward.py's measure)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _csr(seed, hub_col=None):
    """n = 10 000 rows: the listed lengths at the listed rows, 0-8 edges elsewhere; random columns and values.  hub_col: 9000
    of the rows also hold that column (a transposed row of 9000 entries)."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 9, N_ROWS)
    deg[list(AT)] = LENGTHS
    extra = np.zeros(N_ROWS, dtype=np.int64)
    if hub_col is not None:
        extra[rng.permutation(N_ROWS)[:9000]] = 1
    rowptr = np.zeros(N_ROWS + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg + extra)
    col = rng.integers(0, N_ROWS, int(rowptr[-1])).astype(np.int32)
    if hub_col is not None:
        col[rowptr[:-1][extra == 1]] = hub_col
    val = rng.standard_normal(col.size).astype(np.float32)
    return rowptr, col, val


_cache = {}


def _case(dev, D):
    """The graph, x and the two references of width D, made once."""
    if D not in _cache:
        from ragraph_amd import kernels as K

        rowptr, col, val = _csr(1)
        X = np.random.default_rng(D).standard_normal((N_ROWS, D)).astype(np.float32)
        t = tuple(torch.from_numpy(a).to(dev) for a in (rowptr, col, val, X))
        full = {lr: K.spmm_csr(*t, long_rows=lr) for lr in (False, True)}
        _cache[D] = (t, full, torch.from_numpy(cref.spmm_csr(rowptr, col, val, X)).to(dev))
    return _cache[D]


def _poison(dev, nnz, R, D):
    from ragraph_amd import kernels as K

    nbytes = K.N.lib().ragraph_spmm_csr_rows_workspace_bytes(nnz, R, D)
    K._workspace(nbytes, dev).fill_(0xFF)     # (the buffer the next call on this stream is handed)


@pytest.mark.parametrize("long_rows", [False, True])
@pytest.mark.parametrize("D", [64, 128, 256, 8])
def test_rows_match_full_product_and_oracle(dev, D, long_rows):
    from ragraph_amd import kernels as K

    (rowptr, col, val, x), full, oracle = _case(dev, D)
    assert torch.equal(full[long_rows], oracle)
    deg = (rowptr[1:] - rowptr[:-1])[torch.tensor(AT, device=dev)]
    assert deg.tolist() == list(LENGTHS)
    for rows in (ROWS, [2600], [0], ROWS[:3]):          # R = 10 fills no workgroup; R = 1: the hub alone, an empty row alone
        r = torch.tensor(rows, device=dev)
        _poison(dev, col.numel(), r.numel(), D)
        got = K.spmm_csr_rows(rowptr, col, val, x, r, long_rows=long_rows)
        assert got.shape == (len(rows), D)
        assert torch.equal(got, full[long_rows][r]) and torch.equal(got, oracle[r])
    every = torch.randperm(N_ROWS, generator=torch.Generator().manual_seed(D)).to(dev)   # many blocks of requests
    _poison(dev, col.numel(), N_ROWS, D)
    assert torch.equal(K.spmm_csr_rows(rowptr, col, val, x, every, long_rows=long_rows), oracle[every])
    assert K.spmm_csr_rows(rowptr, col, val, x, every[:0], long_rows=long_rows).shape == (0, D)


def test_more_hub_requests_than_the_area_holds(dev):
    """The same 3-block row 40 times: 120 block sums asked of an area of R + nnz / 4096 + 1 < 120.  Requests that find no room
    are walked by their own lanes: the same bits, and the bytes behind the workspace stay as they were."""
    from ragraph_amd import kernels as K

    D = 64
    (rowptr, col, val, x), full, _ = _case(dev, D)
    L = K.N.lib()
    R, nnz = 40, col.numel()
    assert R + nnz // 4096 + 1 < 3 * R
    rows = torch.full((R,), 2600, device=dev)
    nbytes = L.ragraph_spmm_csr_rows_workspace_bytes(nnz, R, D)
    guard = 1 << 16
    buf = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=dev)
    y = torch.empty(R, D, device=dev)
    K.N.check(L.ragraph_spmm_csr_rows_f32(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), N_ROWS, x.data_ptr(), D,
                                          rows.data_ptr(), R, y.data_ptr(), nnz, buf.data_ptr(), nbytes, K._stream()), "rows")
    assert torch.equal(y, full[True][rows])
    assert bool((buf[nbytes:] == 0xA5).all())
    assert torch.equal(K.spmm_csr_rows(rowptr, col, val, x, rows, long_rows=True), y)


def test_one_finish_kernel_with_an_epilogue_and_without(dev):
    """The full product and the row subset finish their hub rows in the same kernel (spmm_long_finish_kernel: a row's block
    sums in block order), one with bias, activation, residual and pre-activation, the other with none of them and the sum
    stored at the request's position.  One small graph, hub rows of two and three blocks, every user against the oracle."""
    from ragraph_amd import kernels as K

    rng = np.random.default_rng(77)
    n, D, hub, hub2, short = 64, 32, 5, 40, 9
    deg = rng.integers(0, 9, n)
    deg[[hub, hub2, short]] = 4097, 2 * 4096 + 3, 7
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    val = rng.standard_normal(col.size).astype(np.float32)
    X = rng.standard_normal((n, D)).astype(np.float32)
    b = rng.standard_normal(D).astype(np.float32)
    Yin = rng.standard_normal((n, D)).astype(np.float32)
    t = tuple(torch.from_numpy(a).to(dev) for a in (rowptr, col, val, X))
    bd, yd = torch.from_numpy(b).to(dev), torch.from_numpy(Yin).to(dev)

    got = K.spmm_csr(*t, bias=bd, act=K.ACT_PRELU, alpha=0.25, beta=0.5, y_in=yd, long_rows=True)
    ref = cref.spmm_csr(rowptr, col, val, X, bias=b, act=2, alpha=0.25, beta=0.5, Y_in=Yin)
    assert np.array_equal(got.cpu().numpy(), ref)

    y, z = K.spmm_csr_prelu_dev(*t, bd, torch.tensor([0.25], device=dev), want_z=True, long_rows=True)
    assert np.array_equal(y.cpu().numpy(), cref.spmm_csr(rowptr, col, val, X, bias=b, act=2, alpha=0.25))
    assert np.array_equal(z.cpu().numpy(), cref.spmm_csr(rowptr, col, val, X, bias=b, act=0))

    rows = [hub, short, hub, n + 3, hub2]                      # n + 3: no such row, an empty one
    want = np.zeros((len(rows), D), dtype=np.float32)
    plain = cref.spmm_csr(rowptr, col, val, X)
    for i, r in enumerate(rows):
        if r < n:
            want[i] = plain[r]
    _poison(dev, col.size, len(rows), D)
    sub = K.spmm_csr_rows(*t, torch.tensor(rows, device=dev), long_rows=True)
    assert np.array_equal(sub.cpu().numpy(), want)


def _grads(g, x0, rows, w):
    from ragraph_amd import autograd as A

    x = x0.clone().requires_grad_(True)
    y = A.spmm_csr_rows(g, x, rows)
    (y * w).sum().backward()
    x2 = x0.clone().requires_grad_(True)
    y2 = A.spmm_csr(g, x2)[rows]
    (y2 * w).sum().backward()
    assert torch.equal(y.detach(), y2.detach())
    return x.grad, x2.grad


def test_gradient_is_the_full_paths_on_short_columns(dev):
    """No column holds more than 4096 entries and the rows are distinct and ascending: both backward chains walk a column's
    requested rows in the same order and differ by fmaf(v, 0, acc) terms only -- the same bits."""
    from ragraph_amd.graph import CSRGraph

    rowptr, col, val = (torch.from_numpy(a).to(dev) for a in _csr(1))
    assert int(torch.bincount(col.long(), minlength=N_ROWS).max()) <= 4096
    g = CSRGraph(rowptr, col, val, N_ROWS)
    torch.manual_seed(2)
    x0 = torch.randn(N_ROWS, 64, device=dev)
    pick = torch.randperm(N_ROWS, generator=torch.Generator().manual_seed(3))[:700]
    rows = torch.cat([pick, torch.tensor(AT)]).unique().to(dev)          # (sorted; test set-up, not the library's path)
    w = torch.randn(rows.numel(), 64, device=dev)
    got, ref = _grads(g, x0, rows, w)
    assert float(got.abs().max()) > 0 and torch.equal(got, ref)


def test_gradient_with_a_hub_column_and_repeated_rows(dev):
    """A column of 9000 entries (its transposed row is cut into 4096-blocks from the full row there, from the subset here) and
    repeated, scrambled rows (summed in another association): the project's tolerance for this step, close(..., 2e-4)."""
    from ragraph_amd.graph import CSRGraph

    rowptr, col, val = (torch.from_numpy(a).to(dev) for a in _csr(4, hub_col=123))
    assert int(torch.bincount(col.long(), minlength=N_ROWS).max()) >= 9000
    g = CSRGraph(rowptr, col, val, N_ROWS)
    torch.manual_seed(5)
    x0 = torch.randn(N_ROWS, 64, device=dev)
    rows = torch.randint(0, N_ROWS, (9500,), generator=torch.Generator().manual_seed(6)).to(dev)
    w = torch.randn(rows.numel(), 64, device=dev)
    got, ref = _grads(g, x0, rows, w)
    err = float((got - ref).abs().max())
    print(f"hub-column gradient: max abs err {err:.3e}, ref max {float(ref.abs().max()):.3e}")
    assert close(got, ref, 2e-4)


def test_call_is_capturable(dev):
    from ragraph_amd import kernels as K

    (rowptr, col, val, x), _, _ = _case(dev, 64)
    rows = torch.tensor(ROWS, device=dev)
    x2 = torch.randn(N_ROWS, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    eager = K.spmm_csr_rows(rowptr, col, val, x2, rows, long_rows=True)
    xs = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.spmm_csr_rows(rowptr, col, val, xs, rows, long_rows=True)      # (warm-up: code objects, the stream's workspace)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = K.spmm_csr_rows(rowptr, col, val, xs, rows, long_rows=True)
    xs.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
