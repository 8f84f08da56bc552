"""Device dense -> CSR (ragraph_dense_to_csr_f32, K.dense_to_csr) and its users: CSRGraph.from_dense / as_csr on device
tensors, sparse_features, both averageemb functions, and a captured forward that takes its adjacency as a DENSE input.

The reference of every comparison is computed here with torch on a CPU copy (nonzero, bincount, cumsum, a[rows, cols]), never
with the code under test; equality is torch.equal on rowptr / col and on val viewed as int32 (the values keep their bits)."""
import contextlib

import numpy as np
import pytest
import torch

from guarded_workspace import GuardedWorkspace

pytestmark = pytest.mark.gpu


def ref_csr(a_cpu: torch.Tensor):
    """The torch construction on a host copy: (rowptr int64, col int32, val fp32)."""
    assert a_cpu.device.type == "cpu" and a_cpu.dim() == 2
    nz = torch.nonzero(a_cpu, as_tuple=False)
    rows, cols = nz[:, 0], nz[:, 1]
    rowptr = torch.zeros(a_cpu.shape[0] + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=a_cpu.shape[0]), 0)
    return rowptr, cols.to(torch.int32), a_cpu[rows, cols].contiguous()


def same_csr(got, want):
    rp, col, val = (t.cpu() for t in got[:3])
    assert rp.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
    assert torch.equal(rp, want[0]), "rowptr differs"
    assert torch.equal(col, want[1]), "col differs"
    assert torch.equal(val.view(torch.int32), want[2].view(torch.int32)), "val bits differ"


@contextlib.contextmanager
def no_sync():
    """A read-back (or any other synchronisation torch knows of) raises inside."""
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode(mode)


def sparse(shape, density, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(shape, generator=g)
    return torch.where(torch.rand(shape, generator=g) < density, v, torch.zeros(shape))


SPECIALS = [-0.0, float("nan"), float("inf"), float("-inf"), 1e-45, -1e-40, 0.0, 1.5]   # -0 / +0 dropped, the rest kept


def with_specials(a):
    flat = a.reshape(-1)
    pos = torch.arange(len(SPECIALS)) * 7 % flat.numel()
    flat[pos] = torch.tensor(SPECIALS)
    flat[-1] = float("nan")
    nan = torch.tensor([0x7FC12345], dtype=torch.int32).view(torch.float32)      # a NaN with a payload
    flat[flat.numel() // 2] = nan[0]
    return a


def _one_full_row():
    a = torch.zeros(3, 4097)
    a[1] = torch.arange(1, 4098, dtype=torch.float32)
    a[2, 4096] = 2.0
    return a


# name -> a function of the device that returns the matrix (a view where the layout is the point)
SHAPES = {
    "0x5": lambda d: torch.zeros(0, 5, device=d),
    "5x0": lambda d: torch.zeros(5, 0, device=d),
    "1x1-zero": lambda d: torch.zeros(1, 1, device=d),
    "1x1-nonzero": lambda d: torch.full((1, 1), -3.0, device=d),
    "5x3": lambda d: sparse((5, 3), 0.5, 1).to(d),
    "64x64-full": lambda d: (torch.arange(64 * 64, dtype=torch.float32).reshape(64, 64) + 1).to(d),
    "65x63": lambda d: sparse((65, 63), 0.3, 2).to(d),
    "7x257": lambda d: sparse((7, 257), 0.2, 3).to(d),
    "3x4097-one-full-row": lambda d: _one_full_row().to(d),
    "300x1433-1.5pct": lambda d: sparse((300, 1433), 0.015, 4).to(d),
    "130x130-all-zero": lambda d: torch.zeros(130, 130, device=d),
    "1x48x48-view": lambda d: sparse((48, 48), 0.2, 5).to(d)[None],
    # 128-bit loads (16-byte aligned base, lda % 4 == 0): whole chunks, a ragged end, more than one trip of the loop
    "9x260-vec": lambda d: sparse((9, 260), 0.2, 6).to(d),
    "6x772-vec": lambda d: sparse((6, 772), 0.1, 7).to(d),
    "2x4096-vec-full": lambda d: (torch.arange(2 * 4096, dtype=torch.float32).reshape(2, 4096) + 1).to(d),
    # lda > cols: a column slice -- off the 16-byte grid (scalar walk), and on it with cols % 4 != 0 (vector walk, ragged end)
    "col-slice-unaligned": lambda d: sparse((20, 300), 0.2, 8).to(d)[:, 5:205],
    "col-slice-aligned-333": lambda d: sparse((11, 600), 0.2, 9).to(d)[:, 4:337],
    "col-slice-narrow": lambda d: sparse((70, 100), 0.3, 10).to(d)[:, 3:50],
    # a base pointer off the 16-byte grid: a row slice starting at an odd offset of a larger buffer
    "row-slice-odd-offset": lambda d: sparse((34, 131), 0.2, 11).to(d)[1:],
    # -0.0 dropped; NaN (with payload), +-inf and denormals kept, with their bits -- in each of the three walks
    "specials-one-chunk": lambda d: with_specials(sparse((3, 40), 0.3, 12)).to(d),
    "specials-vec": lambda d: with_specials(sparse((3, 72), 0.3, 13)).to(d),
    "specials-scalar": lambda d: with_specials(sparse((3, 73), 0.3, 14)).to(d),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_dense_to_csr_matches_the_torch_construction(dev, name):
    from ragraph_amd import kernels as K

    a = SHAPES[name](dev)
    a2 = a[0] if a.dim() == 3 else a
    want = ref_csr(a2.cpu())
    if "specials" in name:
        kept = want[2]
        assert torch.isnan(kept).sum() >= 2 and torch.isinf(kept).sum() == 2 and (kept.abs() < 1e-38).sum() == 2
        assert not ((kept == 0) & ~torch.isnan(kept)).any()
    if name == "row-slice-odd-offset":
        assert a.data_ptr() % 16 != 0
    if name == "col-slice-aligned-333":
        assert a.data_ptr() % 16 == 0 and a.stride(0) % 4 == 0 and a.shape[1] % 4 != 0
    same_csr(K.dense_to_csr(a), want)
    # the capturable form of the same call: capacity = every slot, nothing read back
    cap = a2.shape[0] * a2.shape[1]
    with no_sync():
        rp, col, val, status = K.dense_to_csr(a, capacity=cap)
    nnz = want[1].numel()
    assert col.numel() == cap and val.numel() == cap and status.tolist() == [nnz, 0]
    same_csr((rp, col[:nnz], val[:nnz]), want)


# ---- 2. the capacity form on the C ABI: caller's buffers with a sentinel tail, exact-size guarded workspace -------------------
SENT_I, SENT_F = -77, -1234.5
TAIL = 64


def _raw_call(K, a, capacity, count_only=False, fill=0xFF):
    L = K._ready()
    rows, cols = a.shape
    gw = GuardedWorkspace(fill=fill)
    ws = gw(L.ragraph_dense_to_csr_workspace_bytes(rows, cols), a.device)
    rowptr = torch.full((rows + 1 + TAIL,), SENT_I, dtype=torch.int64, device=a.device)
    status = torch.full((2 + TAIL,), SENT_I, dtype=torch.int64, device=a.device)
    col = torch.full((capacity + TAIL,), SENT_I, dtype=torch.int32, device=a.device)
    val = torch.full((capacity + TAIL,), SENT_F, dtype=torch.float32, device=a.device)
    with no_sync():
        rc = L.ragraph_dense_to_csr_f32(a.data_ptr(), rows, cols, a.stride(0), 0 if count_only else capacity, rowptr.data_ptr(),
                                        None if count_only else col.data_ptr(), None if count_only else val.data_ptr(),
                                        status.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == 0, K.N.last_error()
    assert gw.check() == 1
    assert (rowptr[rows + 1:] == SENT_I).all() and (status[2:] == SENT_I).all()
    return rowptr[:rows + 1].cpu(), col.cpu(), val.cpu(), status[:2].tolist()


@pytest.mark.parametrize("layout", ["scalar", "vec", "one-chunk"])
def test_capacity_form_writes_nothing_behind_the_capacity(dev, layout):
    from ragraph_amd import kernels as K

    shape = {"scalar": (37, 301), "vec": (37, 300), "one-chunk": (90, 61)}[layout]
    a = sparse(shape, 0.1, 21).to(dev)
    want = ref_csr(a.cpu())
    nnz = want[1].numel()
    assert nnz > 200
    for capacity in (nnz, nnz + 100, nnz - 57, 1):
        rp, col, val, status = _raw_call(K, a, capacity)
        kept = min(nnz, capacity)
        assert status == [nnz, 1 if nnz > capacity else 0]
        assert torch.equal(rp, want[0])                                   # the TRUE prefix, whatever the capacity
        assert torch.equal(col[:kept], want[1][:kept])
        assert torch.equal(val[:kept].view(torch.int32), want[2][:kept].view(torch.int32))
        assert (col[kept:] == SENT_I).all() and (val[kept:] == SENT_F).all()   # the unused slots and the tail: untouched
    rp, col, val, status = _raw_call(K, a, 50, count_only=True, fill=0xA5)
    assert status == [nnz, 1] and torch.equal(rp, want[0])               # (count-only: capacity 0, so any entry overflows it)
    assert (col == SENT_I).all() and (val == SENT_F).all()


def test_bad_arguments_are_refused_before_anything_runs(dev):
    from ragraph_amd import kernels as K

    L = K._ready()
    a = torch.ones(4, 8, device=dev)
    i64 = torch.full((16,), SENT_I, dtype=torch.int64, device=dev)
    i32 = torch.full((64,), SENT_I, dtype=torch.int32, device=dev)
    f32 = torch.full((64,), SENT_F, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    call = lambda rows, cols, lda, cap, col, val, ws_bytes=ws.numel(): L.ragraph_dense_to_csr_f32(
        a.data_ptr(), rows, cols, lda, cap, i64.data_ptr(), col, val, i64[8:].data_ptr(), ws.data_ptr(), ws_bytes, None)
    assert call(4, 8, 7, 32, i32.data_ptr(), f32.data_ptr()) == K.N.EINVAL                 # lda < cols
    assert call(-1, 8, 8, 32, i32.data_ptr(), f32.data_ptr()) == K.N.EINVAL
    assert call(1 << 16, 1 << 15, 1 << 15, 32, i32.data_ptr(), f32.data_ptr()) == K.N.EINVAL   # 2^31 elements
    assert K.N.last_error().startswith("dense_to_csr")
    assert call(4, 8, 8, 32, i32.data_ptr(), None) == K.N.EINVAL                           # col without val
    assert call(4, 8, 8, 32, None, None) == K.N.EINVAL                                     # a capacity without buffers
    assert call(4, 8, 8, 32, i32.data_ptr(), f32.data_ptr(), ws_bytes=8) == K.N.EWORKSPACE
    torch.cuda.synchronize()
    assert (i64 == SENT_I).all() and (i32 == SENT_I).all() and (f32 == SENT_F).all()
    with pytest.raises(K.RagraphNativeError, match="float32"):
        K.dense_to_csr(a.double())


# ---- 3. users: CSRGraph.from_dense / as_csr ---------------------------------------------------------------------------------
def sym_normalized(n, seed, active=None, p=0.1):
    """D^-1/2 (A + I) D^-1/2 over the first `active` nodes (fp32, dense); node 7 and the nodes behind `active` are isolated:
    all-zero rows and columns."""
    rng = np.random.default_rng(seed)
    active = n if active is None else active
    a = np.zeros((n, n))
    m = rng.random((active, active)) < p
    a[:active, :active] = (m | m.T) | np.eye(active, dtype=bool)
    a[7, :] = 0
    a[:, 7] = 0
    d = a.sum(1)
    dinv = np.where(d > 0, 1.0 / np.sqrt(np.maximum(d, 1)), 0.0)
    return torch.from_numpy((a * dinv[:, None] * dinv[None, :]).astype(np.float32))


def test_from_dense_and_as_csr_on_device_tensors(dev):
    from ragraph_amd import kernels as K
    from ragraph_amd.graph import CSRGraph, as_csr

    n = 48
    a = sym_normalized(n, 0)
    want = ref_csr(a)
    assert want[0][8] == want[0][7]                                        # the isolated node: an empty row
    ad = a.to(dev)
    for g in (CSRGraph.from_dense(ad), as_csr(ad), as_csr(ad[None])):
        assert g.n == n and not g.padded and g.nnz == want[1].numel()
        same_csr((g.rowptr, g.col, g.val), want)
        assert g._has_long_rows is False                                   # set at construction: n <= ROW_BLOCK
    with no_sync():                                                        # a capacity: no read-back anywhere
        g = CSRGraph.from_dense(ad, capacity=n * n)
        assert g.has_long_rows is False
    assert g.padded and g.nnz == n * n and g.status.tolist() == [want[1].numel(), 0]
    same_csr((g.rowptr, g.col[:want[1].numel()], g.val[:want[1].numel()]), want)
    with pytest.raises(K.RagraphNativeError, match="padded graph is inference-only"):
        g.transposed()
    # the kernels a forward relies on walk the row pointers: the padded graph gives the bits of the exact one
    exact = CSRGraph.from_dense(ad)
    x = torch.randn(n, 32, device=dev)
    assert torch.equal(K.spmm_csr(g.rowptr, g.col, g.val, x), K.spmm_csr(exact.rowptr, exact.col, exact.val, x))
    m = want[1].numel()
    assert torch.equal(g.row_normalized_values()[:m], exact.row_normalized_values())


# ---- 4. sparse_features -----------------------------------------------------------------------------------------------------
def test_sparse_features_through_the_library(dev):
    from ragraph_amd.layers.gcn import sparse_features

    x = torch.where(torch.rand(300, 512, generator=torch.Generator().manual_seed(1)) < 0.02,
                    torch.randn(300, 512, generator=torch.Generator().manual_seed(2)), torch.zeros(300, 512))
    xs = x.to_sparse_csr()
    got = sparse_features(x.to(dev))
    assert got is not None
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
    assert torch.equal(got[0].cpu(), xs.crow_indices()) and torch.equal(got[1].cpu(), xs.col_indices().to(torch.int32))
    assert torch.equal(got[2].cpu().view(torch.int32), xs.values().view(torch.int32))
    dense = torch.where(torch.rand(300, 512, generator=torch.Generator().manual_seed(3)) < 0.10, torch.ones(300, 512),
                        torch.zeros(300, 512))
    assert sparse_features(dense.to(dev)) is None


# ---- 5. both averageemb functions against the parent's torch chain, restated ------------------------------------------------
def _labels(dev):
    lab = torch.tensor([0, 1, 2, 1, 0, 2, 2, 1, 0, 0, 5, -1, 1, 2, 0, 1, 3, 2, 1, 0,
                        2, 2, 1, 0, 1, 7, 0, 2, 1, 0, 1, 2, -3, 0, 1, 2, 0, 1, 2, 1])
    assert lab.numel() == 40
    return lab.to(dev)


def test_node_averageemb_equals_the_torch_chain(dev):
    from ragraph_amd import autograd as AG
    from ragraph_amd import downprompt_node as dn

    lab = _labels(dev)
    raw = torch.randn(40, 24, device=dev, generator=torch.Generator(device=dev).manual_seed(0))

    def parent(rawret):
        n, half = 40, 20
        keep = (lab >= 0) & (lab < 3)
        lab_k = lab[keep]
        counts = torch.bincount(lab_k, minlength=3)
        assert int(counts.max()) <= half
        order = torch.nonzero(keep).reshape(-1)[torch.sort(lab_k, stable=True).indices]
        seg = torch.zeros(4, dtype=torch.int64, device=dev)
        seg[1:] = torch.cumsum(counts, 0)
        sums = AG.segment_sum(AG.gather_rows(rawret, order), seg)
        return AG.mul_cols(sums, torch.full((rawret.shape[1],), 1.0 / half, device=dev))

    with torch.no_grad():
        assert torch.equal(dn.averageemb(lab, raw), parent(raw))
    w = torch.randn(3, 24, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    grads = []
    for fn in (lambda r: dn.averageemb(lab, r), parent):
        r = raw.clone().requires_grad_(True)
        out = fn(r)
        (out * w).sum().backward()
        grads.append((out.detach(), r.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert (grads[0][1][torch.tensor([10, 11, 16, 25, 32], device=dev)] == 0).all()     # rows of other labels: skipped
    crowded = torch.zeros(40, dtype=torch.int64, device=dev)
    crowded[:19] = 1                                                                    # class 0 holds 21 > int(40 / 2) rows
    with pytest.raises(IndexError, match="21 rows"):
        dn.averageemb(crowded, raw)
    with pytest.raises(IndexError):
        dn.averageemb(lab[:1], raw[:1])


def test_graph_averageemb_equals_the_torch_chain(dev):
    from ragraph_amd import downprompt as dg
    from ragraph_amd import kernels as K

    lab_all = _labels(dev)
    inside = (lab_all >= 0) & (lab_all < 3)
    lab = torch.where(inside, lab_all, torch.ones_like(lab_all))       # (the parent's bincount refuses labels outside the classes)
    raw = torch.randn(40, 100, device=dev, generator=torch.Generator(device=dev).manual_seed(2))

    def parent(labels, nb_class):
        order = torch.sort(labels, stable=True).indices
        counts = torch.bincount(labels, minlength=nb_class)
        seg = torch.zeros(nb_class + 1, dtype=torch.int64, device=dev)
        seg[1:] = torch.cumsum(counts, 0)
        out = K.segment_reduce(K.gather_rows(raw, order), seg, mean_mode=True)
        out[counts == 0] = 0
        return out

    assert torch.equal(dg.averageemb(lab, raw, 3), parent(lab, 3))
    got5 = dg.averageemb(lab, raw, 5)                                   # classes 3 and 4 are empty: zero rows, no NaN
    assert torch.equal(got5, parent(lab, 5)) and (got5[3:] == 0).all()
    # labels outside the classes are ignored now (the parent raised on them): the in-range rows give the same means
    rows_in = torch.nonzero(inside).reshape(-1)[torch.sort(lab_all[inside], stable=True).indices]
    seg = torch.zeros(4, dtype=torch.int64, device=dev)
    seg[1:] = torch.cumsum(torch.bincount(lab_all[inside], minlength=3), 0)
    assert torch.equal(dg.averageemb(lab_all, raw, 3), K.segment_reduce(K.gather_rows(raw, rows_in), seg, mean_mode=True))


# ---- 6. capture: the adjacency is a captured input, in dense form -----------------------------------------------------------
N_NODES, F_IN, D_EMB, BANK = 48, 32, 256, 256


def _model(dev, flavour):
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph import RAGraph, RAGraphGraph

    torch.manual_seed(0)
    C = 3 if flavour == "node" else 2
    pre = PrePrompt(F_IN, D_EMB, "prelu", 1, 0.3).to(dev)
    model = (RAGraph if flavour == "node" else RAGraphGraph)(pre, None, F_IN, C, D_EMB, device=dev).eval()
    model.toy_graph_base.add_resources(torch.nn.functional.normalize(torch.randn(BANK, D_EMB, device=dev), dim=-1),
                                       torch.randn(BANK, D_EMB, device=dev),
                                       torch.nn.functional.one_hot(torch.randint(0, C, (BANK,), device=dev), C).float())
    return model


@pytest.mark.parametrize("flavour", ["node", "graph"])
def test_captured_forward_takes_a_dense_adjacency_input(dev, flavour):
    from ragraph_amd.capture import CapturedForward
    from ragraph_amd.graph import CSRGraph

    model = _model(dev, flavour)
    feats = torch.randn(N_NODES, F_IN, device=dev)
    adj1 = sym_normalized(N_NODES, 1).to(dev)
    adj2 = sym_normalized(N_NODES, 2, active=N_NODES - 8, p=0.2).to(dev)     # another pattern; the last 8 nodes are padding
    assert (adj2[-8:] == 0).all() and (adj2[:, -8:] == 0).all()
    assert int((adj1 != 0).sum()) != int((adj2 != 0).sum())
    assert not torch.equal((adj1 != 0)[:40, :40], (adj2 != 0)[:40, :40])
    fwd = CapturedForward(lambda x, a: model(x, a), feats, adj1)
    with torch.no_grad():
        want2 = model(feats, CSRGraph.from_dense(adj2))
        want1 = model(feats, CSRGraph.from_dense(adj1))
    assert not torch.equal(want1, want2)
    assert torch.equal(fwd(feats, adj2).clone(), want2)
    assert torch.equal(fwd(feats, adj1).clone(), want1)
    feats2 = torch.randn(N_NODES, F_IN, device=dev)
    with torch.no_grad():
        want3 = model(feats2, CSRGraph.from_dense(adj2))
    assert torch.equal(fwd(feats2, adj2), want3)


def test_a_large_dense_adjacency_is_refused_under_capture(dev):
    from ragraph_amd import kernels as K
    from ragraph_amd.graph import CSRGraph, as_csr

    small = sym_normalized(N_NODES, 3).to(dev)
    big = torch.zeros(K.ROW_BLOCK + 1, K.ROW_BLOCK + 1, device=dev)
    big.fill_diagonal_(1.0)
    CSRGraph.from_dense(small, capacity=N_NODES * N_NODES)                # (warm-up: workspace)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        CSRGraph.from_dense(small, capacity=N_NODES * N_NODES)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            with torch.no_grad():
                g = as_csr(small)
                with pytest.raises(K.RagraphNativeError, match=str(K.ROW_BLOCK)):
                    as_csr(big)
            with pytest.raises(K.RagraphNativeError, match="padded graph is inference-only"):
                as_csr(small)                                             # (with gradients enabled: a training step)
        graph.replay()
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert g.padded and g._has_long_rows is False
    want = ref_csr(small.cpu())
    m = want[1].numel()
    assert g.status.tolist() == [m, 0]
    same_csr((g.rowptr, g.col[:m], g.val[:m]), want)
    eager = CSRGraph.from_dense(big)                                       # outside a capture the large one converts
    assert eager.nnz == K.ROW_BLOCK + 1 and eager._has_long_rows is None and eager.has_long_rows is False
