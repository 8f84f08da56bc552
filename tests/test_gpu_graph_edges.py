"""The graph-analytic kernels at the shapes on each side of every block and stride edge, on DIRECTED graphs: dense
Floyd-Warshall and position_code (rows.hip, 256 columns / outputs per block), the batched LDS kernel (bank.hip, 256 threads
over n * n slots, n <= 64), the two CSR routes at the LDS kernel's 1024-thread stride, and PageRank, sample_prob and the CSR
row sums (bank.hip, reductions strided by 256 per graph).

Every result is held to two references: the C oracle bit for bit (oracle/cref.py restates the kernels' operation order),
and the independent float64 references of tests/graph_reference.py -- equality on lattice graphs, a derived bound otherwise.
tests/test_cpu_graph_reference.py proves the same float64 statements of the oracle for these very cases, without a GPU.
Every call runs twice and must give the same bits."""
import numpy as np
import pytest
import torch

import graph_reference as R
from oracle import cref

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def twice(fn):
    """fn() twice: the same bits both times; the first result as numpy (a tuple stays a tuple)."""
    a, b = fn(), fn()
    one = not isinstance(a, tuple)
    a, b = ((a,), (b,)) if one else (a, b)
    a, b = [x.cpu().numpy() for x in a], [x.cpu().numpy() for x in b]
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "two runs of the same call differ"
    return a[0] if one else tuple(a)


def same_bits_or_nan(a, b):
    """fp32 bit equality where neither side is NaN, and NaN in the same places (0/0 on the host and on the device may differ
    in the NaN's sign bit: that is no property of the operation)."""
    a, b = R.f32(a), R.f32(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32))


# ---- (a) dense all-pairs: floyd_warshall, then position_code ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "real"])
@pytest.mark.parametrize("n", R.DENSE_SIZES)
def test_dense_floyd_warshall_and_position_code(dev, n, kind):
    from ragraph_amd import kernels as K

    adj, dist64, _ = R.dense_case(n, kind)
    a = T(adj, dev)
    fw = twice(lambda: K.floyd_warshall(a))
    assert R.same_bits(fw, cref.floyd_warshall(adj)), "device Floyd-Warshall differs from the oracle"
    err = R.check_paths(fw, dist64, kind)          # lattice: equal to float64 Dijkstra; real: same infinities, (n - 1) u
    print(f"dense n={n} {kind}: {err:.2f} u")
    d_dev = T(fw, dev)
    for A in R.DENSE_ANCHOR_COUNTS:
        anchors = R.dense_anchors(n, A)
        an = T(anchors, dev)
        for dis_q in R.DIS_QS:
            codes = twice(lambda: K.position_code(d_dev, an, dis_q))
            assert R.same_bits(codes, cref.position_code(fw, anchors, dis_q)), (A, dis_q)
            if kind == "lattice":
                assert R.same_bits(codes, R.position_code64(dist64, anchors, dis_q)), (A, dis_q)


# ---- (b) batched: one workgroup per graph ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "real"])
@pytest.mark.parametrize("n,G", R.BATCH_CASES)
def test_batch_position_codes(dev, n, G, kind):
    from ragraph_amd import kernels as K

    adj, dist64, _ = R.batch_case(n, G, kind)
    a = T(adj, dev)
    fw_ref = np.stack([cref.floyd_warshall(adj[g]) for g in range(G)])
    dense_route = {g: K.floyd_warshall(a[g]) for g in sorted({0, G // 2, G - 1})}      # (a)'s route on the same matrices
    for A in R.BATCH_ANCHOR_COUNTS:
        anchors = R.batch_anchors(n, G, A)        # every graph its own anchors: a wrong graph stride cannot pass
        an = T(anchors, dev)
        for dis_q in R.DIS_QS:
            codes, dist = twice(lambda: K.position_codes_batch(a, an, dis_q, return_dist=True))
            only = twice(lambda: K.position_codes_batch(a, an, dis_q))
            assert R.same_bits(only, codes), "the call without dist gives other codes"
            assert R.same_bits(dist, fw_ref), "batched distances differ from the oracle"
            R.check_paths(dist, dist64, kind)
            want = np.stack([cref.position_code(fw_ref[g], anchors[g], dis_q) for g in range(G)])
            assert R.same_bits(codes, want), (A, dis_q)
            if kind == "lattice":
                assert R.same_bits(codes, R.position_code64(dist64, anchors, dis_q)), (A, dis_q)
            for g, d_g in dense_route.items():
                assert R.same_bits(dist[g], d_g.cpu().numpy())
                assert R.same_bits(codes[g], K.position_code(d_g, an[g], dis_q).cpu().numpy())


# ---- (c) CSR routes: the LDS kernel (1024 threads stride over the nodes) and the global path ------------------------------------
@pytest.mark.parametrize("n", R.CSR_SIZES)
def test_csr_routes_at_the_lds_stride(dev, n):
    from ragraph_amd import kernels as K

    _, (rowptr, col, val) = R.csr_case(n, "lattice")        # explicit zero entries and self-loops are stored
    rp, c, v = T(rowptr, dev), T(col, dev), T(val, dev)
    for A in R.CSR_ANCHOR_COUNTS:
        anchors = R.csr_anchors(n, A)                        # A >= 2: the last anchor duplicates the first
        an = T(anchors, dev)
        d64 = R.anchor_dists64(rowptr, col, val, anchors)
        for dis_q in R.CSR_DIS_QS:
            o_codes, o_dist = cref.position_codes_csr(rowptr, col, val, anchors, dis_q)
            for method in (None, "global"):
                codes, dist = twice(lambda: K.position_codes_csr(rp, c, v, an, dis_q, return_dist=True, method=method))
                R.check_paths(dist, d64, "lattice")
                assert R.same_bits(dist, o_dist) and R.same_bits(codes, o_codes), (A, dis_q, method)
                assert R.same_bits(codes, R.position_code64(d64, None, dis_q)), (A, dis_q, method)
                assert R.same_bits(K.position_codes_csr(rp, c, v, an, dis_q, method=method).cpu().numpy(), codes)


def test_csr_real_weights_within_path_bound(dev):
    from ragraph_amd import kernels as K

    n = 257
    _, (rowptr, col, val) = R.csr_case(n, "real")
    anchors = R.csr_anchors(n, 17)
    o_codes, o_dist = cref.position_codes_csr(rowptr, col, val, anchors, 10.0)
    d64 = R.anchor_dists64(rowptr, col, val, anchors)
    for method in (None, "global"):
        codes, dist = twice(lambda: K.position_codes_csr(T(rowptr, dev), T(col, dev), T(val, dev), T(anchors, dev), 10.0,
                                                         return_dist=True, method=method))
        assert R.same_bits(dist, o_dist) and R.same_bits(codes, o_codes)
        R.check_paths(dist, d64, "real")


@pytest.mark.parametrize("n", R.CROSS_SIZES)
def test_four_routes_agree_on_one_graph(dev, n):
    """Dense Floyd-Warshall, the batched LDS kernel, the CSR LDS kernel and the CSR global path on the same lattice graph: the
    same distances to the anchors (the anchors' columns of the all-pairs matrix) and the same codes, all equal to float64."""
    from ragraph_amd import kernels as K

    adj, (rowptr, col, val) = R.csr_case(n, "lattice")
    a = T(adj, dev)
    for A in (1, 17):
        anchors = R.csr_anchors(n, A)
        an = T(anchors, dev)
        d64 = R.anchor_dists64(rowptr, col, val, anchors)
        for dis_q in R.CSR_DIS_QS:
            want = R.position_code64(d64, None, dis_q)
            fw = K.floyd_warshall(a)
            b_codes, b_dist = K.position_codes_batch(a[None], an[None], dis_q, return_dist=True)
            routes = {"dense": (K.position_code(fw, an, dis_q), fw[:, an]),
                      "batch": (b_codes[0], b_dist[0][:, an]),
                      "lds": K.position_codes_csr(T(rowptr, dev), T(col, dev), T(val, dev), an, dis_q, return_dist=True),
                      "global": K.position_codes_csr(T(rowptr, dev), T(col, dev), T(val, dev), an, dis_q, return_dist=True,
                                                     method="global")}
            for name, (codes, dist) in routes.items():
                assert np.array_equal(dist.cpu().numpy(), R.f32(d64)), (name, A, dis_q)
                assert R.same_bits(codes.cpu().numpy(), want), (name, A, dis_q)


# ---- (d) PageRank --------------------------------------------------------------------------------------------------------------
def _pagerank_inputs(dev, which="pagerank"):
    from ragraph_amd import kernels as K

    _, gp, (rowptr, _, val), (rt, ct, vt) = R.pagerank_case(which)
    out_deg = K.csr_row_sums(T(rowptr, dev), T(val, dev))
    assert R.same_bits(out_deg.cpu().numpy(), cref.csr_row_sums(rowptr, val))
    return gp, (rt, ct, vt), (T(rt, dev), T(ct, dev), T(vt, dev), out_deg, T(gp, dev))


@pytest.mark.parametrize("d", R.PAGERANK_DS)
@pytest.mark.parametrize("max_iter", R.PAGERANK_MAX_ITERS)
def test_pagerank_bits_and_float64(dev, max_iter, d):
    """Sizes 1 (self-loop), 1 (dangling), 2, 0, 255, 256, 257, 513, 1025, 40 (all rows zero), 0 in one batch; the empty graphs
    are legal (no node, no iteration).  The iteration COUNT is pinned by the oracle's bits only: a float64 run may stop one
    iteration earlier or later at the eps edge."""
    from ragraph_amd import kernels as K

    gp, (rt, ct, vt), args = _pagerank_inputs(dev)
    p, iters = twice(lambda: K.pagerank(*args, d=d, eps=R.PAGERANK_EPS, max_iter=max_iter))
    out_deg = args[3].cpu().numpy()
    p_ref, it_ref = cref.pagerank(rt, ct, vt, out_deg, gp, d=d, eps=R.PAGERANK_EPS, max_iter=max_iter)
    assert np.array_equal(iters, it_ref) and R.same_bits(p, p_ref)
    if max_iter == 1:
        print(f"one update d={d}: worst error / bound = {R.check_pagerank_step(p, 'pagerank', d):.3f}")
    if max_iter == 128:
        l1, ratio = R.check_pagerank_converged(p, iters, "pagerank", d, R.PAGERANK_EPS, max_iter)
        print(f"converged d={d}: worst L1 = {l1:.3e}, worst error / bound = {ratio:.3f}")
        zero = slice(int(gp[9]), int(gp[10]))          # every row zero: the uniform vector is the fixpoint, kept at once
        assert iters[9] == 0 and R.same_bits(p[zero], np.full(40, np.float32(1) / np.float32(40)))


def test_pagerank_runs_every_iteration_at_eps_zero(dev):
    from ragraph_amd import kernels as K

    gp, (rt, ct, vt), args = _pagerank_inputs(dev)
    p, iters = twice(lambda: K.pagerank(*args, d=0.85, eps=0.0, max_iter=5))
    assert np.array_equal(iters, np.where(np.diff(gp) > 0, 5, 0))
    p_ref, it_ref = cref.pagerank(rt, ct, vt, args[3].cpu().numpy(), gp, d=0.85, eps=0.0, max_iter=5)
    assert np.array_equal(iters, it_ref) and R.same_bits(p, p_ref)


# ---- (e) sample_prob as a pure function -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", R.SAMPLE_ALPHAS)
def test_sample_prob_pure_function(dev, alpha):
    """Random positive p and col_sum on the sizes of (d).  A one-node graph divides by N - 1 = 0: the result there is NaN, on
    the device, in the oracle and in the float64 restatement alike -- pinned here, not endorsed."""
    from ragraph_amd import kernels as K

    _, gp, _, _ = R.pagerank_case("pagerank")
    p, c = R.sample_inputs(gp)
    prob = twice(lambda: K.sample_prob(T(p, dev), T(c, dev), T(gp, dev), alpha, R.SAMPLE_EPS))
    assert same_bits_or_nan(prob, cref.sample_prob(p, c, gp, alpha, R.SAMPLE_EPS))
    worst = R.check_sample_prob(prob, p, c, gp, alpha, R.SAMPLE_EPS)
    assert np.isnan(prob[:2]).all() and not np.isnan(prob[2:]).any()
    print(f"sample_prob alpha={alpha}: worst error / bound = {worst:.3f}")


# ---- (f) csr_row_sums -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "real"])
@pytest.mark.parametrize("n", R.ROW_SUM_SIZES)
def test_csr_row_sums(dev, n, kind):
    from ragraph_amd import kernels as K

    rowptr, val = R.row_sum_case(n, kind)          # empty rows, short rows and one row of 5000 entries
    out = twice(lambda: K.csr_row_sums(T(rowptr, dev), T(val, dev)))
    assert R.same_bits(out, cref.csr_row_sums(rowptr, val))
    R.check_row_sums(out, rowptr, val, kind)


# ---- (g) compute_sample_prob end to end -------------------------------------------------------------------------------------------
def test_compute_sample_prob_end_to_end(dev):
    """bank_build.compute_sample_prob on the batch of (d) without the empty and the one-node graphs: equal to the composition
    of the kernels of (d) to (f), equal to the oracle's composition, and within graph_reference.pipeline_bound of the float64
    pipeline.  The propagation: importance = alpha p + (1 - alpha) c / (N - 1) is LINEAR in the PageRank vector p, so an error
    dp with ||dp||_1 <= pagerank_l1_bound moves it by at most alpha * that bound, its inverse by the relative amount
    rho = alpha * bound / (least importance + eps) (plus the rounding of the column sums), and the normalised probability
    by at most twice rho / (1 - rho); sample_prob's own rounding, sample_prob_bound, comes on top."""
    from ragraph_amd import kernels as K
    from ragraph_amd.bank_build import compute_sample_prob
    from ragraph_amd.graph import CSRGraph

    _, gp, (rowptr, col, val), (rt, ct, vt) = R.pagerank_case("pipeline")
    n = int(gp[-1])
    gpd = T(gp, dev)
    prob = twice(lambda: compute_sample_prob(CSRGraph(T(rowptr, dev), T(col, dev), T(val, dev), n), gpd))
    out_deg = K.csr_row_sums(T(rowptr, dev), T(val, dev))
    p, iters = K.pagerank(T(rt, dev), T(ct, dev), T(vt, dev), out_deg, gpd)
    composed = K.sample_prob(p, K.csr_row_sums(T(rt, dev), T(vt, dev)), gpd)
    assert int(iters.max()) < 128 and R.same_bits(prob, composed.cpu().numpy())
    p_ref, _ = cref.pagerank(rt, ct, vt, cref.csr_row_sums(rowptr, val), gp)
    assert R.same_bits(prob, cref.sample_prob(p_ref, cref.csr_row_sums(rt, vt), gp))
    print(f"compute_sample_prob: worst error / bound = {R.check_pipeline(prob):.3f}")


# ---- the wrappers' shape checks: an error before any launch, not a read outside the tensor ------------------------------------------
def _raises(fn):
    from ragraph_amd.kernels import RagraphNativeError

    with pytest.raises(RagraphNativeError):
        fn()


def test_floyd_warshall_rejects_a_matrix_that_is_not_square(dev):
    from ragraph_amd import kernels as K

    _raises(lambda: K.floyd_warshall(torch.zeros(3, 4, device=dev)))
    _raises(lambda: K.floyd_warshall(torch.zeros(9, device=dev)))
    _raises(lambda: K.floyd_warshall(torch.zeros(1, 3, 3, device=dev)))


def test_position_code_rejects_bad_shapes(dev):
    from ragraph_amd import kernels as K

    anchors = torch.zeros(2, dtype=torch.int64, device=dev)
    _raises(lambda: K.position_code(torch.zeros(3, 4, device=dev), anchors))
    _raises(lambda: K.position_code(torch.zeros(9, device=dev), anchors))
    _raises(lambda: K.position_code(torch.zeros(3, 3, device=dev), anchors.reshape(1, 2)))
    _raises(lambda: K.position_code(torch.zeros(3, 3, device=dev), anchors[:0]))


def test_position_codes_batch_rejects_bad_shapes(dev):
    from ragraph_amd import kernels as K

    anchors = torch.zeros((2, 5), dtype=torch.int64, device=dev)
    _raises(lambda: K.position_codes_batch(torch.zeros(4, 4, device=dev), anchors))
    _raises(lambda: K.position_codes_batch(torch.zeros(2, 3, 4, device=dev), anchors))
    _raises(lambda: K.position_codes_batch(torch.zeros(2, 4, 4, device=dev), anchors[0]))
    _raises(lambda: K.position_codes_batch(torch.zeros(3, 4, 4, device=dev), anchors))


def test_pagerank_rejects_out_deg_of_another_length(dev):
    from ragraph_amd import kernels as K

    rowptr_t = torch.tensor([0, 1, 2, 2], dtype=torch.int64, device=dev)
    col_t = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    val_t = torch.ones(2, device=dev)
    gp = torch.tensor([0, 3], dtype=torch.int64, device=dev)
    _raises(lambda: K.pagerank(rowptr_t, col_t, val_t, torch.ones(4, device=dev), gp))
    _raises(lambda: K.pagerank(rowptr_t, col_t, val_t, torch.ones(2, device=dev), gp))
