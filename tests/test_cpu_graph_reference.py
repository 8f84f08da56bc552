"""tests/graph_reference.py without a GPU: the float64 references on hand-computed graphs, and -- for EVERY shape and seed
tests/test_gpu_graph_edges.py runs -- the C oracle (oracle/cref.py) against them under the rule the device is held to
(equality on lattice graphs, a derived bound otherwise).  The device is compared with the oracle bit for bit, so "the
oracle computes the operation" is what is proved here.  The cases are also shown not to be vacuous, from the reference's
output alone.  Every test prints the figures it measured (pytest -s)."""
import numpy as np
import pytest

import graph_reference as R
from oracle import cref

INF = float("inf")


# ---- hand-computed cases ------------------------------------------------------------------------------------------------
# A directed triangle 0 -> 1 -> 2 -> 0 (lengths 1, 2, 4) whose reverse distances differ, a self-loop at 1 (ignored), and
# node 3 with the single edge 3 -> 0: nothing reaches 3.
HAND = np.array([[0, 1, 0, 0],
                 [0, 0.25, 2, 0],
                 [4, 0, 0, 0],
                 [0.5, 0, 0, 0]], dtype=np.float32)
HAND_DIST = np.array([[0, 1, 3, INF],
                      [6, 0, 2, INF],
                      [4, 5, 0, INF],
                      [0.5, 1.5, 3.5, 0]])


def test_shortest_paths_hand_computed():
    dist, hops = R.shortest_paths64(HAND, return_hops=True)
    assert np.array_equal(dist, HAND_DIST)
    assert dist[0, 2] != dist[2, 0] and dist[0, 1] != dist[1, 0]             # directed: the reverse distances differ
    assert np.array_equal(hops, [[0, 1, 2, 0], [2, 0, 1, 0], [1, 2, 0, 0], [1, 2, 3, 0]])
    assert np.array_equal(R.shortest_paths64(np.stack([HAND, HAND.T]))[1], HAND_DIST.T)     # a stack; the transpose reverses
    assert np.array_equal(R.shortest_paths64(np.zeros((1, 1))), [[0.0]])
    assert np.array_equal(cref.floyd_warshall(HAND), HAND_DIST.astype(np.float32))


def test_anchor_dists_hand_computed():
    # the same graph as a CSR with an explicit zero entry (0 -> 3), the self-loop, and a parallel, longer edge 2 -> 0
    rowptr = np.array([0, 2, 4, 6, 7])
    col = np.array([1, 3, 1, 2, 0, 0, 0])
    val = np.array([1, 0, 0.25, 2, 9, 4, 0.5], dtype=np.float32)
    anchors = np.array([2, 3, 0, 2])
    d = R.anchor_dists64(rowptr, col, val, anchors)
    assert np.array_equal(d, HAND_DIST[:, anchors])
    codes, dist = cref.position_codes_csr(rowptr, col, val, anchors, 3.0)
    assert np.array_equal(dist, d.astype(np.float32)) and np.array_equal(codes, R.position_code64(d, None, 3.0))


def test_position_code_hand_computed():
    # anchor 2 at dis_q = 3: dist[0][2] = 3 is EQUAL to dis_q -> 0 (strict), 2 -> 1/3, 0 -> 1, 3.5 -> 0; anchor 3: unreachable
    third = np.float32(1) / np.float32(3)
    want = np.array([[0, 0], [third, 0], [1, 0], [0, 1]], dtype=np.float32)
    assert np.array_equal(R.position_code64(HAND_DIST, [2, 3], 3.0), want)
    assert np.array_equal(R.position_code64(HAND_DIST[:, [2, 3]], None, 3.0), want)
    assert np.array_equal(R.position_code64(HAND_DIST[None], [[2, 3]], 3.0)[0], want)
    assert np.array_equal(cref.position_code(HAND_DIST.astype(np.float32), np.array([2, 3]), 3.0), want)
    just_above = np.nextafter(np.float32(3), np.float32(4))
    assert R.position_code64(HAND_DIST, [2], just_above)[0, 0] == np.float32(0.25)
    assert np.array_equal(R.position_code64(HAND_DIST, [3], INF)[:, 0], [0, 0, 0, 1])      # inf < inf is false


def test_pagerank_hand_computed():
    # 0 -> 1, 0 -> 2, 1 -> 2; node 2 is dangling; d = 0.5.  One update from (1/3, 1/3, 1/3): (2/9, 11/36, 17/36); the fixpoint
    # solves pi = 1/6 + (P^T pi + pi_2 / 3) / 2: (8, 10, 15) / 33.  Beside it: a one-node dangling graph and an empty one.
    adj = np.zeros((4, 4), dtype=np.float32)
    adj[0, 1] = adj[0, 2] = adj[1, 2] = 1
    gp = np.array([0, 3, 3, 4])
    assert np.allclose(R.pagerank64_steps(adj, gp, 0.5, 0), [1 / 3, 1 / 3, 1 / 3, 1], rtol=0, atol=1e-16)
    assert np.allclose(R.pagerank64_steps(adj, gp, 0.5, 1), [2 / 9, 11 / 36, 17 / 36, 1], rtol=0, atol=1e-15)
    assert np.allclose(R.pagerank64_fixpoint(adj, gp, 0.5), [8 / 33, 10 / 33, 15 / 33, 1], rtol=0, atol=1e-14)
    it = R.pagerank64_stop_iters(adj, gp, 0.5, 1e-6)
    assert 3 <= it[0] < 128 and it[1] == 0 and it[2] == 0
    # dropping the dangling term loses mass: the reference does not
    assert abs(R.pagerank64_fixpoint(adj, gp, 0.5)[:3].sum() - 1) < 1e-14
    rt, ct, vt = cref.dense_to_csr_t(adj)
    p, iters = cref.pagerank(rt, ct, vt, adj.sum(1), gp, d=0.5, eps=1e-6, max_iter=128)
    assert np.abs(p[:3] - np.array([8, 10, 15]) / 33).sum() < R.pagerank_l1_bound(1e-6, 0.5, 2, 3) and iters[1] == 0


def test_sample_prob_and_row_sums_hand_computed():
    # importance = 0.5 p + 0.5 c / 2 = (1/8, 5/8, 5/4): inverses (8, 8/5, 4/5), total 52/5: (10, 2, 1) / 13
    p, c = np.array([0.25, 0.25, 0.5], dtype=np.float32), np.array([0, 2, 4], dtype=np.float32)
    got = R.sample_prob64(p, c, np.array([0, 3]), 0.5, 0.0)
    assert np.allclose(got, np.array([10, 2, 1]) / 13, rtol=0, atol=1e-15)
    wrong = 1 / np.array([1 / 8, 11 / 24, 11 / 12])              # N instead of N - 1 in the degree centrality
    assert np.abs(got - wrong / wrong.sum()).max() > 1e-2
    one = R.sample_prob64(np.array([1.0, 1.0]), np.array([2.0, 0.0]), np.array([0, 1, 2]), 1.0, 1e-6)
    assert np.isnan(one).all()                                  # one-node graphs: N - 1 = 0
    assert np.array_equal(R.row_sums64([0, 0, 3, 4], [1.5, -2, 4, 8]), [0, 3.5, 8])
    assert R.row_sum_bound(1, 5.0) == 0 and R.row_sum_bound(0, 0.0) == 0 and R.row_sum_bound(3, 2.0) == 4 * R.U


def test_generators_are_directed_and_on_the_lattice():
    for n in (25, 257):
        a = R.lattice_graph(n, 5)
        assert not np.array_equal(a, a.T) and np.array_equal(a * 64, np.round(a * 64)) and a.max() <= 4 and a.min() >= 0
        assert (np.diag(a) != 0).any()                           # self-loops are there to be ignored
        r = R.real_graph(n, 5)
        assert not np.array_equal(r, r.T) and r[r != 0].min() >= 0.05 and r.max() <= 3
        assert 2.5 <= (a != 0).sum() / n <= 5
    adj, gp = R.graph_batch(R.PAGERANK_SPEC, R.PAGERANK_SEED)
    assert np.array_equal(np.diff(gp), [1, 1, 2, 0, 255, 256, 257, 513, 1025, 40, 0])
    for g, (lo, hi) in enumerate(zip(gp[:-1], gp[1:])):
        b = adj[lo:hi, lo:hi]
        nz = np.count_nonzero(b)
        assert np.count_nonzero(adj[lo:hi]) == nz and np.count_nonzero(adj[:, lo:hi]) == nz       # block-diagonal
        if hi - lo >= 3:
            assert (b.sum(1) == 0).any(), f"graph {g} has no dangling node"
            assert (b != 0).sum(1).max() <= 4
        if hi - lo > 40:
            assert not np.array_equal(b, b.T)
            assert np.isin(b, [0, 1]).all() == (g % 2 == 0)
    assert adj[0, 0] == 1 and adj[1, 1] == 0 and not adj[gp[9]:gp[10]].any()


# ---- (a) dense all-pairs ---------------------------------------------------------------------------------------------------
def _vacuity_paths(dist, hops):
    """n >= 16: unreachable pairs, finite pairs, and at least a quarter of the finite pairs at >= 3 hops."""
    n = dist.shape[-1]
    if n < 16:
        return
    for d, h in zip(dist.reshape(-1, n, n), hops.reshape(-1, n, n)):
        fin = np.isfinite(d) & ~np.eye(n, dtype=bool)
        assert (~np.isfinite(d)).any() and fin.any() and (h[fin] >= 3).mean() >= 0.25


def _vacuity_dis_q(d, dis_q):
    """The distances the codes read: below dis_q, above it, infinite -- and EQUAL to it: the lattice's planted chain hits
    2.0 and 10.0 exactly (no distance is above inf or, among the finite ones, equal to it)."""
    fin = np.isfinite(d)
    assert (~fin).any() and (d < dis_q).any()
    if dis_q != INF:
        assert (fin & (d > dis_q)).any()
        assert (d == dis_q).any()


@pytest.mark.parametrize("kind", ["lattice", "real"])
@pytest.mark.parametrize("n", R.DENSE_SIZES)
def test_oracle_dense_paths_and_codes(n, kind):
    adj, dist, hops = R.dense_case(n, kind)
    _vacuity_paths(dist, hops)
    fw = cref.floyd_warshall(adj)
    err = R.check_paths(fw, dist, kind)
    for A in R.DENSE_ANCHOR_COUNTS:
        anchors = R.dense_anchors(n, A)
        assert A < 2 or anchors[0] == anchors[-1]                # a duplicate anchor
        for dis_q in R.DIS_QS:
            if kind == "lattice" and n >= 16:
                _vacuity_dis_q(dist[:, anchors], dis_q)
            # the code formula on the oracle's own distances (equal to float64's on the lattice)
            assert R.same_bits(cref.position_code(fw, anchors, dis_q), R.position_code64(fw, anchors, dis_q))
            if kind == "lattice":
                assert R.same_bits(cref.position_code(fw, anchors, dis_q), R.position_code64(dist, anchors, dis_q))
    print(f"dense n={n} {kind}: {err:.2f} u (bound {max(n - 1, 1)} u)")


# ---- (b) batched ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "real"])
@pytest.mark.parametrize("n,G", R.BATCH_CASES)
def test_oracle_batch_paths_and_codes(n, G, kind):
    adj, dist, hops = R.batch_case(n, G, kind)
    _vacuity_paths(dist, hops)
    assert G == 1 or not np.array_equal(adj[0], adj[1]) or n == 1
    fw = np.stack([cref.floyd_warshall(adj[g]) for g in range(G)])
    err = R.check_paths(fw, dist, kind)
    for A in R.BATCH_ANCHOR_COUNTS:
        anchors = R.batch_anchors(n, G, A)
        assert G == 1 or n < 16 or A == 1 or not np.array_equal(anchors[0], anchors[1])
        for dis_q in R.DIS_QS:
            if kind == "lattice" and n >= 16:
                _vacuity_dis_q(np.take_along_axis(dist, np.broadcast_to(anchors[:, None, :], (G, n, A)), axis=2), dis_q)
            codes = cref.position_codes_batch(adj, anchors, dis_q)
            assert R.same_bits(codes, R.position_code64(fw, anchors, dis_q))
            if kind == "lattice":
                assert R.same_bits(codes, R.position_code64(dist, anchors, dis_q))
    print(f"batch n={n} G={G} {kind}: {err:.2f} u (bound {max(n - 1, 1)} u)")


# ---- (c) CSR routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.CSR_SIZES + R.CROSS_SIZES)
def test_oracle_csr_anchor_distances(n):
    adj, (rowptr, col, val) = R.csr_case(n, "lattice")
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    assert (val == 0).any() or n < 16                             # explicit zero entries
    assert ((rows == col) & (val != 0)).any() or n < 16           # self-loops
    full = R.shortest_paths64(adj) if n <= 64 else None
    for A in R.CSR_ANCHOR_COUNTS:
        anchors = R.csr_anchors(n, A)
        d64 = R.anchor_dists64(rowptr, col, val, anchors)
        if full is not None:
            assert np.array_equal(d64, full[:, anchors])          # two routes through the reference itself
        for dis_q in R.CSR_DIS_QS:
            if n >= 16:
                _vacuity_dis_q(d64, dis_q)
            codes, dist = cref.position_codes_csr(rowptr, col, val, anchors, dis_q)
            R.check_paths(dist, d64, "lattice")
            assert R.same_bits(codes, R.position_code64(d64, None, dis_q))


def test_oracle_csr_real_weights_within_path_bound():
    n = 257
    adj, (rowptr, col, val) = R.csr_case(n, "real")
    anchors = R.csr_anchors(n, 17)
    _, dist = cref.position_codes_csr(rowptr, col, val, anchors, 10.0)
    err = R.check_paths(dist, R.anchor_dists64(rowptr, col, val, anchors), "real")
    print(f"csr n={n} real: {err:.2f} u (bound {n - 1} u)")


# ---- (d) PageRank -----------------------------------------------------------------------------------------------------------------
def _oracle_pagerank(which, d, max_iter, eps=R.PAGERANK_EPS):
    _, gp, (rowptr, _, val), (rt, ct, vt) = R.pagerank_case(which)
    return cref.pagerank(rt, ct, vt, cref.csr_row_sums(rowptr, val), gp, d=d, eps=eps, max_iter=max_iter)


@pytest.mark.parametrize("d", R.PAGERANK_DS)
def test_oracle_pagerank_one_update_within_step_bound(d):
    p, iters = _oracle_pagerank("pagerank", d, 1)
    worst = R.check_pagerank_step(p, "pagerank", d)
    print(f"one PageRank update d={d}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("d", R.PAGERANK_DS)
def test_oracle_pagerank_converged_within_l1_bound(d):
    adj, gp, _, _ = R.pagerank_case("pagerank")
    sizes = np.diff(gp)
    it64 = R.pagerank64_stop_iters(adj, gp, d, R.PAGERANK_EPS)
    for g in range(len(sizes)):                                    # no trivial case: real graphs iterate, and converge
        has_edges = adj[gp[g]:gp[g + 1]].any()
        if sizes[g] >= 3 and has_edges:
            assert 3 <= it64[g] < 128, f"graph {g}: {it64[g]} float64 iterations"
        if sizes[g] >= 3:
            assert (adj[gp[g]:gp[g + 1]].sum(1) == 0).any()
    p, iters = _oracle_pagerank("pagerank", d, 128)
    l1, ratio = R.check_pagerank_converged(p, iters, "pagerank", d, R.PAGERANK_EPS, 128)
    assert np.abs(iters - it64).max() <= 1                         # (the count itself may differ by one at the eps edge)
    zero = slice(gp[9], gp[10])
    assert iters[9] == 0 and np.array_equal(p[zero], np.full(40, np.float32(1) / np.float32(40)))
    print(f"converged PageRank d={d}: worst L1 = {l1:.3e}, worst error / bound = {ratio:.3f}, iterations {iters.tolist()}")


def test_oracle_pagerank_fixed_iterations():
    _, gp, _, _ = R.pagerank_case("pagerank")
    p, iters = _oracle_pagerank("pagerank", 0.85, 5, eps=0.0)
    assert np.array_equal(iters, np.where(np.diff(gp) > 0, 5, 0))


# ---- (e) sample_prob, (f) row sums, (g) the pipeline -------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", R.SAMPLE_ALPHAS)
def test_oracle_sample_prob_within_bound(alpha):
    _, gp, _, _ = R.pagerank_case("pagerank")
    p, c = R.sample_inputs(gp)
    worst = R.check_sample_prob(cref.sample_prob(p, c, gp, alpha, R.SAMPLE_EPS), p, c, gp, alpha, R.SAMPLE_EPS)
    print(f"sample_prob alpha={alpha}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("kind", ["lattice", "real"])
@pytest.mark.parametrize("n", R.ROW_SUM_SIZES)
def test_oracle_row_sums(n, kind):
    rowptr, val = R.row_sum_case(n, kind)
    lens = np.diff(rowptr)
    assert lens.max() == R.ROW_SUM_LONG and (n == 1 or (lens == 0).any())
    worst = R.check_row_sums(cref.csr_row_sums(rowptr, val), rowptr, val, kind)
    print(f"row sums n={n} {kind}: worst error / bound = {worst:.3f}")


def test_oracle_pipeline_within_propagated_bound():
    adj, gp, (rowptr, _, val), (rt, ct, vt) = R.pagerank_case("pipeline")
    assert np.diff(gp).min() >= 2
    p, iters = cref.pagerank(rt, ct, vt, cref.csr_row_sums(rowptr, val), gp)
    assert iters.max() < 128
    prob = cref.sample_prob(p, cref.csr_row_sums(rt, vt), gp)
    worst = R.check_pipeline(prob)
    print(f"compute_sample_prob pipeline: worst error / bound = {worst:.3f}")
