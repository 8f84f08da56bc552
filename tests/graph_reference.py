"""Independent float64 references for the graph-analytic kernels: all-pairs and anchor shortest paths with their position
codes (rows.hip: fw_init / fw_step / position_code / anchor_dist and the global relaxation; bank.hip:
fw_position_batch), PageRank, the inverse-importance sampling probabilities and the CSR row sums (bank.hip).

numpy and the standard library only.  Nothing here restates a kernel's operation order: the shortest paths come from
Dijkstra's label-setting algorithm (the device runs Floyd-Warshall and a Bellman-Ford style relaxation), PageRank is a
dense float64 power iteration.  The formulas are the ones include/ragraph_hip.h states:
  dist = adj with 0 -> no edge, diagonal 0 (self-loops ignored);  code = 1 / (d + 1) if d < dis_q else 0
  p = 1/N;  new_p = (1 - d)/N + d (P^T p + dangling mass / N),  P = adj / row sums;  stop when ||new_p - p||_1 < eps and
      keep p (the iterate BEFORE the converged step)
  importance = alpha p + (1 - alpha) col_sum / (N - 1);  prob = (1 / (importance + eps)) / (sum over the graph)

Three kinds of statement follow from them (tests/test_cpu_graph_reference.py holds the C oracle to them, without a GPU;
tests/test_gpu_graph_edges.py holds the kernels to them and to the oracle's bits):
  * equality: on a lattice graph (weights k/64, k in 1..256) every path sum is a multiple of 2^-6 below 2^13 -- 19 bits --
    so fp32 adds them exactly under ANY association: Floyd-Warshall, the relaxation fixpoint and float64 Dijkstra are equal;
    so are the row sums of lattice values (5000 * 4 < 2^15: 21 bits);
  * bounds, each derived in its function's docstring from u = 2^-24 (the unit roundoff of fp32);
  * the position code itself is one correctly rounded fp32 add and one correctly rounded fp32 division of the fp32
    distance: numpy float32 does the same, so codes are compared for equality whenever the distances are.

Measured on the CPU oracle, for the shapes and seeds of the case lists at the end of this file (both test files print
these figures: pytest -s); the device gives the oracle's bits, hence the same figures:
  Floyd-Warshall / relaxation, lattice graphs    equal at every case                           equality
  Floyd-Warshall, real weights, dense            <= 5.11 u relative (n = 255)                  bound (n - 1) u = 254 u
  Floyd-Warshall, real weights, batched          <= 5.80 u relative (n = 64, G = 300)          bound 63 u
  relaxation on the CSR, real weights            3.87 u relative (n = 257)                     bound 256 u
  one PageRank update                            <= 0.25 of the bound                          bound (indeg + 8) u per element
  converged PageRank, L1                         <= 1.64e-6 (d = 0.85), 8.8e-7 (d = 0.5):      bound (eps + (..) u) / (1 - d)
                                                 <= 0.19 of the bound
  sample_prob                                    <= 0.22 of the bound                          bound (ceil(n/256) + 17) u
  row sums, lattice values                       equal                                         equality
  row sums, real values                          <= 0.90 of the bound (a row of two entries:   bound (len - 1) u sum |v|
                                                 one rounding of up to u |sum| against u sum|v|)
  compute_sample_prob end to end                 <= 0.005 of the bound                         pipeline_bound
"""
import functools
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24


def f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def same_bits(a, b):
    """Equal shapes and equal fp32 bit patterns (+0 and -0 differ, NaNs compare by payload)."""
    a, b = f32(a), f32(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def rel_err(got, ref):
    """max |got - ref| / |ref| over the finite, non-zero entries of ref (float64); 0.0 when there are none."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    m = np.isfinite(ref) & (ref != 0)
    return float((np.abs(got[m] - ref[m]) / np.abs(ref[m])).max()) if m.any() else 0.0


# ---- shortest paths -------------------------------------------------------------------------------------------------------
def _weights(adj):
    """[B, n, n] float64 edge lengths: 0 -> no edge (inf), diagonal -> no edge (a self-loop never shortens a path)."""
    w = np.array(adj, dtype=np.float64)
    w[w == 0] = np.inf
    idx = np.arange(w.shape[-1])
    w[..., idx, idx] = np.inf
    return w


def _dijkstra(w, graph_of, src):
    """Dijkstra's algorithm, one instance per source, the instances advanced side by side: source s lives in graph
    graph_of[s] of w [B, n, n] and starts at node src[s].  Each instance settles the unsettled node of least distance
    and relaxes that node's out-edges; with non-negative lengths a settled distance is final.  Returns (dist [S, n],
    hops [S, n]): the length of the shortest path source -> node and the number of edges of the path that gave it."""
    S, n = len(src), w.shape[-1]
    rows = np.arange(S)
    dist = np.full((S, n), np.inf)
    hops = np.zeros((S, n), dtype=np.int64)
    dist[rows, src] = 0.0
    settled = np.zeros((S, n), dtype=bool)
    for _ in range(n):
        cand = np.where(settled, np.inf, dist)
        u = cand.argmin(axis=1)
        du = cand[rows, u]
        live = np.isfinite(du)              # (an instance whose unsettled nodes are all unreachable is finished)
        if not live.any():
            break
        settled[rows[live], u[live]] = True
        via = du[:, None] + w[graph_of, u, :]
        better = (via < dist) & ~settled
        hops = np.where(better, hops[rows, u][:, None] + 1, hops)
        dist = np.where(better, via, dist)
    return dist, hops


def shortest_paths64(adj, return_hops=False):
    """dist[i][j] = length of the shortest path i -> j along out-edges of the directed dense matrix adj [n, n] (or a stack
    [G, n, n] of them), float64; inf where there is none, 0 on the diagonal.  adj == 0 is no edge, self-loops are ignored."""
    a = np.asarray(adj)
    w = _weights(a.reshape((-1,) + a.shape[-2:]))
    B, n = w.shape[0], w.shape[-1]
    dist, hops = _dijkstra(w, np.repeat(np.arange(B), n), np.tile(np.arange(n), B))
    dist, hops = dist.reshape(a.shape), hops.reshape(a.shape)
    return (dist, hops) if return_hops else dist


def anchor_dists64(rowptr, col, val, anchors):
    """dist[u][a] = length of the shortest path u -> anchors[a] on the CSR (float64): Dijkstra from every anchor along the
    REVERSED edges.  Explicit zero entries are no edges, self-loops are ignored, parallel entries are parallel edges."""
    rowptr, col, val = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(val, dtype=np.float64)
    anchors = np.asarray(anchors, dtype=np.int64).reshape(-1)
    n = rowptr.shape[0] - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    keep = (val != 0) & (row != col)
    wr = np.full((1, n, n), np.inf)
    np.minimum.at(wr[0], (col[keep], row[keep]), val[keep])      # wr[v][u] = length of the edge u -> v
    dist, _ = _dijkstra(wr, np.zeros(anchors.shape[0], dtype=np.int64), anchors)
    return np.ascontiguousarray(dist.T)


def position_code64(dist, anchors, dis_q):
    """code[u][a] = 1 / (d + 1) where d = dist[u][anchors[a]] < dis_q (strictly), else 0.  dist: [n, n] with anchors [A],
    [G, n, n] with anchors [G, A], or -- anchors None -- distances to the anchors already ([n, A]).  The distance is
    cast to fp32 first (on a lattice graph that cast is exact); the comparison, the add and the division then run in
    numpy float32, each correctly rounded, as the device's are."""
    d = np.asarray(dist)
    if anchors is not None:
        anchors = np.asarray(anchors, dtype=np.int64)
        if d.ndim == 3:
            d = np.take_along_axis(d, np.broadcast_to(anchors[:, None, :], (d.shape[0], d.shape[1], anchors.shape[1])), axis=2)
        else:
            d = d[:, anchors]
    d = f32(d)
    with np.errstate(over="ignore"):
        return np.where(d < F32(dis_q), F32(1) / (d + F32(1)), F32(0)).astype(F32)


def path_bound(n):
    """Relative bound on |fp32 shortest distance - real shortest distance| for positive weights: (n - 1) u.
    A shortest path is simple: at most n - 1 positive terms.  An fp32 sum of m positive terms, under any association, is
    within a factor (1 + u)^(m-1) of the real sum: <= (m - 1) u to first order, and the terms are the fp32 inputs
    themselves (no rounding of a term).  Both device algorithms return, per pair, the minimum over a set of such fp32
    path sums that contains a sum of the truly shortest path: the minimum is therefore <= real * (1 + (n-2) u), and
    every candidate is >= its own path's real length * (1 - (n-2) u) >= real * (1 - (n-2) u).  (n - 1) u covers both sides
    and the final cast of the float64 reference.  Reachability is no matter of rounding: the infinities must be equal."""
    return max(n - 1, 1) * U


# ---- PageRank, sampling probabilities, row sums ---------------------------------------------------------------------------
def row_sums64(rowptr, val):
    """Exactly rounded float64 sum of every CSR row (math.fsum)."""
    rowptr, val = np.asarray(rowptr, dtype=np.int64), np.asarray(val, dtype=np.float64)
    return np.array([math.fsum(val[lo:hi]) for lo, hi in zip(rowptr[:-1], rowptr[1:])], dtype=np.float64)


def row_sum_bound(length, abs_sum):
    """Absolute bound on |fp32 sequential sum - real sum| of `length` terms: (length - 1) u * sum |v|.
    Each of the length - 1 additions rounds a partial sum whose magnitude is at most sum |v| (1 + u)^k: relative error u
    of at most that, so every addition contributes at most u * sum |v| to first order.  (The first addition, 0 + v, is exact.)"""
    return np.maximum(np.asarray(length, dtype=np.float64) - 1, 0) * U * np.asarray(abs_sum, dtype=np.float64)


def _graphs(adj, graph_ptr):
    """(lo, hi, P^T [N, N] float64, dangling mask [N]) for every non-empty graph of the block-diagonal dense batch."""
    adj = np.asarray(adj)
    for lo, hi in zip(graph_ptr[:-1], graph_ptr[1:]):
        lo, hi = int(lo), int(hi)
        if hi == lo:
            continue
        b = adj[lo:hi, lo:hi].astype(np.float64)
        out = b.sum(axis=1)
        dang = out == 0
        p_mat = np.divide(b, out[:, None], out=np.zeros_like(b), where=~dang[:, None])
        yield lo, hi, np.ascontiguousarray(p_mat.T), dang


def _update(pt, dang, p, d):
    n = p.shape[0]
    return (1.0 - d) / n + d * (pt @ p + p[dang].sum() / n)


def _d64(d):
    return float(F32(d))      # the damping factor the kernel receives is an fp32 argument


def pagerank64_steps(adj, graph_ptr, d, steps):
    """The PageRank iterate after exactly `steps` updates from the uniform start, per graph of the batch, float64."""
    p = np.zeros(int(graph_ptr[-1]), dtype=np.float64)
    for lo, hi, pt, dang in _graphs(adj, graph_ptr):
        q = np.full(hi - lo, 1.0 / (hi - lo))
        for _ in range(steps):
            q = _update(pt, dang, q, _d64(d))
        p[lo:hi] = q
    return p


def pagerank64_fixpoint(adj, graph_ptr, d, tol=1e-15, limit=5000):
    """The stationary vector per graph: float64 power iteration from the uniform start until the L1 change is below tol."""
    p = np.zeros(int(graph_ptr[-1]), dtype=np.float64)
    for lo, hi, pt, dang in _graphs(adj, graph_ptr):
        q = np.full(hi - lo, 1.0 / (hi - lo))
        for _ in range(limit):
            nq = _update(pt, dang, q, _d64(d))
            change = np.abs(nq - q).sum()
            q = nq
            if change < tol:
                break
        else:
            raise RuntimeError(f"pagerank64_fixpoint: graph [{lo}, {hi}) did not settle within {limit} iterations")
        p[lo:hi] = q
    return p


def pagerank64_stop_iters(adj, graph_ptr, d, eps):
    """Updates a float64 run ASSIGNS per graph under the stop rule (break before the assignment once ||new_p - p||_1 < eps);
    0 for an empty graph.  Only to show that a case is no trivial one: the device's count may differ by one at the edge."""
    iters = np.zeros(len(graph_ptr) - 1, dtype=np.int64)
    sizes = np.diff(np.asarray(graph_ptr))
    where = np.flatnonzero(sizes > 0)
    for g, (lo, hi, pt, dang) in zip(where, _graphs(adj, graph_ptr)):
        q = np.full(hi - lo, 1.0 / (hi - lo))
        while iters[g] < 100000:
            nq = _update(pt, dang, q, _d64(d))
            if np.abs(nq - q).sum() < eps:
                break
            q = nq
            iters[g] += 1
    return iters


def pagerank_step_bound(indeg):
    """Relative, per element, for the state after ONE update from the uniform start (max_iter = 1): (indeg + 8) u.
    new_p[j] = a + d * (s + dang) with non-negative terms, so relative errors combine as a maximum, plus one per operation
    (to first order in u):
      s = sum over the indeg in-edges of (val / out_deg[i]) * p0:  p0 = fl(1/N) (1), out_deg = the fp32 sum of the row's
          entries (at most 3 roundings: the generators keep real-weight rows to <= 4 entries; 0/1 rows sum exactly), the
          division (1), one fused multiply-add per in-edge (indeg): <= indeg + 5;
      dang = (tree sum of the dangling nodes' p0) / N: one dangling node: p0 (1) and the division (1); the all-dangling
          graph of 40 nodes: p0 (1), a tree over 40 EQUAL values in which only 2 p0 + p0 and 3 p0 + 2 p0 can round (2), the
          division (1): <= 4, no more than s;
      s + dang (1), * d (1): <= indeg + 7;  a = fl(fl(1 - d) / N): 2;  the last addition (1): <= indeg + 8.
    d itself is the fp32 value the kernel receives, in the reference too."""
    return (np.asarray(indeg, dtype=np.float64) + 8) * U


def pagerank_l1_bound(eps, d, max_indeg, n):
    """Bound on ||p - pi||_1 for the kept iterate p of a converged run (pi = the float64 fixpoint):
    (eps + (max_indeg + n/256 + 16) u) / (1 - d).
    T (the exact update) contracts L1 distances between probability vectors by d.  The run stops on
    ||T~ p - p||_1 < eps with T~ the rounded update, and keeps p.  Then ||p - pi|| <= ||p - T p|| + ||T p - T pi|| <=
    (eps + delta) + d ||p - pi||, so ||p - pi|| <= (eps + delta) / (1 - d) with delta >= ||T~ p - T p||_1 plus the rounding
    of the L1 change itself.  Per element T~ p is within (max_indeg + 8) u (pagerank_step_bound, p now any iterate: its
    dangling sum is 256 strided partial sums, ceil(n/256) - 1 additions each, and an 8-level tree: n/256 + 8 more on the
    dangling part, which is a convex part of the element), and ||T p||_1 = 1: delta <= (max_indeg + n/256 + 16) u covers it;
    the fp32 L1 change (a sum of n non-negative terms of total ~eps, relative error (n/256 + 9) u of eps) is far below u."""
    return (eps + (max_indeg + n / 256.0 + 16) * U) / (1.0 - _d64(d))


def sample_prob64(p, col_sum, graph_ptr, alpha, eps):
    """prob = (1 / (alpha p + (1 - alpha) col_sum / (N - 1) + eps)) / (sum over the graph), float64, on the fp32 inputs and
    the fp32 values of alpha and eps the kernel receives.  A one-node graph divides by N - 1 = 0: col_sum / 0 is inf (or
    NaN), the importance inf (or NaN), its inverse 0 (or NaN), the total the same, and 0 / 0 = NaN: NaN either way."""
    p, col_sum = np.asarray(p, dtype=np.float64), np.asarray(col_sum, dtype=np.float64)
    alpha, eps = float(F32(alpha)), float(F32(eps))
    out = np.zeros_like(p)
    with np.errstate(divide="ignore", invalid="ignore"):
        for lo, hi in zip(graph_ptr[:-1], graph_ptr[1:]):
            lo, hi = int(lo), int(hi)
            if hi == lo:
                continue
            imp = alpha * p[lo:hi] + (1.0 - alpha) * (col_sum[lo:hi] / float(hi - lo - 1))
            inv = 1.0 / (imp + eps)
            out[lo:hi] = inv / inv.sum()
    return out


def sample_prob_bound(n):
    """Relative, per element: (ceil(n/256) + 17) u, for alpha in {0, 0.5, 1} (products by 0, 0.5 and 1 are exact, and so is
    1 - alpha; any other alpha adds 4).  Every term is non-negative, so relative errors never amplify:
      imp = alpha p + (1 - alpha) (col_sum / fl(N - 1)): the division (1) and the addition (1): <= 2;  + eps (1), the inverse
      (1): inv <= 4.  tot: 256 strided partial sums of at most ceil(n/256) terms (ceil(n/256) - 1 additions) and an 8-level
      tree (8) over terms that carry 4 each: <= 4 + ceil(n/256) + 7.  prob = inv / tot (1): 4 + 4 + ceil(n/256) + 7 + 1 =
      ceil(n/256) + 16 to first order; one more unit covers the second-order terms and the fp32 eps, alpha arguments."""
    return (math.ceil(n / 256) + 17) * U


def pipeline_bound(n, alpha, l1_bound, max_col_len, imp_min, eps):
    """Relative, per element, for compute_sample_prob end to end against the float64 pipeline:
    sample_prob_bound(n) + 2 rho / (1 - rho),  rho = (alpha * l1_bound) / (imp_min + eps) + (max_col_len - 1) u.
    The fp32 pipeline feeds sample_prob a PageRank vector with ||dp||_1 <= l1_bound, hence |dp_i| <= l1_bound, and column
    sums of positive entries with relative error (len - 1) u (row_sum_bound).  imp = alpha p + (1 - alpha) c / (N - 1) is
    LINEAR in p and c: |d imp_i| <= alpha |dp_i| + (len - 1) u imp_i, so inv_i = 1 / (imp_i + eps) moves by a relative
    rho_i / (1 - rho_i) with rho_i <= rho (imp_min = the least float64 importance of the graph).  prob_i = inv_i / sum inv:
    the sum of positive terms moves by at most the same relative amount, the quotient by at most twice it.  On top comes
    the rounding of sample_prob itself on the inputs it was given."""
    rho = alpha * l1_bound / (imp_min + eps) + max(max_col_len - 1, 0) * U
    return sample_prob_bound(n) + 2 * rho / (1 - rho)


# ---- generators (every graph is DIRECTED) -----------------------------------------------------------------------------
def _structure(n, rng):
    """Directed edge mask [n, n]: every node i has the forward edge i -> i+1, each of i -> i+2, i -> i+3 with probability
    3/4, one backward edge to one of i-1 .. i-3, a long edge to a random node with probability 1/10 and a self-loop with
    probability 1/10 (about 4 out-edges); the last node always has a self-loop.  n >= 8: the rows of the last n//4 nodes
    are zeroed in the columns of the others (that block of pairs is unreachable), and the four nodes before t = n//2 keep
    ONE edge each, the chain t-4 -> t-3 -> t-2 -> t-1 -> t: every path out of them runs along it, so their distances to t
    are the sums of the chain's lengths."""
    m = np.zeros((n, n), dtype=bool)
    for i in range(n):
        for o in (1, 2, 3):
            if i + o < n and (o == 1 or rng.random() < 0.75):
                m[i, i + o] = True
        if i > 0:
            m[i, i - int(rng.integers(1, min(i, 3) + 1))] = True
        if rng.random() < 0.1:
            m[i, int(rng.integers(0, n))] = True
        if rng.random() < 0.1 or (i == n - 1 and n >= 2):
            m[i, i] = True
    if n >= 8:
        tail = n - n // 4
        m[tail:, :tail] = False
        for i in planted_chain(n):
            m[i, :] = False
            m[i, i + 1] = True
    return m


def planted_chain(n):
    """The nodes t-4 .. t-1 of _structure (n >= 8)."""
    return range(n // 2 - 4, n // 2)


def planted_anchor(n):
    """The node t of _structure (the end of the planted chain), or 0 for graphs too small to have one."""
    return n // 2 if n >= 8 else 0


def lattice_graph(n, seed):
    """Directed dense adjacency [n, n] fp32 with weights k/64, k in 1..256, on _structure; the planted chain weighs
    4, 4, 4, 2: the distances to t along it are 14, 10, 6 and 2 -- exact hits of dis_q = 2.0 and of dis_q = 10.0, and values
    on both sides of each.  A simple path has at most n - 1 <= 1024 edges of at most 4: every path sum and every
    d[i][k] + d[k][j] is a multiple of 2^-6 below 2^13 -- exact in fp32 under any association."""
    rng = np.random.default_rng([seed, n, 1])
    m = _structure(n, rng)
    a = np.where(m, rng.integers(1, 257, (n, n)) / 64.0, 0.0).astype(F32)
    if n >= 8:
        for i, w in zip(planted_chain(n), (4.0, 4.0, 4.0, 2.0)):
            a[i, i + 1] = w
    return a


def real_graph(n, seed):
    """The same structure with weights U(0.05, 3), fp32."""
    rng = np.random.default_rng([seed, n, 2])
    m = _structure(n, rng)
    return np.where(m, rng.uniform(0.05, 3.0, (n, n)), 0.0).astype(F32)


def draw_anchors(n, A, seed):
    """A anchors in [0, n): the planted anchor first, random ones after it, and -- A >= 2 -- the last a duplicate of the first."""
    rng = np.random.default_rng([seed, n, A, 3])
    anchors = rng.integers(0, n, A).astype(np.int64)
    anchors[0] = planted_anchor(n)
    if A >= 2:
        anchors[-1] = anchors[0]
    return anchors


def to_csr(adj, seed=None):
    """(rowptr int64, col int32, val fp32) of a dense adjacency, columns ascending within a row; the diagonal's non-zeros stay
    (self-loops).  With a seed, about one explicit ZERO entry per four rows is stored too (no edge, by the convention),
    and entry (0, 0) whatever its value."""
    a = f32(adj)
    n = a.shape[0]
    keep = a != 0
    if seed is not None:
        rng = np.random.default_rng([seed, n, 4])
        keep = keep | (rng.random((n, n)) < 0.25 / n)
        keep[0, 0] = True                 # (an entry even in a one-node graph: a self-loop, or an explicit zero)
    rows, cols = np.nonzero(keep)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return rowptr, cols.astype(np.int32), a[rows, cols].astype(F32)


def graph_batch(spec, seed):
    """Block-diagonal dense batch for PageRank: (adj [N, N] fp32, graph_ptr [G+1] int64).  spec lists a size, or (size, kind)
    with kind "loop" (one node with a self-loop), "dangling" (no entry) or "zero" (every row zero).  Graphs at an even
    position have 0/1 entries (four random out-edges per node, self-loops possible); graphs at an odd position have the
    real weights deg_i^-1/2 deg_j^-1/2 of (B + I), B directed 0/1 with up to three out-edges per node (a row holds at
    most 4 entries).  Every graph of >= 3 nodes has one all-zero (dangling) row; the two-node graph is the edge 0 -> 1."""
    sizes = [s if isinstance(s, int) else s[0] for s in spec]
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    adj = np.zeros((int(gp[-1]), int(gp[-1])), dtype=F32)
    for g, s in enumerate(spec):
        kind = None if isinstance(s, int) else s[1]
        n = sizes[g]
        rng = np.random.default_rng([seed, g, n, 5])
        b = np.zeros((n, n), dtype=np.float64)
        if kind == "loop":
            b[:] = 1.0
        elif kind in ("dangling", "zero") or n == 0:
            pass
        elif n == 1:
            raise ValueError("graph_batch: a one-node graph needs a kind")
        elif n == 2:
            b[0, 1] = 1.0
        else:
            deg = 4 if g % 2 == 0 else 3
            for i in range(n):
                b[i, rng.choice(n, size=min(deg, n - 1), replace=False)] = 1.0
            if g % 2 == 1:
                b[np.arange(n), np.arange(n)] = 0.0
                for i in range(n):               # (a target equal to i was dropped: at most three off-diagonal entries)
                    assert b[i].sum() <= 3
                b = b + np.eye(n)
                dg = b.sum(axis=1) ** -0.5
                b = b * dg[:, None] * dg[None, :]
            b[int(rng.integers(0, n))] = 0.0
        adj[gp[g]:gp[g + 1], gp[g]:gp[g + 1]] = b.astype(F32)
    return adj, gp


def batch_csr(adj):
    """((rowptr, col, val), (rowptr_t, col_t, val_t)): the CSR of the batch and of its transpose, columns ascending."""
    a = f32(adj)
    return to_csr(a), to_csr(np.ascontiguousarray(a.T))


# ---- the cases: ONE list for tests/test_cpu_graph_reference.py and tests/test_gpu_graph_edges.py ----------------------------
DIS_QS = (10.0, 2.0, float("inf"))

# (a) dense all-pairs: 256 columns per block of fw_step (255 / 256 / 257 / 513), n * A = 256 for position_code (25, 26 at A = 10)
DENSE_SIZES = (1, 2, 3, 25, 26, 255, 256, 257, 513)
DENSE_ANCHOR_COUNTS = (1, 10, 17)
DENSE_SEED = 11

# (b) batched: 256 threads over n * n slots (16 / 17), the LDS limit n = 64; G = 300 is more workgroups than the chip has CUs
BATCH_SIZES = (1, 2, 15, 16, 17, 63, 64)
BATCH_GRAPHS = (1, 3, 300)
BATCH_CASES = tuple((n, G) for n in BATCH_SIZES for G in BATCH_GRAPHS)
BATCH_ANCHOR_COUNTS = (1, 10, 17)
BATCH_SEED = 23

# (c) CSR routes: the LDS kernel's 1024 threads stride over the nodes
CSR_SIZES = (1, 2, 1023, 1024, 1025)
CSR_ANCHOR_COUNTS = (1, 16, 17)
CSR_DIS_QS = (2.0, 10.0)
CSR_SEED = 37
CROSS_SIZES = (1, 2, 17, 64)        # dense, batch, LDS and global on one graph

# (d) PageRank: 256-strided reductions per graph; the empty graphs are legal
PAGERANK_SPEC = ((1, "loop"), (1, "dangling"), 2, 0, 255, 256, 257, 513, 1025, (40, "zero"), 0)
PAGERANK_SEED = 41
PAGERANK_DS = (0.85, 0.5)
PAGERANK_MAX_ITERS = (1, 3, 128)
PAGERANK_EPS = 1e-6

# (e) sample_prob on the sizes of (d)
SAMPLE_ALPHAS = (0.0, 0.5, 1.0)
SAMPLE_EPS = 1e-6
SAMPLE_SEED = 43

# (f) row sums: 256 rows per block
ROW_SUM_SIZES = (1, 255, 256, 257)
ROW_SUM_LONG = 5000
ROW_SUM_SEED = 47

# (g) compute_sample_prob end to end: (d) without the empty and the one-node graphs
PIPELINE_SPEC = (2, 255, 256, 257, 513, 1025, (40, "zero"))
PIPELINE_SEED = 53


@functools.lru_cache(maxsize=None)
def dense_case(n, kind):
    """(adj fp32, dist64, hops) of dense case n, kind "lattice" or "real" (computed once per process; treat as read-only)."""
    adj = lattice_graph(n, DENSE_SEED) if kind == "lattice" else real_graph(n, DENSE_SEED)
    dist, hops = shortest_paths64(adj, return_hops=True)
    return adj, dist, hops


def dense_anchors(n, A):
    return draw_anchors(n, A, DENSE_SEED)


@functools.lru_cache(maxsize=None)
def batch_case(n, G, kind):
    """(adj [G, n, n] fp32, dist64 [G, n, n], hops): every graph of the batch is a different one."""
    make = lattice_graph if kind == "lattice" else real_graph
    adj = np.stack([make(n, BATCH_SEED + 1000 * (g + 1)) for g in range(G)])
    dist, hops = shortest_paths64(adj, return_hops=True)
    return adj, dist, hops


def batch_anchors(n, G, A):
    """[G, A]: every graph has its own anchors."""
    return np.stack([draw_anchors(n, A, BATCH_SEED + 1000 * (g + 1)) for g in range(G)])


@functools.lru_cache(maxsize=None)
def csr_case(n, kind, seed=CSR_SEED):
    """(adj fp32, (rowptr, col, val)) of a CSR case: explicit zero entries and self-loops are stored."""
    adj = lattice_graph(n, seed) if kind == "lattice" else real_graph(n, seed)
    return adj, to_csr(adj, seed)


def csr_anchors(n, A, seed=CSR_SEED):
    return draw_anchors(n, A, seed)


@functools.lru_cache(maxsize=None)
def pagerank_case(which="pagerank"):
    """(adj, graph_ptr, csr, csr_t) of the batch of (d) ("pagerank") or of (g) ("pipeline")."""
    adj, gp = graph_batch(PAGERANK_SPEC, PAGERANK_SEED) if which == "pagerank" else graph_batch(PIPELINE_SPEC, PIPELINE_SEED)
    csr, csr_t = batch_csr(adj)
    return adj, gp, csr, csr_t


def graph_max_indeg(rowptr_t, graph_ptr):
    """Per graph: the most entries a row of the transposed CSR holds (0 for an empty graph)."""
    lens = np.diff(np.asarray(rowptr_t))
    return np.array([int(lens[lo:hi].max()) if hi > lo else 0 for lo, hi in zip(graph_ptr[:-1], graph_ptr[1:])])


def sample_inputs(graph_ptr):
    """Random positive (p, col_sum) fp32 for (e): NOT a PageRank vector, sample_prob is tested as a pure function."""
    rng = np.random.default_rng([SAMPLE_SEED, int(graph_ptr[-1])])
    n = int(graph_ptr[-1])
    return rng.uniform(1e-4, 1.0, n).astype(F32), rng.uniform(0.0, 8.0, n).astype(F32) + F32(0.125)


@functools.lru_cache(maxsize=None)
def row_sum_case(n, kind):
    """(rowptr, val) of a CSR with empty rows, short rows and one row of ROW_SUM_LONG entries (the middle row)."""
    rng = np.random.default_rng([ROW_SUM_SEED, n, 0 if kind == "lattice" else 1])
    lens = rng.integers(0, 9, n)
    lens[rng.random(n) < 0.3] = 0
    lens[n // 2] = ROW_SUM_LONG
    if n > 1:
        lens[n - 1] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(rowptr[-1])
    if kind == "lattice":
        val = (rng.integers(1, 257, nnz) / 64.0).astype(F32)
    else:
        val = (rng.uniform(0.05, 3.0, nnz) * rng.choice([-1.0, 1.0], nnz)).astype(F32)
    return rowptr, val


# ---- the rules: ONE statement of each check, applied to the oracle (CPU) and to the device (GPU) -----------------------------
def check_paths(got, dist64, kind):
    """Distances against float64: equality on a lattice graph; on real weights the same infinities and path_bound(n).
    Returns the measured relative error in units of u."""
    got, n = f32(got), dist64.shape[-1]
    assert got.shape == dist64.shape
    if kind == "lattice":
        assert np.array_equal(got, f32(dist64)), "lattice distances differ from float64 Dijkstra"
        return 0.0
    assert np.array_equal(np.isinf(got), np.isinf(dist64)), "reachability differs from float64 Dijkstra"
    assert not np.isnan(got).any()
    err = rel_err(got, dist64)
    assert err <= path_bound(n), f"relative error {err / U:.2f} u > (n - 1) u, n = {n}"
    return err / U


@functools.lru_cache(maxsize=None)
def pagerank_reference(which, d, steps=None):
    """pagerank64_steps (steps given) or pagerank64_fixpoint of a PageRank case, computed once."""
    adj, gp, _, _ = pagerank_case(which)
    return pagerank64_steps(adj, gp, d, steps) if steps is not None else pagerank64_fixpoint(adj, gp, d)


def check_pagerank_step(p, which, d):
    """max_iter = 1 against pagerank64_steps(..., 1), element by element; returns the worst error / bound."""
    _, gp, _, (rowptr_t, _, _) = pagerank_case(which)
    ref = pagerank_reference(which, d, 1)
    bound = pagerank_step_bound(np.diff(rowptr_t)) * ref
    err = np.abs(np.asarray(p, dtype=np.float64) - ref)
    assert p.shape == ref.shape and (err <= bound).all(), \
        f"one PageRank update: worst error / bound = {(err / bound).max():.3f} at node {int((err / bound).argmax())}"
    return float((err / bound).max())


def check_pagerank_converged(p, iters, which, d, eps, max_iter):
    """A converged run against the float64 fixpoint: every non-empty graph stopped before max_iter and lies within
    pagerank_l1_bound; returns (worst L1 error, worst error / bound)."""
    _, gp, _, (rowptr_t, _, _) = pagerank_case(which)
    ref = pagerank_reference(which, d)
    indeg = graph_max_indeg(rowptr_t, gp)
    worst, worst_ratio = 0.0, 0.0
    for g, (lo, hi) in enumerate(zip(gp[:-1], gp[1:])):
        if hi == lo:
            continue
        assert int(iters[g]) < max_iter, f"graph {g} did not converge within {max_iter} iterations"
        l1 = float(np.abs(np.asarray(p[lo:hi], dtype=np.float64) - ref[lo:hi]).sum())
        bound = pagerank_l1_bound(eps, d, int(indeg[g]), int(hi - lo))
        assert l1 <= bound, f"graph {g} (n = {hi - lo}): ||p - pi||_1 = {l1:.3e} > {bound:.3e}"
        worst, worst_ratio = max(worst, l1), max(worst_ratio, l1 / bound)
    return worst, worst_ratio


def check_sample_prob(prob, p, col_sum, graph_ptr, alpha, eps):
    """sample_prob against float64: NaN exactly where the float64 restatement is NaN (the one-node graphs), the other
    elements within sample_prob_bound(n), and every graph of >= 2 nodes sums to 1 within (n/256 + 20) u (prob_i = inv_i / tot
    rounds once, and tot is the fp32 sum of the inv_i: ceil(n/256) + 7 roundings).  Returns the worst error / bound."""
    ref = sample_prob64(p, col_sum, graph_ptr, alpha, eps)
    prob = np.asarray(prob, dtype=np.float64)
    assert prob.shape == ref.shape and np.array_equal(np.isnan(prob), np.isnan(ref)), "NaN pattern differs"
    worst = 0.0
    for lo, hi in zip(graph_ptr[:-1], graph_ptr[1:]):
        n = int(hi - lo)
        if n == 1:
            assert np.isnan(ref[lo])          # N - 1 = 0: pinned as NaN
        if n < 2:
            continue
        err = np.abs(prob[lo:hi] - ref[lo:hi]) / ref[lo:hi]
        assert (err <= sample_prob_bound(n)).all(), f"graph of {n}: {err.max() / U:.2f} u > {sample_prob_bound(n) / U:.0f} u"
        assert abs(float(prob[lo:hi].sum()) - 1.0) <= (n / 256.0 + 20) * U
        worst = max(worst, float(err.max()) / sample_prob_bound(n))
    return worst


def check_row_sums(out, rowptr, val, kind):
    """Row sums against float64: equality for lattice values, row_sum_bound otherwise; returns the worst error / bound."""
    ref = row_sums64(rowptr, val)
    out = np.asarray(out, dtype=np.float64)
    assert out.shape == ref.shape
    if kind == "lattice":
        assert np.array_equal(out, ref), "lattice row sums differ from float64"
        return 0.0
    bound = row_sum_bound(np.diff(rowptr), row_sums64(rowptr, np.abs(val)))
    err = np.abs(out - ref)
    assert (err <= bound).all()
    return float((err[bound > 0] / bound[bound > 0]).max())


@functools.lru_cache(maxsize=None)
def pipeline_reference(alpha=0.5, eps=1e-6, d=0.85):
    """The float64 pipeline of compute_sample_prob on the batch of (g): (prob64, importance64)."""
    adj, gp, _, _ = pagerank_case("pipeline")
    pi = pagerank_reference("pipeline", d)
    col_sum = np.asarray(adj, dtype=np.float64).sum(axis=0)
    imp = np.zeros_like(pi)
    for lo, hi in zip(gp[:-1], gp[1:]):
        imp[lo:hi] = float(F32(alpha)) * pi[lo:hi] + (1 - float(F32(alpha))) * col_sum[lo:hi] / float(hi - lo - 1)
    return sample_prob64(pi, col_sum, gp, alpha, eps), imp


def check_pipeline(prob, alpha=0.5, eps=1e-6, d=0.85):
    """compute_sample_prob's result against the float64 pipeline under pipeline_bound, per graph; returns the worst
    error / bound."""
    _, gp, _, (rowptr_t, _, _) = pagerank_case("pipeline")
    ref, imp = pipeline_reference(alpha, eps, d)
    indeg = graph_max_indeg(rowptr_t, gp)
    prob = np.asarray(prob, dtype=np.float64)
    assert prob.shape == ref.shape and not np.isnan(prob).any()
    worst = 0.0
    for g, (lo, hi) in enumerate(zip(gp[:-1], gp[1:])):
        n = int(hi - lo)
        bound = pipeline_bound(n, alpha, pagerank_l1_bound(PAGERANK_EPS, d, int(indeg[g]), n), int(indeg[g]),
                               float(imp[lo:hi].min()), float(F32(eps)))
        err = np.abs(prob[lo:hi] - ref[lo:hi]) / ref[lo:hi]
        assert (err <= bound).all(), f"graph {g} (n = {n}): {err.max():.3e} > {bound:.3e}"
        worst = max(worst, float(err.max()) / bound)
    return worst
