"""Numpy restatement (uint64 / float32 / float64 arithmetic) of the draws of bank construction with build_rng = "device"
(ragraph_amd/csrc/rng.h, csrc/bank.hip): lp_draw, u53, the three event rules (edge slot, node drop, value drop), the weight
quantisation and the inverse-CDF pick.  tests/test_cpu_bank_rng.py pins it to tests/noise_oracle.py (Python ints);
tests/test_gpu_bank_rng.py holds the kernels to it bit for bit."""
import numpy as np

U64 = np.uint64
M32 = U64(0xFFFFFFFF)


def _u64(x):
    return np.asarray(x).astype(U64)


def splitmix64(x):
    with np.errstate(over="ignore"):
        x = _u64(x) + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def lp_draw(seed, row, draw):
    """splitmix64(splitmix64(seed ^ splitmix64(row)) + draw), broadcasting."""
    with np.errstate(over="ignore"):
        return splitmix64(splitmix64(U64(int(seed) & (2 ** 64 - 1)) ^ splitmix64(row)) + _u64(draw))


def lp_below(h, m):
    """The high 64 bits of h * m, from 32-bit halves (every partial product and sum stays below 2^64)."""
    h, m = _u64(h), _u64(m)
    h0, h1, m0, m1 = h & M32, h >> U64(32), m & M32, m >> U64(32)
    mid = h1 * m0 + ((h0 * m0) >> U64(32))
    mid2 = h0 * m1 + (mid & M32)
    return h1 * m1 + (mid >> U64(32)) + (mid2 >> U64(32))


def u53(w):
    return (_u64(w) >> U64(11)).astype(np.float64) * 2.0 ** -53


def event(w, t):
    """An event of probability t (float32) happens iff u53(w) < (double)t."""
    return u53(w) < np.asarray(t, np.float32).astype(np.float64)


# ---- edge rewrite -----------------------------------------------------------------------------------------------------------
def edge_threshold(p_i, p_j):
    return (np.asarray(p_i, np.float32) + np.asarray(p_j, np.float32)) * np.float32(0.5)


def edge_rewrite(seed, prob, graph_ptr, row_chunk=512):
    """(rowptr int64 [n+1], col int32): slot (i, j) of graph g kept iff event(lp_draw(seed, i, j - lo_g), (p_i + p_j) * 0.5f)."""
    prob = np.asarray(prob, np.float32)
    n = prob.shape[0]
    counts = np.zeros(n, np.int64)
    cols = []
    for lo, hi in zip(graph_ptr[:-1], graph_ptr[1:]):
        lo, hi = int(lo), int(hi)
        local = np.arange(hi - lo, dtype=U64)
        for r0 in range(lo, hi, row_chunk):
            rows = np.arange(r0, min(r0 + row_chunk, hi), dtype=U64)
            keep = event(lp_draw(seed, rows[:, None], local[None, :]), edge_threshold(prob[r0:r0 + rows.size, None], prob[None, lo:hi]))
            counts[r0:r0 + rows.size] = keep.sum(1)
            cols.append((np.nonzero(keep)[1] + lo).astype(np.int32))
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(counts)
    return rowptr, (np.concatenate(cols) if cols else np.zeros(0, np.int32))


def edge_thresholds_total(prob, graph_ptr):
    """(sum of the thresholds, sum of t (1 - t)) over every slot, in float64: mean and variance of the kept total."""
    prob = np.asarray(prob, np.float32)
    mean = var = 0.0
    for lo, hi in zip(graph_ptr[:-1], graph_ptr[1:]):
        t = np.clip(edge_threshold(prob[lo:hi, None], prob[None, lo:hi]).astype(np.float64), 0.0, 1.0)
        mean += float(t.sum())
        var += float((t * (1 - t)).sum())
    return mean, var


# ---- multinomial ------------------------------------------------------------------------------------------------------------
def weights(p):
    """w = (uint64)((double)min(p, 1) * 2^40); 0 for a negative or NaN p."""
    p = np.asarray(p, np.float32)
    ok = p > 0
    return np.where(ok, (np.minimum(np.where(ok, p, np.float32(0)), np.float32(1)).astype(np.float64) * 2.0 ** 40).astype(U64), U64(0))


def multinomial_segments(seed, prob, seg_ptr, S):
    """int64 [G, S]: seg start + the smallest i whose inclusive prefix exceeds t = lp_below(lp_draw(seed, g, s), W_g); -1 when
    W_g = 0."""
    w = weights(prob)
    G = len(seg_ptr) - 1
    out = np.full((G, S), -1, np.int64)
    draws = np.arange(S, dtype=U64)
    for g in range(G):
        lo, hi = int(seg_ptr[g]), int(seg_ptr[g + 1])
        cum = np.cumsum(w[lo:hi], dtype=U64)
        if hi <= lo or cum[-1] == 0:
            continue
        t = lp_below(lp_draw(seed, U64(g), draws), cum[-1])
        out[g] = lo + np.searchsorted(cum, t, side="right")
    return out


# ---- augment features ---------------------------------------------------------------------------------------------------------
def rows_kept(seed_drop, ids, prob, rate):
    """Row i kept iff event(lp_draw(seed_drop, id_i, 0), p_i * rate) (one float32 product)."""
    return event(lp_draw(seed_drop, _u64(ids), U64(0)), np.asarray(prob, np.float32) * np.float32(rate))
