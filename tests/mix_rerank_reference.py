"""Mixed retrieval through the filter: the numpy restatement of ragraph_topk_mix_rerank_f32 over cref scores, and the inputs
the CPU and the GPU tests share (tests/test_cpu_topk_mix_filtered.py, tests/test_gpu_topk_mix_filtered.py).

The restatement uses the contract's own operations: cref.linear on the normalised rows (the fmaf chains from +0), cref.axpby
(two multiplies and one add, each rounded), float32 numpy arithmetic for the bound.  Nothing here reads the library."""
import functools

import numpy as np

from oracle import cref

WEIGHTS = ((0.02, 0.98), (0.05, 0.95), (0.3, 0.7))
# The route's reference shape (the smallest the rules send through the k <= 32 filtered entry) and its seed.
B0, N0, D0, A0, K0, KL0, SEED0 = 512, 8192, 128, 10, 10, 32, 1
# Unproven rows of np_rerank on route_inputs() at each of WEIGHTS, computed by tests/test_cpu_topk_mix_filtered.py (which
# asserts these very numbers from the restatement) and required of the device route by the GPU tests.
UNPROVEN0 = {(0.02, 0.98): 0, (0.05, 0.95): 130, (0.3, 0.7): 512}


def make_codes(rng, n, A, zero_rows=0.03):
    """As make_codes in tests/test_gpu_topk_mix.py: 1 / (d + 1) for a hop distance d, 0 for an anchor that cannot be reached;
    some rows reach no anchor at all."""
    d = rng.integers(0, 7, (n, A)).astype(np.float32)
    c = (1.0 / (d + 1.0)).astype(np.float32)
    c[rng.random((n, A)) < 0.3] = 0.0
    c[rng.random(n) < zero_rows] = 0.0
    return c


def make_raw(seed, B, N, D, A):
    """(q [B,D], keys [N,D], pq [B,A], codes [N,A]), all raw: Gaussian embeddings, codes as make_codes."""
    rng = np.random.default_rng(seed)
    keys = rng.standard_normal((N, D), dtype=np.float32)
    q = rng.standard_normal((B, D), dtype=np.float32)
    codes = make_codes(rng, N, A)
    pq = make_codes(rng, B, A)
    return q, keys, pq, codes


def make_inputs(seed, B, N, D, A):
    """make_raw with the bank normalised: (q raw, kn [N,D], pq raw, pnn [N,A])."""
    q, keys, pq, codes = make_raw(seed, B, N, D, A)
    return q, cref.normalize_rows(keys), pq, cref.normalize_rows(codes)


@functools.lru_cache(maxsize=1)
def route_inputs():
    """The reference shape's inputs with their semantic and structural score matrices (computed once per process)."""
    q, kn, pq, pnn = make_inputs(SEED0, B0, N0, D0, A0)
    sem = cref.linear(cref.normalize_rows(q), kn)
    struct = cref.linear(cref.normalize_rows(pq), pnn)
    for a in (q, kn, pq, pnn, sem, struct):
        a.setflags(write=False)
    return q, kn, pq, pnn, sem, struct


def oracle_mixed_topk(sem, struct, ws, wm, k):
    """The contract: axpby over the whole matrices, canonical row top-k."""
    return cref.topk_rows(cref.axpby(struct, np.float32(ws), sem, np.float32(wm)), k)


def np_slack(ws):
    """|w_struct| (1 + 2^-10) in double, rounded to float, one ulp up (csrc/mix_slack.h)."""
    w = np.float64(np.float32(ws))
    return np.nextafter(np.float32(abs(w) * (1.0 + 1.0 / 1024)), np.float32(np.inf), dtype=np.float32)


def np_rerank(sem_s, sem_i, pq, pnn, ws, wm, k, idx_base=0):
    """ragraph_topk_mix_rerank_f32: (scores [B,k], idx [B,k], unproven [B] int32).  sem_s, sem_i: canonical semantic lists
    [B,k'] (indices carry idx_base, all inside the bank); pq raw, pnn normalised."""
    sem_s = np.ascontiguousarray(sem_s, dtype=np.float32)
    sem_i = np.ascontiguousarray(sem_i, dtype=np.int64)
    B, kl = sem_s.shape
    assert 1 <= k < kl <= 128
    ws32, wm32 = np.float32(ws), np.float32(wm)
    struct = cref.linear(cref.normalize_rows(pq), pnn)                      # [B, N]: the chain of every (query, key)
    st = np.take_along_axis(struct, sem_i - idx_base, 1)
    mixed = cref.axpby(st, ws32, sem_s, wm32)
    out_s = np.empty((B, k), dtype=np.float32)
    out_i = np.empty((B, k), dtype=np.int64)
    for b in range(B):
        order = np.lexsort((sem_i[b], -mixed[b]))[:k]                       # score descending, index ascending
        out_s[b], out_i[b] = mixed[b, order], sem_i[b, order]
    with np.errstate(over="ignore", invalid="ignore"):
        bound = (sem_s[:, -1] * wm32).astype(np.float32) + np_slack(ws)
    finite = np.isfinite(mixed).all(1)
    unproven = (~((out_s[:, k - 1] > bound) & finite)).astype(np.int32)
    return out_s, out_i, unproven
