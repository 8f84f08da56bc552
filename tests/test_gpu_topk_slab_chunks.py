"""The slab paths of the exact top-k calls on a bank of more than one key chunk (K.topk_cosine, K.topk_cosine_mix,
K.topk_dot_masked; csrc/topk_cosine.hip, slab_topk): per-chunk lists, chunk index bases, the merge per query slab.

N = 2^22 + 1 keys is above both chunk limits (2^22 and 65535 x 64), so every call scores the bank in G = 2 chunks of
nc = 2097153 keys; D = 8 is no fused width, so every call takes slabs; at this N a slab holds 64 queries, so B = 66 makes
two query slabs, the second of 2 rows.  Bit-exact (scores and indices) against oracle.cref on ALL 66 rows: normalize_rows,
linear, axpby, topk_rows as in test_gpu_topk_mix.oracle_topk; masked: the history entries set to the mask value, then
topk_rows.  The oracle is computed once per module, in blocks of query rows (a block's score matrix is 185 MB)."""
import numpy as np
import pytest
import torch

from oracle import cref

pytestmark = pytest.mark.gpu

N, D, A, B = (1 << 22) + 1, 8, 4, 66
NC = (N + 1) // 2                  # keys per chunk: chunk 0 = [0, NC), chunk 1 = [NC, N)
KS = (7, 70)                       # row top-k lists / the ordered large-k selection
W_STRUCT, W_SEM = 0.3, 0.7
MASK_VALUE = -1e8
PLANTED = (5, 65)                  # one query of each query slab: the same query, its normalised row at keys NC - 1, NC, N - 1
BLOCK = 11                         # oracle rows per block


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _codes(rng, n):
    d = rng.integers(0, 7, (n, A)).astype(np.float32)
    c = (1.0 / (d + 1.0)).astype(np.float32)
    c[rng.random((n, A)) < 0.3] = 0.0
    return c


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(4194305)
    q = rng.standard_normal((B, D), dtype=np.float32)
    pq = _codes(rng, B)
    pq[PLANTED[0]] = (1.0, 0.5, 0.0, 0.25)
    q[PLANTED[1]], pq[PLANTED[1]] = q[PLANTED[0]], pq[PLANTED[0]]
    keys = rng.standard_normal((N, D), dtype=np.float32)
    codes = _codes(rng, N)
    keys[NC - 1] = keys[NC] = keys[N - 1] = cref.normalize_rows(q[PLANTED[0]:PLANTED[0] + 1])[0]
    codes[NC - 1] = codes[NC] = codes[N - 1] = pq[PLANTED[0]]
    kn, pnn = cref.normalize_rows(keys), cref.normalize_rows(codes)
    qn, pqn = cref.normalize_rows(q), cref.normalize_rows(pq)

    # histories (query -> items): a query of each slab, items on both sides of the chunk boundary and the last key, a
    # duplicate, unsorted; every other query (64 among them, the first of the second slab) has an empty list
    hist = {0: [N - 1, NC, 12345, NC, NC - 1],
            PLANTED[0]: [NC - 1, 99],                      # the first planted key masked: NC and N - 1 stay on top
            64: [],
            PLANTED[1]: [NC, NC, N - 1, 0]}
    plain, mixed, masked = {k: [] for k in KS}, {k: [] for k in KS}, []
    for b0 in range(0, B, BLOCK):
        rows = slice(b0, min(b0 + BLOCK, B))
        sem = cref.linear(qn[rows], kn)
        for k in KS:
            plain[k].append(cref.topk_rows(sem, k))
        mix = cref.axpby(cref.linear(pqn[rows], pnn), np.float32(W_STRUCT), sem, np.float32(W_SEM))
        for k in KS:
            mixed[k].append(cref.topk_rows(mix, k))
        del sem, mix
        dot = cref.linear(q[rows], kn)                      # the masked call: raw rows, inner product
        if b0 == 0:                                         # (query 1's history: its own three best keys, so the mask decides)
            hist[1] = cref.topk_rows(dot[1:2], 3)[1][0].tolist()
        for b, items in hist.items():
            if rows.start <= b < rows.stop and items:
                dot[b - rows.start, items] = MASK_VALUE
        masked.append(cref.topk_rows(dot, KS[0]))
        del dot

    def cat(parts):
        return np.concatenate([s for s, _ in parts]), np.concatenate([i for _, i in parts])

    lists = [hist.get(b, []) for b in range(B)]
    rp = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    items = np.array([i for l in lists for i in l], dtype=np.int64)
    c = {"q": q, "pq": pq, "kn": kn, "pnn": pnn, "rp": rp, "items": items, "hist": hist,
         "plain": {k: cat(plain[k]) for k in KS}, "mixed": {k: cat(mixed[k]) for k in KS}, "masked": cat(masked)}
    for a in c["plain"], c["mixed"]:
        for k in KS:
            for b in PLANTED:                               # the merge must order an exact tie across the chunk boundary
                assert a[k][1][b, :3].tolist() == [NC - 1, NC, N - 1] and a[k][0][b, 0] == a[k][0][b, 1] == a[k][0][b, 2]
        i70 = a[KS[1]][1]                                   # 70 of 2^22 random keys: both chunks in every query's answer
        assert (i70 < NC).any(axis=1).all() and (i70 >= NC).any(axis=1).all()
    return c


@pytest.fixture(scope="module")
def bank(case, dev):
    return {n: T(case[n], dev) for n in ("q", "pq", "kn", "pnn", "rp", "items")}


def _equal(got, want, idx_base=0):
    s, i = got
    assert tuple(s.shape) == want[0].shape == (B, want[0].shape[1])                          # all 66 rows are compared
    assert np.array_equal(i.cpu().numpy(), want[1] + idx_base), "indices"
    assert np.array_equal(s.cpu().numpy(), want[0]), "scores"


@pytest.mark.parametrize("idx_base", [0, 1000])
@pytest.mark.parametrize("k", KS)
def test_cosine_over_two_key_chunks(dev, monkeypatch, case, bank, k, idx_base):
    from ragraph_amd import kernels as K

    monkeypatch.delenv("RAGRAPH_TOPK_SLAB", raising=False)
    _equal(K.topk_cosine(bank["q"], bank["kn"], k, idx_base=idx_base), case["plain"][k], idx_base)


@pytest.mark.parametrize("idx_base", [0, 1000])
@pytest.mark.parametrize("k", KS)
def test_mixed_over_two_key_chunks(dev, monkeypatch, case, bank, k, idx_base):
    from ragraph_amd import kernels as K

    monkeypatch.delenv("RAGRAPH_TOPK_SLAB", raising=False)
    got = K.topk_cosine_mix(bank["q"], bank["kn"], bank["pq"], bank["pnn"], W_STRUCT, W_SEM, k, idx_base=idx_base)
    _equal(got, case["mixed"][k], idx_base)


def test_masked_over_two_key_chunks(dev, monkeypatch, case, bank):
    from ragraph_amd import kernels as K

    monkeypatch.delenv("RAGRAPH_TOPK_SLAB", raising=False)
    k = KS[0]
    want_s, want_i = case["masked"]
    # the histories decide: query 1's three best keys are gone, the planted queries keep (NC, N - 1) and NC - 1 alone
    assert not set(case["hist"][1]) & set(want_i[1].tolist())
    assert want_i[PLANTED[0], :2].tolist() == [NC, N - 1] and NC - 1 not in want_i[PLANTED[0]]
    assert want_i[PLANTED[1], 0] == NC - 1 and NC not in want_i[PLANTED[1]] and N - 1 not in want_i[PLANTED[1]]
    assert (want_s > MASK_VALUE).all()
    _equal(K.topk_dot_masked(bank["q"], bank["kn"], k, bank["rp"], bank["items"], mask_value=MASK_VALUE), case["masked"])
