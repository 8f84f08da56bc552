"""A growing bank on the GPU: ragraph_topk_cosine_tail_f32 alone, KeyIndex with a tail behind every sealed dispatch class,
learnt state across extend, ToyGraphBase, capture.

Every comparison is bit for bit (scores as int32 views, indices as int64), against code that knows nothing of tails: a FRESH
K.KeyIndex over all rows (no extend was ever called on it: the path of a bank of one version) and, for 4 queries of every
case, oracle/cref.py::topk_cosine.

One case of the end-to-end list is stated with a bank of 2000 rows and appends of 40 + 300 rows; the sealing rule
(tail_rows > sealed_rows // 8 seals) folds that tail in at the second append, so that case asserts the seal the rule
demands, and a bank of 2800 rows on the same kernel carries the 340-row tail the list asks every case to end with."""

import numpy as np
import pytest
import torch

from oracle import cref

pytestmark = pytest.mark.gpu

I64_MAX = np.iinfo(np.int64).max


@pytest.fixture(scope="module")
def K(dev):
    from ragraph_amd import kernels
    return kernels


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same(got, want, what=""):
    assert torch.equal(got[1], want[1]), f"{what}: indices differ"
    assert torch.equal(_bits(got[0]), _bits(want[0])), f"{what}: score bits differ"


def _assert_oracle(got, q, rows, k, idx_base=0, n=4):
    os_, oi = cref.topk_cosine(q[:n], rows, k, idx_base)
    assert np.array_equal(got[1][:n].cpu().numpy(), oi)
    assert np.array_equal(got[0][:n].cpu().numpy().view(np.int32), os_.view(np.int32))


_others = {}


def _other_rows(K, dev, D):
    """3000 unit rows per width, made once and never changed."""
    if D not in _others:
        host = cref.normalize_rows(np.random.default_rng(100 + D).standard_normal((3000, D), dtype=np.float32))
        _others[D] = (host, torch.from_numpy(host).to(dev))
    return _others[D]


# every value of each axis at least once (T: 1, k - 1, k, 63, 64, 65, 257, 4097) + the corner
ENTRY_SHAPES = [(64, 1, 1, 1), (128, 10, 3, 9), (256, 10, 16, 10), (64, 32, 17, 63), (128, 33, 129, 64), (64, 64, 16, 65),
                (128, 10, 300, 257), (256, 32, 1, 31), (64, 33, 3, 4097), (256, 64, 300, 4097)]


@pytest.mark.parametrize("D, k, B, T", ENTRY_SHAPES)
def test_entry_continues_a_seed_over_a_tail(K, dev, D, k, B, T):
    """Seeds from K.topk_cosine over 3000 other rows; in the tail: bit copies of seed rows (the seed's copy must stay in front),
    rows that beat every seed row, all-zero rows; among the queries: one equal to a stored row, one all zero."""
    rng = np.random.default_rng(D * 1000 + k * 10 + B + T)
    other_h, other_d = _other_rows(K, dev, D)
    q = rng.standard_normal((B, D), dtype=np.float32)
    q[0] = other_h[100] * 2.5                       # its best seed rows: 100 and whatever lies next to it
    if B > 2:
        q[2] = 0
    tail = cref.normalize_rows(rng.standard_normal((T, D), dtype=np.float32))
    slots = iter(range(T))
    for j in slots:                                 # (T = 1 takes the first variant only, and so on)
        tail[j] = other_h[100]                      # a copy of query 0's best seed row: ties it, loses on the index
        break
    for j in slots:
        tail[j] = cref.normalize_rows(q[B - 1:B])[0]   # beats every seed row of the last query
        break
    for j in slots:
        tail[j] = 0                                 # scores 0 against every query
        break
    for j in slots:
        tail[j] = other_h[101]
        break
    if T > 64:
        tail[T - 1] = other_h[100]                  # the same copy again, in the last tile
        tail[T // 2] = cref.normalize_rows(q[B - 1:B])[0]
    qd, td = torch.from_numpy(q).to(dev), torch.from_numpy(tail).to(dev)
    seed_s, seed_i = K.topk_cosine(qd, other_d, k, idx_base=5)
    got = K.topk_cosine_tail(qd, td, seed_s, seed_i, 5 + 3000)
    rows_d = torch.cat([other_d, td])
    want = K.KeyIndex(rows_d).topk(qd, k, idx_base=5)
    _assert_same(got, want, f"D={D} k={k} B={B} T={T}")
    _assert_oracle(got, q, np.concatenate([other_h, tail]), k, 5)
    if B > 2:                                       # an all-zero query scores 0 everywhere: the seed comes back unchanged
        assert torch.equal(got[1][2], seed_i[2]) and torch.equal(_bits(got[0][2]), _bits(seed_s[2]))


@pytest.mark.parametrize("T", [3, 40])
def test_entry_takes_a_padded_seed(K, dev, T):
    """A seed made from 5 rows at k = 10: its end is -inf / INT64_MAX, as a shard's list; T = 3 leaves two entries padded."""
    D, k, B = 128, 10, 17
    rng = np.random.default_rng(7 + T)
    five = cref.normalize_rows(rng.standard_normal((5, D), dtype=np.float32))
    tail = cref.normalize_rows(rng.standard_normal((T, D), dtype=np.float32))
    tail[1] = five[3]
    q = rng.standard_normal((B, D), dtype=np.float32)
    q[0], q[2] = five[3], 0
    qd = torch.from_numpy(q).to(dev)
    s5, i5 = K.topk_cosine(qd, torch.from_numpy(five).to(dev), 5)
    seed_s = torch.full((B, k), float("-inf"), device=dev)
    seed_i = torch.full((B, k), I64_MAX, dtype=torch.int64, device=dev)
    seed_s[:, :5], seed_i[:, :5] = s5, i5
    got = K.topk_cosine_tail(qd, torch.from_numpy(tail).to(dev), seed_s, seed_i, 5)
    n = min(k, 5 + T)
    os_, oi = cref.topk_cosine(q, np.concatenate([five, tail]), n)
    assert np.array_equal(got[1][:, :n].cpu().numpy(), oi)
    assert np.array_equal(got[0][:, :n].cpu().numpy().view(np.int32), os_.view(np.int32))
    assert bool((got[1][:, n:] == I64_MAX).all()) and bool(torch.isinf(got[0][:, n:]).all())


def test_entry_refuses_bad_arguments_before_any_launch(K, dev):
    from ragraph_amd import _native as N

    L = K._ready()
    B, k = 4, 10
    buf = {D: torch.zeros(64, D, device=dev) for D in (100, 128)}
    ss, si = torch.zeros(B, 64, device=dev), torch.zeros(B, 64, dtype=torch.int64, device=dev)
    os_, oi = torch.full((B, 64), 7.0, device=dev), torch.full((B, 64), 7, dtype=torch.int64, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)

    def call(T=8, D=128, k=k, q=True, kt=True, seeds=True, out=True, w=True, ws_bytes=1 << 16):
        p = lambda t, on: t.data_ptr() if on else None
        return L.ragraph_topk_cosine_tail_f32(p(buf[D], q), B, p(buf[D], kt), T, D, k, 100, p(ss, seeds), p(si, seeds), p(os_, out),
                                              p(oi, out), p(ws, w), ws_bytes, None)

    assert N.TOPK_TAIL_MAX == 65536 and L.ragraph_abi_version() == 1
    assert call(T=0) == N.EINVAL and "T=0" in N.last_error()
    assert call(T=N.TOPK_TAIL_MAX + 1) == N.EINVAL
    assert call(k=65) == N.EINVAL and "k=65" in N.last_error()
    assert call(k=0) == N.EINVAL
    assert call(D=100) == N.EUNSUPPORTED and "D=100" in N.last_error()
    for null in ("q", "kt", "seeds", "out", "w"):
        assert call(**{null: False}) == N.EINVAL and "null" in N.last_error()
    assert call(ws_bytes=8) == N.EWORKSPACE
    assert L.ragraph_topk_cosine_tail_workspace_bytes(B, 0, 128, k) == 0
    assert L.ragraph_topk_cosine_tail_workspace_bytes(B, 8, 100, k) == 0
    torch.cuda.synchronize()
    assert bool((os_ == 7.0).all()) and bool((oi == 7).all())    # nothing ran
    assert call() == N.OK
    torch.cuda.synchronize()


# ---- KeyIndex end to end: one case per sealed dispatch class ------------------------------------------------------------------
def _bank_rows(K, dev, case):
    """(all rows on the device: N sealed + 340 appended, queries, k, a check that the sealed search is the class meant)"""
    name, B, N, D, k = case
    rng = np.random.default_rng(7 * B + 3 * N + D + k)
    if name == "collapsed":        # two thirds of the rows are copies: the search runs over the unique rows
        base = rng.standard_normal((N // 3, D), dtype=np.float32)
        host = np.concatenate([base, base, base])[rng.permutation(N)]
        host = np.concatenate([host, rng.standard_normal((340, D), dtype=np.float32)])
        host[N + 5] = host[17]                      # appended copies of sealed rows and of each other
        host[N + 6] = host[17]
        host[N + 50] = host[N + 7]
    else:
        host = rng.standard_normal((N + 340, D), dtype=np.float32)
        host[N + 3] = host[11]
        host[N + 60] = host[N + 3]
    q = rng.standard_normal((B, D), dtype=np.float32)
    q[0] = host[N + 3] if name != "collapsed" else host[N + 5]
    q[1] = host[N + 339]
    if B > 2:
        q[2] = 0
    rows = K.normalize_rows(torch.from_numpy(host).to(dev))
    return rows, torch.from_numpy(q).to(dev), q


INDEX_CASES = [("collapsed", 64, 3000, 64, 10), ("fused", 8192, 2000, 64, 10), ("fused", 8192, 2800, 64, 10),
               ("small", 16, 65536, 128, 10), ("filtered", 300, 65536, 256, 10), ("wide", 300, 65536, 256, 41),
               ("padded", 64, 7000, 100, 10)]


@pytest.mark.parametrize("case", INDEX_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-k{c[4]}")
def test_keyindex_with_a_tail_behind_every_dispatch_class(K, dev, case):
    name, B, N, D, k = case
    rows, qd, q = _bank_rows(K, dev, case)
    W = K.padded_dim(D)
    if name == "fused":
        assert K.fused_helps(B, N, W, k)
    elif name == "small":
        assert K.small_helps(B, N, W, k)
    elif name == "filtered":
        assert K.filter_helps(B, N, W, k) and not K.small_helps(B, N, W, k) and not K.fused_helps(B, N, W, k)
    elif name == "wide":
        assert K.filter_wide_helps(B, N, W, k)

    def fresh(n):
        return K.KeyIndex(rows[:n].clone()).topk(qd, k, idx_base=3)

    index = K.KeyIndex(rows[:N])
    _assert_same(index.topk(qd, k, idx_base=3), fresh(N), "before any append")
    if name == "collapsed":
        assert isinstance(index._collapsed, tuple)
    seen = index._queries
    index.extend(rows[:N + 40])
    assert (index.sealed_rows, index.tail_rows) == (N, 40) and index._queries == seen
    got = index.topk(qd, k, idx_base=3)
    _assert_same(got, fresh(N + 40), "40 rows appended")
    index.extend(rows)
    if N == 2000:          # 340 > 2000 // 8: the sealing rule folds this tail in (see the module docstring)
        assert (index.sealed_rows, index.tail_rows) == (2340, 0)
    else:
        assert (index.sealed_rows, index.tail_rows) == (N, 340)
    if name == "collapsed":
        assert isinstance(index._collapsed, tuple)   # the groups of the sealed rows are still in use
    got = index.topk(qd, k, idx_base=3)
    want = fresh(N + 340)
    _assert_same(got, want, "340 rows appended")
    host_rows = rows.cpu().numpy()
    _assert_oracle(got, q, host_rows, k, 3)
    if D == 100:
        assert tuple(index.keys_normalized.shape) == (N + 340, 128)
    else:
        assert index.keys_normalized is rows
    had_tail = index.tail_rows > 0
    index.seal()
    assert (index.sealed_rows, index.tail_rows) == (N + 340, 0)
    assert index._bf16 is None or not had_tail           # (the copies of the sealed rows go with a tail that is folded in)
    _assert_same(index.topk(qd, k, idx_base=3), want, "after seal()")


def test_a_learnt_prior_survives_extend(K, dev):
    case = ("filtered", 300, 65536, 256, 10)
    _, B, N, D, k = case
    rows, qd, _ = _bank_rows(K, dev, case)
    index = K.KeyIndex(rows[:N])
    g = torch.Generator(device=dev).manual_seed(3)
    assert B >= index.SPEC_MIN_BATCH
    for _ in range(index.SPEC_WARM_CALLS + 2):           # (a call's words are judged at the call after they arrived)
        index.topk(torch.randn(B, D, device=dev, generator=g), k)
        torch.cuda.synchronize()
    index.topk(torch.randn(B, D, device=dev, generator=g), k)
    assert index.last_prior is not None                   # warm
    spec, queries = index._spec, index._queries
    index.extend(rows[:N + 40])
    assert index._spec is spec and index._queries == queries and index.tail_rows == 40
    qn = torch.randn(B, D, device=dev, generator=g)
    got = index.topk(qn, k)
    assert index.last_prior is not None                   # no bound pass after the append
    _assert_same(got, K.KeyIndex(rows[:N + 40].clone()).topk(qn, k), "under the learnt prior")
    index.seal()
    got = index.topk(qn, k)
    assert index.last_prior is not None                   # nor after the fold
    _assert_same(got, K.KeyIndex(rows[:N + 40].clone()).topk(qn, k), "sealed, under the learnt prior")


def _toy_bank(dev, structure_weight=0.0):
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    tgb = ToyGraphBase(None, 3, 64, 3, device=dev)
    tgb.structure_weight = structure_weight
    return tgb


def test_toygraphbase_appends_behind_a_live_index(K, dev):
    rng = np.random.default_rng(11)
    n0, D, C, A = 5000, 64, 3, 10
    cuts = (n0, n0 + 40, n0 + 340)
    keys = torch.from_numpy((rng.standard_normal((cuts[-1], D)) * 2).astype(np.float32)).to(dev)
    values = torch.from_numpy(rng.standard_normal((cuts[-1], D), dtype=np.float32)).to(dev)
    labels = torch.from_numpy(np.eye(C, dtype=np.float32)[rng.integers(0, C, cuts[-1])]).to(dev)
    pos = torch.from_numpy(rng.random((cuts[-1], A), dtype=np.float32)).to(dev)
    h = torch.from_numpy(rng.standard_normal((200, D), dtype=np.float32)).to(dev)
    h[0] = keys[n0 + 20]
    hp = torch.from_numpy(rng.random((200, A), dtype=np.float32)).to(dev)

    grown = _toy_bank(dev)
    grown.add_resources(keys[:n0], values[:n0], labels[:n0], pos[:n0])
    grown.retrieve_reduced(h)
    index = grown._index
    assert index is not None
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        grown.add_resources(keys[lo:hi], values[lo:hi], labels[lo:hi], pos[lo:hi])
        assert grown._index is index and index.keys_normalized is grown._keys_normalized
        assert grown._keys_normalized.shape[0] == hi
    assert (index.sealed_rows, index.tail_rows) == (n0, 340)
    once = _toy_bank(dev)
    once.add_resources(keys, values, labels, pos)
    assert torch.equal(_bits(grown.keys_normalized), _bits(once.keys_normalized))
    a, b = grown.retrieve_reduced(h), once.retrieve_reduced(h)
    assert torch.equal(a[2], b[2]) and torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert bool((a[2][0] == n0 + 20).any())
    # structure-aware retrieval reads the code cache, which grew the same way
    grown_s, once_s = _toy_bank(dev, 0.001), _toy_bank(dev, 0.001)
    grown_s.add_resources(keys[:n0], values[:n0], labels[:n0], pos[:n0])
    grown_s.topk(h, 4, hp)
    first = grown_s._positions_normalized
    assert first is not None
    grown_s.add_resources(keys[n0:], values[n0:], labels[n0:], pos[n0:])
    assert grown_s._positions_normalized is not None and grown_s._positions_normalized.shape[0] == cuts[-1]
    once_s.add_resources(keys, values, labels, pos)
    assert torch.equal(_bits(grown_s.positions_normalized), _bits(once_s.positions_normalized))
    _assert_same(grown_s.topk(h, 4, hp), once_s.topk(h, 4, hp), "structure_weight = 0.001")


def test_a_captured_topk_with_a_tail_replays_and_never_seals(K, dev):
    from ragraph_amd.capture import CapturedForward

    rng = np.random.default_rng(13)
    N, D, k, B = 20000, 128, 10, 64
    rows = K.normalize_rows(torch.from_numpy(rng.standard_normal((N + 40, D), dtype=np.float32)).to(dev))
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    tgb = ToyGraphBase(None, 3, D, 3, device=dev)
    tgb.add_resources(rows[:N], rows[:N], torch.zeros(N, 3, device=dev))
    q = torch.from_numpy(rng.standard_normal((B, D), dtype=np.float32)).to(dev)
    tgb.topk(q, k)
    tgb.add_resources(rows[N:], rows[N:], torch.zeros(40, 3, device=dev))
    index = tgb._index
    assert index.tail_rows == 40
    want = K.KeyIndex(tgb.keys_normalized.clone()).topk(q, k)
    _assert_same(tgb.topk(q, k), want, "eager")

    def both(x):                                          # (one static output: the indices are exact in fp32 at this size)
        s, i = tgb.topk(x, k)
        return torch.cat([s, i.float()])

    fwd = CapturedForward(both, q)
    q2 = torch.from_numpy(rng.standard_normal((B, D), dtype=np.float32)).to(dev)
    q2[1] = rows[N + 7]
    out = fwd(q2).clone()
    want2 = K.KeyIndex(tgb.keys_normalized.clone()).topk(q2, k)
    assert torch.equal(_bits(out[:B]), _bits(want2[0])) and torch.equal(out[B:].long(), want2[1])
    assert bool((want2[1][1] == N + 7).any())
    # an over-limit tail under capture: no seal (it would drop copies mid-graph), no synchronisation, the same bits
    index.TAIL_MAX_ROWS = 8
    graph = torch.cuda.CUDAGraph()
    mode = torch.cuda.get_sync_debug_mode()
    static_q = q2.clone()
    with torch.no_grad(), torch.cuda.graph(graph):
        torch.cuda.set_sync_debug_mode("error")
        try:
            cap_s, cap_i = index.topk(static_q, k)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    assert (index.sealed_rows, index.tail_rows) == (N, 40)
    graph.replay()
    torch.cuda.synchronize()
    _assert_same((cap_s, cap_i), want2, "captured with an over-limit tail")
    index.topk(q2, k)                                     # the next eager call folds it in
    assert (index.sealed_rows, index.tail_rows) == (N + 40, 0)
