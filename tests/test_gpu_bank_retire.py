"""A shrinking bank on the GPU: ragraph_topk_drop_rows_f32 and ragraph_rows_retire_u32 alone, KeyIndex with retired rows behind
every dispatch class, ToyGraphBase.remove_resources / compact, capture.

Every comparison is bit for bit (scores as int32 views, indices equal).  The two entries are held to numpy restatements
written here; KeyIndex and ToyGraphBase to code that knows nothing of retired rows -- a FRESH K.KeyIndex (or bank) over a
clone of the live rows, its indices mapped through the live positions -- and, for 4 queries of every index case, to
oracle/cref.py::topk_cosine over the live rows."""

import numpy as np
import pytest
import torch

from oracle import cref

pytestmark = pytest.mark.gpu

I64_MAX = np.iinfo(np.int64).max
N_ROWS = 1000   # not a multiple of 32


@pytest.fixture(scope="module")
def K(dev):
    from ragraph_amd import kernels
    return kernels


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same(got, want, what=""):
    assert torch.equal(got[1], want[1]), f"{what}: indices differ"
    assert torch.equal(_bits(got[0]), _bits(want[0])), f"{what}: score bits differ"


def np_retire_rows(bitmap, rows, n_rows):
    for r in np.asarray(rows, dtype=np.int64).reshape(-1):
        if 0 <= r < n_rows:
            bitmap[r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    return bitmap


def np_drop_rows(scores, idx, bitmap, n_rows, k_out, idx_base=0):
    """The entry restated: a stable compaction per list of the entries whose row lies in [0, n_rows) with its bit clear."""
    B = scores.shape[0]
    r = idx - idx_base
    inside = (r >= 0) & (r < n_rows)
    rc = np.clip(r, 0, n_rows - 1)
    live = inside & (((bitmap[rc >> 5] >> (rc & 31).astype(np.uint32)) & 1) == 0)
    pos = np.cumsum(live, axis=1) - 1
    bb, ee = np.nonzero(live & (pos < k_out))
    out_s = np.full((B, k_out), -np.inf, dtype=np.float32)
    out_i = np.full((B, k_out), I64_MAX, dtype=np.int64)
    out_s[bb, pos[bb, ee]] = scores[bb, ee]
    out_i[bb, pos[bb, ee]] = idx[bb, ee]
    return out_s, out_i, int((live.sum(axis=1) < k_out).sum())


def _lists(B, k_in, idx_base, rng, padded=0):
    """B canonical lists over distinct rows of [0, N_ROWS); list 0 starts with rows 31, 32, 63, 64, 999 as far as it goes."""
    rows = np.stack([rng.permutation(N_ROWS)[:k_in] for _ in range(B)]).astype(np.int64)
    special = np.array([31, 32, 63, 64, 999])[:k_in]
    rest = np.array([r for r in rows[0] if r not in set(special.tolist())])
    rows[0] = np.concatenate([special, rest])[:k_in]
    scores = -np.sort(-rng.standard_normal((B, k_in), dtype=np.float32), axis=1)
    idx = rows + idx_base
    if padded:
        scores[:, k_in - padded:] = -np.inf
        idx[:, k_in - padded:] = I64_MAX
    return np.ascontiguousarray(scores), np.ascontiguousarray(idx), rows


@pytest.mark.parametrize("idx_base", [0, 3])
@pytest.mark.parametrize("k_in, k_out", [(2, 1), (33, 10), (64, 64), (65, 41), (128, 106), (129, 64), (300, 10)])
@pytest.mark.parametrize("B", [1, 5, 257])
def test_drop_entry_is_a_stable_compaction(K, dev, B, k_in, k_out, idx_base):
    rng = np.random.default_rng(B * 100000 + k_in * 100 + k_out + idx_base)
    scores, idx, rows = _lists(B, k_in, idx_base, rng)
    one = min(1, B - 1)
    edge = min(max(k_in - 4, 0), 60)                         # a run of adjacent entries, across entry 64 where the list has one
    retired_sets = {
        "none": [],
        "word edges": [31, 32, 63, 64, 999],
        "first entry of list 0": [rows[0, 0]],
        "last entry of list 1": [rows[one, k_in - 1]],
        "adjacent run": rows[0, edge:edge + 8].tolist(),
        "short list": rows[B - 1, :k_in - k_out + 1].tolist(),   # one list left with k_out - 1 live entries
    }
    cases = [(name, scores, idx, r) for name, r in retired_sets.items()]
    if (k_in, k_out) == (129, 64):                           # padded ends: 60 of 129 entries are -inf / INT64_MAX, 5 rows retired
        ps, pi, prow = _lists(B, k_in, idx_base, rng, padded=60)
        cases.append(("padded ends", ps, pi, prow[0, :5].tolist()))
        cases.append(("padded ends, short", ps, pi, prow[0, :6].tolist()))
    for name, s, i, retired in cases:
        bm = np_retire_rows(np.zeros(-(-N_ROWS // 32), dtype=np.uint32), retired, N_ROWS)
        bitmap = K.retire_rows(K.retired_bitmap(N_ROWS, dev), torch.tensor(retired, dtype=torch.int64, device=dev), N_ROWS)
        assert np.array_equal(bitmap.cpu().numpy().view(np.uint32), bm), name
        ws, wi, wshort = np_drop_rows(s, i, bm, N_ROWS, k_out, idx_base)
        gs, gi, gshort = K.topk_drop_rows(torch.from_numpy(s).to(dev), torch.from_numpy(i).to(dev), bitmap, N_ROWS, k_out, idx_base)
        what = f"{name}: B={B} k_in={k_in} k_out={k_out} idx_base={idx_base}"
        assert np.array_equal(gi.cpu().numpy(), wi), what
        assert np.array_equal(gs.cpu().numpy().view(np.int32), ws.view(np.int32)), what
        assert int(gshort.item()) == wshort, what
        if len(retired) <= (k_in - k_out if s is scores else 5):
            assert wshort == 0, what                         # no list can run short: it holds at least k_out live entries
        if name == "short list":
            assert wshort >= 1 and gi[B - 1, k_out - 1].item() == I64_MAX and torch.isinf(gs[B - 1, k_out - 1]), what
        if name == "padded ends, short":                     # 69 entries, 6 of list 0 retired: 63 live, one short of 64
            assert wshort == 1 and gi[0, 63].item() == I64_MAX, what


def test_drop_entry_drops_rows_outside_the_bank(K, dev):
    """Indices below idx_base and at or beyond idx_base + n_rows are dropped like retired rows."""
    s = torch.tensor([[9.0, 8.0, 7.0, 6.0, 5.0]], device=dev)
    i = torch.tensor([[2, 10 + 999, 10 + 1000, 10, I64_MAX]], dtype=torch.int64, device=dev)
    gs, gi, short = K.topk_drop_rows(s, i, K.retired_bitmap(N_ROWS, dev), N_ROWS, 3, idx_base=10)
    assert gi.tolist() == [[1009, 10, I64_MAX]] and gs[0, :2].tolist() == [8.0, 6.0] and int(short.item()) == 1


def test_drop_entry_refuses_bad_arguments_before_any_launch(K, dev):
    from ragraph_amd import _native as N

    L = K._ready()
    B = 4
    s, i = torch.zeros(B, 64, device=dev), torch.zeros(B, 64, dtype=torch.int64, device=dev)
    os_, oi = torch.full((B, 64), 7.0, device=dev), torch.full((B, 64), 7, dtype=torch.int64, device=dev)
    bitmap = K.retired_bitmap(N_ROWS, dev)
    short = torch.full((1,), 7, dtype=torch.int32, device=dev)

    def call(k_in=64, k_out=10, n_rows=N_ROWS, base=0, lists=True, bm=True, out=True, word=True, alias=False):
        p = lambda t, on: t.data_ptr() if on else None
        return L.ragraph_topk_drop_rows_f32(p(s, lists), p(i, lists), B, k_in, base, p(bitmap, bm), n_rows, k_out,
                                            p(s if alias else os_, out), p(oi, out), p(short, word), None)

    assert N.TOPK_ORDERED_MAX == 4096 and L.ragraph_abi_version() == 1
    for null in ("lists", "bm", "out", "word"):
        assert call(**{null: False}) == N.EINVAL and "null" in N.last_error()
    assert call(k_out=0) == N.EINVAL and "k_out=0" in N.last_error()
    assert call(k_in=10, k_out=11) == N.EINVAL and "k_out=11" in N.last_error()
    assert call(k_in=N.TOPK_ORDERED_MAX + 1) == N.EINVAL and "k_in=4097" in N.last_error()
    assert call(n_rows=0) == N.EINVAL and "n_rows=0" in N.last_error()
    assert call(base=-1) == N.EINVAL
    assert call(alias=True) == N.EINVAL and "alias" in N.last_error()
    assert L.ragraph_rows_retire_u32(None, 3, N_ROWS, bitmap.data_ptr(), None) == N.EINVAL and "null" in N.last_error()
    assert L.ragraph_rows_retire_u32(i.data_ptr(), 3, 0, bitmap.data_ptr(), None) == N.EINVAL
    assert L.ragraph_rows_retire_u32(i.data_ptr(), 3, N_ROWS, None, None) == N.EINVAL
    torch.cuda.synchronize()
    assert bool((os_ == 7.0).all()) and bool((oi == 7).all()) and short.item() == 7 and not bitmap.any()    # nothing ran
    assert L.ragraph_rows_retire_u32(None, 0, N_ROWS, bitmap.data_ptr(), None) == N.OK                       # m = 0: nothing to do
    short.zero_()
    assert call() == N.OK
    torch.cuda.synchronize()
    assert short.item() == 0 and bool((oi.view(-1)[:B * 10] == 0).all()) and bool((oi.view(-1)[B * 10:] == 7).all())   # out is [B, 10]


def test_retire_rows_sets_bits_once(K, dev):
    bitmap = K.retired_bitmap(N_ROWS, dev)
    assert bitmap.numel() == 32 and bitmap.dtype == torch.int32
    K.retire_rows(bitmap, torch.tensor([5, 31, 999], device=dev), N_ROWS)
    ids = [5, 5, 31, 32, 700, 700, 700, 1000, 1023, -1, 10 ** 12, 0]      # duplicates, bits already set, ids out of range
    K.retire_rows(bitmap, torch.tensor(ids, device=dev), N_ROWS)
    want = np_retire_rows(np.zeros(32, dtype=np.uint32), [5, 31, 999] + ids, N_ROWS)
    assert np.array_equal(bitmap.cpu().numpy().view(np.uint32), want)
    assert sum(bin(int(w)).count("1") for w in want) == 6    # rows 0, 5, 31, 32, 700, 999
    with pytest.raises(K.RagraphNativeError):
        K.retire_rows(K.retired_bitmap(64, dev), torch.tensor([1], device=dev), N_ROWS)    # a bitmap too short for n_rows


# ---- KeyIndex end to end: the seven shapes of tests/test_gpu_bank_tail.py::INDEX_CASES, one per dispatch class --------------
INDEX_CASES = [("collapsed", 64, 3000, 64, 10), ("fused", 8192, 2000, 64, 10), ("fused", 8192, 2800, 64, 10),
               ("small", 16, 65536, 128, 10), ("filtered", 300, 65536, 256, 10), ("wide", 300, 65536, 256, 41),
               ("padded", 64, 7000, 100, 10)]


def _bank_rows(K, dev, case):
    """(N + 40 normalised rows on the device, queries on the device and on the host, a sealed row stored twice)"""
    name, B, N, D, k = case
    rng = np.random.default_rng(11 * B + 5 * N + D + k)
    if name == "collapsed":        # two thirds of the rows are copies: the search runs over the unique rows
        base = rng.standard_normal((N // 3, D), dtype=np.float32)
        host = np.concatenate([base, base, base])[rng.permutation(N)]
        host = np.concatenate([host, rng.standard_normal((40, D), dtype=np.float32)])
    else:
        host = rng.standard_normal((N + 40, D), dtype=np.float32)
        host[20] = host[11]                                   # a duplicated sealed row
    q = rng.standard_normal((B, D), dtype=np.float32)
    q[1] = host[11] * 1.5
    q[3] = host[N + 7]                                        # a row of the tail
    if B > 4:
        q[4] = 0
    rows = K.normalize_rows(torch.from_numpy(host).to(dev))
    return rows, torch.from_numpy(q).to(dev), q


@pytest.mark.parametrize("case", INDEX_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-k{c[4]}")
def test_keyindex_with_retired_rows_behind_every_dispatch_class(K, dev, case):
    name, B, N, D, k = case
    rows, qd, q = _bank_rows(K, dev, case)
    W, k_in = K.padded_dim(D), k + 3
    if name == "fused":
        assert K.fused_helps(B, N, W, k_in)
    elif name == "small":
        assert K.small_helps(B, N, W, k_in)
    elif name == "filtered":
        assert K.filter_helps(B, N, W, k_in) and not K.small_helps(B, N, W, k_in) and not K.fused_helps(B, N, W, k_in)
    elif name == "wide":
        assert K.filter_wide_helps(B, N, W, k_in)
    host_rows = rows.cpu().numpy()

    def check(index, n, retired, what):
        """index.topk against a fresh index over a clone of the live rows of rows[:n], and 4 queries against the oracle"""
        live = np.setdiff1d(np.arange(n), retired)
        live_d = torch.from_numpy(live).to(dev)
        got = index.topk(qd, k, idx_base=3)
        fs, fi = K.KeyIndex(rows[live_d].clone()).topk(qd, k)
        _assert_same(got, (fs, live_d[fi] + 3), what)
        os_, oi = cref.topk_cosine(q[:4], np.ascontiguousarray(host_rows[live]), k)
        assert np.array_equal(got[1][:4].cpu().numpy(), live[oi] + 3), what
        assert np.array_equal(got[0][:4].cpu().numpy().view(np.int32), os_.view(np.int32)), what
        return got

    index = K.KeyIndex(rows[:N])
    first = index.topk(qd, k, idx_base=3)
    if name == "collapsed":
        assert isinstance(index._collapsed, tuple)
    best0 = int(first[1][0, 0]) - 3                           # the best hit of query 0
    copy1 = int(first[1][1, 0]) - 3                           # one copy of the duplicated row query 1 points at (the lowest)
    assert torch.equal(_bits(first[0][1, 0]), _bits(first[0][1, 1]))      # (its next copy scores the same bits)
    retired = sorted({best0, copy1})
    index.retire(retired)
    got = check(index, N, retired, "two sealed rows retired")
    assert best0 + 3 not in got[1][0].tolist() and int(got[1][1, 0]) == int(first[1][1, 1])   # the surviving copy moved up
    seen = index._queries
    index.extend(rows)
    assert (index.sealed_rows, index.tail_rows, index.retired_rows) == (N, 40, len(retired)) and index._queries == seen
    got = check(index, N + 40, retired, "40 rows appended")
    assert int(got[1][3, 0]) == N + 7 + 3                     # the new rows are live
    index.retire([N + 7])
    retired = retired + [N + 7]
    assert index.retired_rows == 3
    got = check(index, N + 40, retired, "a tail row retired")
    assert N + 7 + 3 not in got[1][3].tolist()
    if name == "collapsed":
        assert isinstance(index._collapsed, tuple)           # the groups of the sealed rows are still in use
    index.seal()
    assert (index.sealed_rows, index.tail_rows, index.retired_rows) == (N + 40, 0, 3)
    check(index, N + 40, retired, "after seal()")


# ---- ToyGraphBase end to end -------------------------------------------------------------------------------------------------
def _toy_bank(dev, data, rows=None, structure_weight=0.0):
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    tgb = ToyGraphBase(None, 3, 64, 3, device=dev)
    tgb.structure_weight = structure_weight
    tgb.add_resources(*((x if rows is None else x[rows].clone()) for x in data))
    return tgb


@pytest.mark.parametrize("structure_weight", [0.0, 0.001])
def test_toygraphbase_removes_rows_behind_a_live_index(K, dev, structure_weight):
    rng = np.random.default_rng(21)
    n, D, C, A, B = 5000, 64, 3, 10, 200
    data = (torch.from_numpy((rng.standard_normal((n, D)) * 2).astype(np.float32)).to(dev),
            torch.from_numpy(rng.standard_normal((n, D), dtype=np.float32)).to(dev),
            torch.from_numpy(np.eye(C, dtype=np.float32)[rng.integers(0, C, n)]).to(dev),
            torch.from_numpy(rng.random((n, A), dtype=np.float32)).to(dev))
    h = torch.from_numpy(rng.standard_normal((B, D), dtype=np.float32)).to(dev)
    hp = torch.from_numpy(rng.random((B, A), dtype=np.float32)).to(dev)
    kw = {"search_positions": hp} if structure_weight else {}
    tgb = _toy_bank(dev, data, structure_weight=structure_weight)
    _, _, idx0 = tgb.retrieve_reduced(h, 10, **kw)
    stores = tgb.resource_keys.data_ptr()

    def same_as_fresh(retired, what):
        live = np.setdiff1d(np.arange(n), retired)
        live_d = torch.from_numpy(live).to(dev)
        a = tgb.retrieve_reduced(h, 10, **kw)
        b = _toy_bank(dev, data, live_d, structure_weight).retrieve_reduced(h, 10, **kw)
        assert torch.equal(a[2], live_d[b[2]] if tgb.retired_rows else b[2]), what
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1])), what
        return live_d

    retired = sorted(set(idx0[:22, 0].tolist()))              # best hits
    retired += [int(r) for r in np.setdiff1d(np.arange(100), retired)[:22 - len(retired)]]
    tgb.remove_resources(torch.tensor(retired, device=dev))
    assert (tgb.retired_rows, tgb.num_resources, tgb.resource_keys.shape[0]) == (22, n - 22, n)
    same_as_fresh(retired, "22 rows retired")
    assert tgb.retired_rows == 22 and tgb.resource_keys.data_ptr() == stores      # k + 22 = 32: the same list class, no compaction
    extra = int(np.setdiff1d(np.arange(200, 300), retired)[0])
    tgb.remove_resources([extra])
    assert tgb.retired_rows == 23
    index = tgb._index
    live_d = same_as_fresh(retired + [extra], "the 23rd retired row compacts")    # k + 23 = 33 crosses the ceiling of 32
    assert tgb.retired_rows == 0 and tgb.resource_keys.shape[0] == n - 23 and tgb._index is index
    assert torch.equal(_bits(tgb.resource_values), _bits(data[1][live_d])) and torch.equal(_bits(tgb.resource_positions), _bits(data[3][live_d]))
    # compact() by hand: results unchanged up to the index map
    before = tgb.topk(h, 10, *( [hp] if structure_weight else []))
    gone = [int(x) for x in before[1][:3, 0].tolist()]
    tgb.remove_resources(gone)
    with_tombstones = tgb.topk(h, 10, *([hp] if structure_weight else []))
    pos = tgb.compact()
    assert pos.dtype == torch.int64 and pos.numel() == n - 23 - len(set(gone)) and tgb.compact() is None
    after = tgb.topk(h, 10, *([hp] if structure_weight else []))
    _assert_same((after[0], pos[after[1]]), with_tombstones, "after compact()")


def test_a_captured_topk_with_retired_rows_replays_and_never_compacts(K, dev):
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    rng = np.random.default_rng(23)
    N, D, k, B = 20000, 128, 10, 64
    rows = K.normalize_rows(torch.from_numpy(rng.standard_normal((N, D), dtype=np.float32)).to(dev))
    tgb = ToyGraphBase(None, 3, D, 3, device=dev)
    tgb.add_resources(rows, rows, torch.zeros(N, 3, device=dev))
    qs = [torch.from_numpy(rng.standard_normal((B, D), dtype=np.float32)).to(dev) for _ in range(3)]
    first = tgb.topk(qs[0], k)
    retired = sorted(set(first[1][:3, 0].tolist()))
    kn = tgb.keys_normalized.clone()                          # the bank's own normalised rows (it normalises what it is given)

    def fresh(q, gone):
        live_d = torch.from_numpy(np.setdiff1d(np.arange(N), gone)).to(dev)
        s, i = K.KeyIndex(kn[live_d].clone()).topk(q, k)
        return s, live_d[i]

    def captured(gone, what):
        _assert_same(tgb._index.topk(qs[0], k), fresh(qs[0], gone), f"{what}: eager")     # (warm: the copies exist before the capture)
        graph = torch.cuda.CUDAGraph()
        mode = torch.cuda.get_sync_debug_mode()
        static_q = qs[0].clone()
        with torch.no_grad(), torch.cuda.graph(graph):
            torch.cuda.set_sync_debug_mode("error")
            try:
                cap_s, cap_i = tgb.topk(static_q, k)
            finally:
                torch.cuda.set_sync_debug_mode(mode)
        assert (tgb.retired_rows, tgb.resource_keys.shape[0]) == (len(gone), N), what     # no compaction under capture
        for q in qs[1:]:                                      # replayed twice, on new queries
            static_q.copy_(q)
            graph.replay()
            torch.cuda.synchronize()
            _assert_same((cap_s, cap_i), fresh(q, gone), f"{what}: replay")

    tgb.remove_resources(retired)
    captured(retired, "3 retired rows")
    # past the class ceiling (k + 23 = 33): an eager ToyGraphBase.topk would compact, a captured one over-fetches and does not
    retired = retired + [int(r) for r in np.setdiff1d(np.arange(500, 600), retired)[:23 - len(retired)]]
    tgb.remove_resources(retired)
    assert tgb.retired_rows == 23
    captured(retired, "23 retired rows")
    tgb.topk(qs[0], k)                                        # the next eager call compacts
    assert (tgb.retired_rows, tgb.resource_keys.shape[0]) == (0, N - 23)
