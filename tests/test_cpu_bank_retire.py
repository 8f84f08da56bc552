"""A shrinking bank on the CPU: KeyIndex.retire / rebase / overfetch_keeps_class, and ToyGraphBase.remove_resources / compact.

The kernels are answered by the C checker (oracle/cref.py) on torch CPU tensors, in the style of TailOps in
tests/test_cpu_bank_tail.py, plus numpy restatements of the two new entries (ragraph_topk_drop_rows_f32,
ragraph_rows_retire_u32) written here.  Every comparison is bit for bit (scores as int32 views, indices equal) against
cref.topk_cosine over the LIVE rows only, indices mapped through the live positions and idx_base added -- what a fresh index
over the surviving rows returns."""
import copy

import numpy as np
import pytest
import torch

from oracle import cref
from ragraph_amd._native import TOPK_ORDERED_MAX, RagraphNativeError
from ragraph_amd.kernels_index import KeyIndex

I64_MAX = np.iinfo(np.int64).max


def np_retire_rows(bitmap, rows, n_rows):
    """ragraph_rows_retire_u32: OR the bits of the ids inside [0, n_rows) into the uint32 words."""
    for r in np.asarray(rows, dtype=np.int64).reshape(-1):
        if 0 <= r < n_rows:
            bitmap[r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    return bitmap


def np_drop_rows(scores, idx, bitmap, n_rows, k_out, idx_base=0):
    """ragraph_topk_drop_rows_f32: per list the entries whose row has its bit clear, in order, the first k_out; padding and
    rows outside [0, n_rows) dropped; short lists padded and counted."""
    B, k_in = scores.shape
    assert 1 <= k_out <= k_in <= TOPK_ORDERED_MAX and n_rows >= 1
    out_s = np.full((B, k_out), -np.inf, dtype=np.float32)
    out_i = np.full((B, k_out), I64_MAX, dtype=np.int64)
    short = 0
    for b in range(B):
        n = 0
        for e in range(k_in):
            r = int(idx[b, e]) - idx_base
            if n < k_out and 0 <= r < n_rows and not (int(bitmap[r >> 5]) >> (r & 31)) & 1:
                out_s[b, n], out_i[b, n] = scores[b, e], idx[b, e]
                n += 1
        short += n < k_out
    return out_s, out_i, short


class PlainOps:
    @staticmethod
    def topk_cosine(q, kn, k, idx_base=0):
        s, i = cref.topk_cosine(q.numpy(), kn.numpy(), k, idx_base)
        return torch.from_numpy(s), torch.from_numpy(i)


class RetireOps(PlainOps):
    """+ the seeded tail pass (as TailOps restates it) and the two new entries; every call of either is counted."""

    TOPK_TAIL_MAX = 65536
    drop_calls = retire_calls = 0
    last_k_in = None

    @staticmethod
    def topk_cosine_tail(q, keys_tail, seed_s, seed_i, idx_base_tail):
        B, k = seed_s.shape
        T = keys_tail.shape[0]
        ts = np.full((B, k), -np.inf, dtype=np.float32)
        ti = np.full((B, k), I64_MAX, dtype=np.int64)
        kt = min(k, T)
        ts[:, :kt], ti[:, :kt] = cref.topk_cosine(q.numpy(), keys_tail.numpy(), kt, idx_base_tail)
        s, i = cref.topk_merge(np.stack([seed_s.numpy(), ts]), np.stack([seed_i.numpy(), ti]))
        return torch.from_numpy(s), torch.from_numpy(i)

    @staticmethod
    def retire_rows(bitmap, rows, n_rows):
        RetireOps.retire_calls += 1
        assert bitmap.dtype == torch.int32 and bitmap.numel() * 32 >= n_rows
        np_retire_rows(bitmap.numpy().view(np.uint32), rows.numpy(), n_rows)   # (in place: the view shares the tensor's memory)
        return bitmap

    @staticmethod
    def topk_drop_rows(scores, idx, bitmap, n_rows, k_out, idx_base=0):
        RetireOps.drop_calls += 1
        RetireOps.last_k_in = scores.shape[1]
        s, i, short = np_drop_rows(scores.numpy(), idx.numpy(), bitmap.numpy().view(np.uint32), n_rows, k_out, idx_base)
        return torch.from_numpy(s), torch.from_numpy(i), torch.tensor([short], dtype=torch.int32)


class PaddedRetireOps(RetireOps):
    @staticmethod
    def padded_dim(D):
        return next((w for w in (64, 128, 256) if D <= w), None)

    @staticmethod
    def pad_cols(x, width):
        if x.shape[1] == width:
            return x
        out = x.new_zeros((x.shape[0], width))
        out[:, :x.shape[1]] = x
        return out


def _rows(rng, n, D):
    return cref.normalize_rows(rng.standard_normal((n, D), dtype=np.float32))


def _want(q, rows, retired, k, base=0):
    """cref.topk_cosine over the live rows, mapped through the live positions."""
    live = np.setdiff1d(np.arange(rows.shape[0]), np.asarray(retired, dtype=np.int64))
    s, i = cref.topk_cosine(q, np.ascontiguousarray(rows[live]), k)
    return s, live[i] + base


def _same(got, want):
    gs, gi = got[0].numpy(), got[1].numpy()
    assert np.array_equal(gi, want[1])
    assert np.array_equal(gs.view(np.int32), want[0].view(np.int32))


def _bitmap_ids(index):
    words = index.retired_bitmap.numpy().view(np.uint32)
    return [r for r in range(words.size * 32) if (int(words[r >> 5]) >> (r & 31)) & 1]


def test_restated_entries_on_a_hand_made_list():
    bm = np.zeros(2, dtype=np.uint32)
    np_retire_rows(bm, [31, 32, 32, 40, 99, -1], 40)           # 40, 99, -1: outside [0, 40)
    assert bm.tolist() == [1 << 31, 1]
    s = np.array([[5, 4, 3, 2, -np.inf]], dtype=np.float32)
    i = np.array([[3 + 31, 3 + 7, 3 + 32, 3 + 50, I64_MAX]], dtype=np.int64)
    os_, oi, short = np_drop_rows(s, i, bm, 40, 2, idx_base=3)   # row 50 is outside the bank, the last entry is padding
    assert oi.tolist() == [[10, I64_MAX]] and os_[0, 0] == 4 and np.isneginf(os_[0, 1]) and short == 1


def test_retire_on_a_plain_bank():
    rng = np.random.default_rng(0)
    rows = _rows(rng, 900, 64)
    rows[201] = rows[202] = rows[200]                 # one row stored three times
    q = rng.standard_normal((6, 64), dtype=np.float32)
    q[0] = rows[200] * 2.0
    index = KeyIndex(torch.from_numpy(rows), ops=RetireOps)
    qt = torch.from_numpy(q)
    s0, i0 = index.topk(qt, 10, idx_base=5)
    _same((s0, i0), cref.topk_cosine(q, rows, 10, 5))
    assert (index.retired_rows, index.live_rows) == (0, 900)
    index.retire([])                                  # nothing: no bitmap, no call
    assert index.retired_rows == 0 and index.retired_bitmap is None
    best = sorted(set((i0[1:, 0] - 5).tolist()))      # the best hit of queries 1..5
    index.retire(torch.tensor(best))
    _same(index.topk(qt, 10, idx_base=5), _want(q, rows, best, 10, 5))
    retired = best + [200, 202]                       # both copies of the duplicated row but one: 201 answers for them
    index.retire(np.array([200, 202]))
    got = index.topk(qt, 10, idx_base=5)
    _same(got, _want(q, rows, retired, 10, 5))
    assert int(got[1][0, 0]) == 201 + 5
    calls = RetireOps.retire_calls
    index.retire([200, best[0], 200])                 # twice: a no-op
    assert RetireOps.retire_calls == calls and index.retired_rows == len(retired)
    assert index.retired_ids.tolist() == sorted(retired) == _bitmap_ids(index)
    assert index.live_rows == 900 - len(retired)
    before = (index.retired_ids.clone(), index.retired_bitmap.clone())
    for bad in ([900], [3, -1], torch.tensor([0, 10 ** 12])):
        with pytest.raises(IndexError):
            index.retire(bad)
    assert torch.equal(index.retired_ids, before[0]) and torch.equal(index.retired_bitmap, before[1])
    assert RetireOps.last_k_in == 10 + len(retired)
    _same(index.topk(qt, 10, idx_base=5), _want(q, rows, retired, 10, 5))


def test_retire_together_with_a_tail():
    rng = np.random.default_rng(1)
    rows = _rows(rng, 880, 64)
    q = rng.standard_normal((5, 64), dtype=np.float32)
    q[0], q[1], q[2] = rows[805], rows[839] * 3.0, rows[850]
    qt = torch.from_numpy(q)
    index = KeyIndex(torch.from_numpy(rows[:800]), ops=RetireOps)
    index.extend(torch.from_numpy(rows[:840]))
    assert index.tail_rows == 40
    retired = [805, 839, 17]                          # two rows of the tail (the best hits of queries 0 and 1), one sealed row
    index.retire(retired)
    assert index.retired_bitmap.numel() == 27
    _same(index.topk(qt, 10), _want(q, rows[:840], retired, 10))
    assert (index.sealed_rows, index.tail_rows) == (800, 40)
    # retire, then extend: the bitmap grows with zero bits and the new rows are live
    index.extend(torch.from_numpy(rows))
    assert index.tail_rows == 80 and index.retired_bitmap.numel() >= 28
    assert _bitmap_ids(index) == sorted(retired) == index.retired_ids.tolist()
    got = index.topk(qt, 10)
    _same(got, _want(q, rows, retired, 10))
    assert int(got[1][2, 0]) == 850
    # retire, then seal
    index.retire([850])
    index.seal()
    assert (index.sealed_rows, index.tail_rows, index.retired_rows) == (880, 0, 4)
    _same(index.topk(qt, 10), _want(q, rows, retired + [850], 10))


def test_small_and_padded_banks():
    rng = np.random.default_rng(2)
    rows = _rows(rng, 20, 64)
    q = rng.standard_normal((4, 64), dtype=np.float32)
    qt = torch.from_numpy(q)
    index = KeyIndex(torch.from_numpy(rows), ops=RetireOps)
    retired = [0, 3, 4, 11, 19]
    index.retire(retired)
    _same(index.topk(qt, 15), _want(q, rows, retired, 15))     # k + r = the physical rows: every row is in the list
    assert RetireOps.last_k_in == 20
    for k in (16, 20, 21):                                     # k + r beyond the physical rows is k beyond the live rows
        with pytest.raises(RagraphNativeError):
            index.topk(qt, k)
    # a tail that the over-fetch outgrows: k + r > sealed_rows seals, as a too-large k does
    index = KeyIndex(torch.from_numpy(rows[:18]), ops=RetireOps)
    index.extend(torch.from_numpy(rows))
    index.retire([1, 2, 19])
    assert index.tail_rows == 2
    _same(index.topk(qt, 16), _want(q, rows, [1, 2, 19], 16))
    assert (index.sealed_rows, index.tail_rows) == (20, 0)
    # a padded width (the index owns the padded matrix; the tail pass and the drop see padded rows and plain indices)
    rows = _rows(rng, 840, 100)
    q = rng.standard_normal((4, 100), dtype=np.float32)
    q[0], q[1] = rows[830], rows[5]
    index = KeyIndex(torch.from_numpy(rows[:800]), ops=PaddedRetireOps)
    index.extend(torch.from_numpy(rows))
    index.retire([830, 5, 6])
    _same(index.topk(torch.from_numpy(q), 10, idx_base=9), _want(q, rows, [830, 5, 6], 10, 9))
    assert tuple(index.keys_normalized.shape) == (840, 128)


def test_refusals():
    rng = np.random.default_rng(3)
    rows = torch.from_numpy(_rows(rng, 5000, 8))
    q = torch.from_numpy(rng.standard_normal((2, 8), dtype=np.float32))
    index = KeyIndex(rows, ops=PlainOps)                       # no topk_drop_rows entry
    with pytest.raises(RagraphNativeError):
        index.retire([1])
    assert index.retired_rows == 0
    index = KeyIndex(rows, ops=RetireOps)
    index.retire([7])
    with pytest.raises(RagraphNativeError, match="sharded"):   # a shard of a sharded bank
        index.topk(q, 5, exchange=lambda *_: None)
    index.retire(np.arange(100, 100 + TOPK_ORDERED_MAX - 10))  # k + r = TOPK_ORDERED_MAX + 1 at k = 10
    assert index.retired_rows == TOPK_ORDERED_MAX - 9
    with pytest.raises(RagraphNativeError, match="compact"):
        index.topk(q, 10)
    index.topk(q, 9)


def test_overfetch_keeps_class_at_its_edges():
    rows = torch.from_numpy(_rows(np.random.default_rng(4), 400, 8))

    def keeps(k, r):
        index = KeyIndex(rows, ops=RetireOps)
        index.retire(list(range(r)))
        assert index.retired_rows == r
        return index.overfetch_keeps_class(k)

    assert keeps(10, 0) and keeps(10, 22) and not keeps(10, 23)        # 32
    assert keeps(41, 23) and not keeps(41, 24)                         # TOPK_MAX = 64
    # k = 64 is itself the last list under TOPK_MAX: any retired row moves it on, to TOPK_FILTER_MAX = 128 (r = 64) or past it (65)
    assert keeps(64, 0) and not keeps(64, 1) and not keeps(64, 64) and not keeps(64, 65)
    assert keeps(65, 63) and not keeps(65, 64)                         # TOPK_FILTER_MAX = 128
    assert keeps(129, 200) and not keeps(32, 1) and keeps(33, 1)
    index = KeyIndex(rows, ops=RetireOps)
    index.retire(list(range(23)))
    assert index.overfetch_keeps_class(41, (32, TOPK_ORDERED_MAX))     # another search's ceilings: 41 and 64 both lie above 32
    assert not index.overfetch_keeps_class(10, (32, TOPK_ORDERED_MAX))


def test_nothing_retired_makes_no_drop_call_and_no_bitmap():
    rng = np.random.default_rng(5)
    rows = _rows(rng, 840, 64)
    q = torch.from_numpy(rng.standard_normal((3, 64), dtype=np.float32))
    index = KeyIndex(torch.from_numpy(rows[:800]), ops=RetireOps)
    drops, retires = RetireOps.drop_calls, RetireOps.retire_calls
    index.topk(q, 10)
    index.extend(torch.from_numpy(rows))
    index.topk(q, 10)
    index.seal()
    index.topk(q, 70)
    index.retire([])
    assert (RetireOps.drop_calls, RetireOps.retire_calls) == (drops, retires)
    assert index.retired_bitmap is None and index._retired is None
    index.retire([3])
    index.topk(q, 10)
    assert (RetireOps.drop_calls, RetireOps.retire_calls) == (drops + 1, retires + 1)    # ONE drop per call


def test_rebase_drops_what_the_rows_made_and_the_priors_and_keeps_the_verdicts():
    rng = np.random.default_rng(6)
    rows = _rows(rng, 840, 100)
    index = KeyIndex(torch.from_numpy(rows[:800]), ops=PaddedRetireOps)
    index.extend(torch.from_numpy(rows))
    index.retire([4, 820])
    index._bf16, index._packed, index._collapsed = "bf16", "packed", False
    index._i8_ok, index.i8_classes = True, {"err": 0.01}
    index._spec[12] = {"hist": [(0.3, 0.4)], "queries": 99, "off_at": None, "after": 1 << 20, "cand": 100.0, "failed": 0,
                       "used": 1, "tight_margin": 0.004}
    index._pending = ("word", "event", 5, False, 12)
    index._i8_off, index._filter_off, index._queries, index._overflowed = True, True, 777, 3
    index._demoted = {"i8": 5, "filter": 6}
    index._reprobe_after = {"i8": 1 << 22, "filter": 1 << 24}
    index._probed_at = {"i8": 1, "filter": 2}
    kept = copy.deepcopy((index._i8_off, index._filter_off, index._demoted, index._reprobe_after, index._probed_at,
                          index._queries, index._overflowed))
    live = np.setdiff1d(np.arange(840), [4, 820])
    index.rebase(torch.from_numpy(rows[live]))
    assert (index.sealed_rows, index.tail_rows, index.retired_rows, index.live_rows) == (838, 0, 0, 838)
    assert index._bf16 is None and index._packed is None and index._i8_ok is None and index.i8_classes is None
    assert index._collapsed is None and index._retired is None and index.retired_bitmap is None
    assert index._spec == {} and index._pending is None
    assert kept == (index._i8_off, index._filter_off, index._demoted, index._reprobe_after, index._probed_at,
                    index._queries, index._overflowed)
    assert tuple(index.keys_normalized.shape) == (838, 128) and index._store is index.keys_normalized      # padded anew
    assert np.array_equal(index.keys_normalized[:, :100].numpy().view(np.int32), rows[live].view(np.int32))
    q = rng.standard_normal((3, 100), dtype=np.float32)
    _same(index.topk(torch.from_numpy(q), 10), cref.topk_cosine(q, np.ascontiguousarray(rows[live]), 10))
    with pytest.raises(ValueError):
        index.rebase(torch.from_numpy(_rows(rng, 10, 64)))
    no_dedup = KeyIndex(torch.from_numpy(rows), ops=PaddedRetireOps, dedup=False)
    no_dedup.rebase(torch.from_numpy(rows[live]))
    assert no_dedup._collapsed is False


# ---- ToyGraphBase on the shim ---------------------------------------------------------------------------------------------
D, C, A, N0 = 16, 3, 10, 300


def _mix(q, kn, pos_q, pn, w_struct, w_sem, k, idx_base=0):
    """K.topk_cosine_mix restated with the checker: linear x 2 + axpby + topk_rows on the materialised matrices."""
    s_struct = cref.cosine_scores(cref.normalize_rows(pos_q.numpy()), pn.numpy())
    s_sem = cref.cosine_scores(cref.normalize_rows(q.numpy()), kn.numpy())
    s, i = cref.topk_rows(cref.axpby(s_struct, w_struct, s_sem, w_sem), k)
    return torch.from_numpy(s), torch.from_numpy(i.astype(np.int64) + idx_base)


@pytest.fixture
def shim(monkeypatch):
    from ragraph_amd import kernels as K

    def normalize_rows(x, out=None):
        r = torch.from_numpy(cref.normalize_rows(x.numpy()))
        if out is None:
            return r
        out.copy_(r)
        return out

    monkeypatch.setattr(K, "normalize_rows", normalize_rows)
    monkeypatch.setattr(K, "gather_rows", lambda v, idx, idx_base=0: v[idx - idx_base].clone())
    monkeypatch.setattr(K, "mask_positions", lambda m: torch.nonzero(m).reshape(-1))
    monkeypatch.setattr(K, "topk_cosine_mix", _mix)
    monkeypatch.setattr(K, "topk_drop_rows", RetireOps.topk_drop_rows)
    return K


def _bank_data(seed):
    rng = np.random.default_rng(seed)
    keys = (rng.standard_normal((N0, D)) * 3).astype(np.float32)
    values = rng.standard_normal((N0, D), dtype=np.float32)
    labels = np.eye(C, dtype=np.float32)[rng.integers(0, C, N0)]
    pos = rng.random((N0, A), dtype=np.float32)
    q = rng.standard_normal((5, D), dtype=np.float32)
    q[0] = keys[7]
    return keys, values, labels, pos, q, rng.random((5, A), dtype=np.float32)


def _bank(K, data, with_index=True, structure_weight=0.0):
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    keys, values, labels, pos = (torch.from_numpy(x) for x in data[:4])
    tgb = ToyGraphBase(None, C, D, 3, device="cpu")
    tgb.structure_weight = structure_weight
    tgb.add_resources(keys, values, labels, pos)
    if with_index:
        tgb.positions_normalized
        tgb._index = K.KeyIndex(tgb.keys_normalized, ops=RetireOps)
    return tgb


def _bits_equal(t, a):
    return np.array_equal(t.numpy().view(np.int32), np.ascontiguousarray(a).view(np.int32))


def test_toygraphbase_retires_then_compacts(shim):
    data = _bank_data(10)
    keys, values, labels, pos, q, _ = data
    tgb = _bank(shim, data)
    index = tgb._index
    retired = [3, 7, 250]
    with pytest.raises(IndexError):
        tgb.remove_resources([5, N0])
    assert tgb.retired_rows == 0
    tgb.remove_resources(retired)
    tgb.remove_resources([7])
    assert (tgb.num_resources, tgb.retired_rows, tgb.resource_keys.shape[0]) == (N0 - 3, 3, N0)   # resource_* stay physical
    kn = cref.normalize_rows(keys)
    want = _want(q, kn, retired, 4)
    got = tgb.topk(torch.from_numpy(q), 4)
    _same(got, want)
    assert 7 not in got[1][0].tolist()
    with pytest.raises(RuntimeError, match="out of range"):
        tgb.topk(torch.from_numpy(q), N0 - 2)                # the live count decides
    live = np.setdiff1d(np.arange(N0), retired)
    pos_live = tgb.compact()
    assert pos_live.dtype == torch.int64 and np.array_equal(pos_live.numpy(), live)
    assert tgb.compact() is None                             # nothing retired any more
    assert (tgb.num_resources, tgb.retired_rows, tgb.resource_keys.shape[0]) == (N0 - 3, 0, N0 - 3)
    for got_t, raw in ((tgb.resource_keys, keys), (tgb.resource_values, values), (tgb.resource_labels, labels),
                       (tgb.resource_positions, pos)):
        assert _bits_equal(got_t, raw[live])
    assert _bits_equal(tgb.keys_normalized, cref.normalize_rows(keys[live]))
    assert _bits_equal(tgb.positions_normalized, cref.normalize_rows(pos[live]))
    assert tgb._index is index and index.keys_normalized is tgb._keys_normalized
    assert (index.sealed_rows, index.tail_rows, index.retired_rows) == (N0 - 3, 0, 0)
    after = tgb.topk(torch.from_numpy(q), 4)                 # unchanged up to the index map
    assert np.array_equal(live[after[1].numpy()], want[1]) and np.array_equal(after[0].numpy().view(np.int32), want[0].view(np.int32))
    # the bank grows again behind the compacted stores
    tgb.add_resources(*(torch.from_numpy(x[:40]) for x in (keys, values, labels, pos)))
    assert tgb.num_resources == N0 + 37 and _bits_equal(tgb.keys_normalized[-40:], kn[:40])


def test_toygraphbase_without_caches_compacts_at_once(shim):
    data = _bank_data(11)
    tgb = _bank(shim, data, with_index=False)
    tgb.remove_resources([0, 299, 150])
    live = np.setdiff1d(np.arange(N0), [0, 150, 299])
    assert tgb._index is None and tgb._keys_normalized is None and tgb.retired_rows == 0
    assert tgb.num_resources == N0 - 3 == tgb.resource_keys.shape[0]
    assert _bits_equal(tgb.resource_keys, data[0][live]) and _bits_equal(tgb.resource_positions, data[3][live])


def test_save_and_load_hold_live_rows_only(shim, tmp_path):
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    data = _bank_data(12)
    tgb = _bank(shim, data)
    tgb.remove_resources([1, 2, 200])
    live = np.setdiff1d(np.arange(N0), [1, 2, 200])
    path = str(tmp_path / "bank.pt")
    tgb.save(path)
    assert tgb.retired_rows == 0 and tgb.resource_keys.shape[0] == N0 - 3      # save compacted
    other = ToyGraphBase(None, C, D, 3, device="cpu")
    other.load(path)
    for name, raw in zip(("resource_keys", "resource_values", "resource_labels", "resource_positions"), data[:4]):
        assert _bits_equal(getattr(other, name), raw[live])
    assert other.retired_rows == 0
    # load without append and set_resources start clean
    tgb.remove_resources([0])
    assert tgb.retired_rows == 1
    tgb.load(path)
    assert tgb.retired_rows == 0 and tgb.num_resources == N0 - 3
    tgb.keys_normalized
    tgb._index = shim.KeyIndex(tgb.keys_normalized, ops=RetireOps)
    tgb.remove_resources([0])
    tgb.set_resources(*(torch.from_numpy(x[:50]) for x in data[:3]))
    assert tgb.retired_rows == 0 and tgb.num_resources == 50


def test_noisy_paths_compact_first(shim, monkeypatch):
    data = _bank_data(13)
    q = torch.from_numpy(data[4])
    tgb = _bank(shim, data)
    tgb.remove_resources([3, 7])
    idx = tgb.retrieve_indices(q, add_noise=True)
    assert tgb.retired_rows == 0 and tgb.resource_keys.shape[0] == N0 - 2
    assert idx.shape[1] == 2 * tgb.retrieve_num + tgb.noise_retrieve_num and int(idx.max()) < N0 - 2
    tgb.remove_resources([5])
    seen = []
    monkeypatch.setattr(shim, "gather_reduce", lambda v, l, idx, *a, **kw: seen.append((v.shape[0], int(idx.max()))) or (None, None))
    tgb.retrieve_reduced_noisy(q)
    assert tgb.retired_rows == 0 and seen == [(N0 - 3, seen[0][1])] and seen[0][1] < N0 - 3
    # without noise nothing compacts
    tgb.remove_resources([5])
    tgb.retrieve_indices(q, add_noise=False)
    assert tgb.retired_rows == 1 and tgb.resource_keys.shape[0] == N0 - 3


def test_mixed_branch_drops_retired_rows(shim):
    data = _bank_data(14)
    keys, _, _, pos, q, qpos = data
    tgb = _bank(shim, data, structure_weight=0.001)
    qt, pt = torch.from_numpy(q), torch.from_numpy(qpos)
    first = tgb.topk(qt, 4, pt)
    retired = sorted(set(first[1][:, 0].tolist()) | {250})       # every query's best hit
    tgb.remove_resources(retired)
    live = np.setdiff1d(np.arange(N0), retired)
    ws, wi = _mix(qt, torch.from_numpy(cref.normalize_rows(keys[live])), pt, torch.from_numpy(cref.normalize_rows(pos[live])),
                  0.001, tgb.semantic_weight, 4)
    drops = RetireOps.drop_calls
    got = tgb.topk(qt, 4, pt)
    assert RetireOps.drop_calls == drops + 1 and tgb.retired_rows == len(retired)
    assert np.array_equal(got[1].numpy(), live[wi.numpy()]) and np.array_equal(got[0].numpy().view(np.int32), ws.numpy().view(np.int32))
    # the class rule at this branch's fused limit of 32: k = 10 compacts at the 23rd retired row, not at the 22nd
    more = [int(r) for r in live[:22 - len(retired)]]
    tgb.remove_resources(more)
    assert tgb.retired_rows == 22
    tgb.topk(qt, 10, pt)
    assert tgb.retired_rows == 22
    tgb.remove_resources([int(live[-1])])
    got = tgb.topk(qt, 10, pt)
    assert tgb.retired_rows == 0 and tgb.resource_keys.shape[0] == N0 - 23
    gone = np.array(sorted(retired + more + [int(live[-1])]))
    live = np.setdiff1d(np.arange(N0), gone)
    ws, wi = _mix(qt, torch.from_numpy(cref.normalize_rows(keys[live])), pt, torch.from_numpy(cref.normalize_rows(pos[live])),
                  0.001, tgb.semantic_weight, 10)
    assert np.array_equal(got[1].numpy(), wi.numpy()) and np.array_equal(got[0].numpy().view(np.int32), ws.numpy().view(np.int32))
