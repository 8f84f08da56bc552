"""A growing bank on the CPU: KeyIndex.extend / seal / the sealing rule, and ToyGraphBase's caches that grow with the bank.

The kernels are answered by the C checker (oracle/cref.py) on torch CPU tensors, in the style of
tests/test_cpu_distributed.py::OracleOps; every comparison is bit for bit (scores as int32 views) against cref.topk_cosine
over ALL rows -- what a fresh index over the grown bank returns."""
import copy

import numpy as np
import pytest
import torch

from oracle import cref
from ragraph_amd.kernels_index import KeyIndex

I64_MAX = np.iinfo(np.int64).max


class PlainOps:
    """No tail entry: what the CPU shims of the older tests are."""

    @staticmethod
    def topk_cosine(q, kn, k, idx_base=0):
        s, i = cref.topk_cosine(q.numpy(), kn.numpy(), k, idx_base)
        return torch.from_numpy(s), torch.from_numpy(i)


class TailOps(PlainOps):
    """+ ragraph_topk_cosine_tail_f32 restated with the checker: the tail's own canonical list, merged with the seed."""

    TOPK_TAIL_MAX = 65536
    tail_calls = 0

    @classmethod
    def topk_cosine_tail(cls, q, keys_tail, seed_s, seed_i, idx_base_tail):
        TailOps.tail_calls += 1
        B, k = seed_s.shape
        T = keys_tail.shape[0]
        assert 1 <= T <= cls.TOPK_TAIL_MAX
        assert bool((seed_i[seed_i != I64_MAX] < idx_base_tail).all())
        ts = np.full((B, k), -np.inf, dtype=np.float32)
        ti = np.full((B, k), I64_MAX, dtype=np.int64)
        kt = min(k, T)
        ts[:, :kt], ti[:, :kt] = cref.topk_cosine(q.numpy(), keys_tail.numpy(), kt, idx_base_tail)
        s, i = cref.topk_merge(np.stack([seed_s.numpy(), ts]), np.stack([seed_i.numpy(), ti]))
        return torch.from_numpy(s), torch.from_numpy(i)


class PaddedTailOps(TailOps):
    """+ the width rule of ragraph_amd.kernels (padded_dim / pad_cols)."""

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


def _same(got, want):
    gs, gi = got[0].numpy(), got[1].numpy()
    assert np.array_equal(gi, want[1])
    assert np.array_equal(gs.view(np.int32), want[0].view(np.int32))


def test_extend_keeps_the_index_and_what_it_learnt():
    rng = np.random.default_rng(0)
    rows = _rows(rng, 900, 64)
    q = torch.from_numpy(rng.standard_normal((5, 64), dtype=np.float32))
    index = KeyIndex(torch.from_numpy(rows[:800]), ops=TailOps)
    index.topk(q, 10)
    index._spec[10] = {"hist": [(0.31, 0.42)], "queries": 640, "off_at": None, "after": 1 << 20, "cand": 120.0, "failed": 0,
                       "used": 3}
    index._i8_off, index._filter_off = True, True
    index._demoted = {"i8": 123, "filter": 456}
    index._pending = ("word", "event", 5, False, 10)
    before = copy.deepcopy((index._spec, index._queries, index._i8_off, index._filter_off, index._demoted,
                            index._reprobe_after, index._probed_at, index._overflowed, index._seen_i8, index._seen_bf16))
    grown = torch.from_numpy(rows[:840])
    index.extend(grown)
    assert (index.sealed_rows, index.tail_rows) == (800, 40)
    assert index.keys_normalized is grown          # an unpadded bank: the caller's own matrix, no copy
    assert before == (index._spec, index._queries, index._i8_off, index._filter_off, index._demoted, index._reprobe_after,
                      index._probed_at, index._overflowed, index._seen_i8, index._seen_bf16)
    assert index._pending == ("word", "event", 5, False, 10)
    index._pending = None
    _same(index.topk(q, 10), cref.topk_cosine(q.numpy(), rows[:840], 10))
    with pytest.raises(ValueError):
        index.extend(torch.from_numpy(rows[:700]))           # shorter than what the index holds
    with pytest.raises(ValueError):
        index.extend(torch.from_numpy(_rows(rng, 900, 32)))  # another width


def test_sealing_rule_at_its_edges(monkeypatch):
    rng = np.random.default_rng(1)
    rows = torch.from_numpy(_rows(rng, 1000, 64))
    q = torch.from_numpy(rng.standard_normal((3, 64), dtype=np.float32))
    assert KeyIndex.TAIL_DIVISOR == 8
    # sealed_rows // TAIL_DIVISOR = 100 rows: exactly at the limit stays a tail, one more row seals
    index = KeyIndex(rows[:800], ops=TailOps)
    index.extend(rows[:900])
    assert (index.sealed_rows, index.tail_rows) == (800, 100)
    index.extend(rows[:901])
    assert (index.sealed_rows, index.tail_rows) == (901, 0)
    # TAIL_MAX_ROWS, when it is the smaller of the two
    index = KeyIndex(rows[:800], ops=TailOps)
    index.TAIL_MAX_ROWS = 50
    index.extend(rows[:850])
    assert index.tail_rows == 50
    index.extend(rows[:851])
    assert (index.sealed_rows, index.tail_rows) == (851, 0)
    # checked again at the start of topk (the limit may have moved since extend)
    index = KeyIndex(rows[:800], ops=TailOps)
    index.extend(rows[:860])
    index.TAIL_MAX_ROWS = 50
    _same(index.topk(q, 5), cref.topk_cosine(q.numpy(), rows[:860].numpy(), 5))
    assert (index.sealed_rows, index.tail_rows) == (860, 0)
    # a 40-row bank that receives 40 more re-seals at once
    index = KeyIndex(rows[:40], ops=TailOps)
    index.extend(rows[:80])
    assert (index.sealed_rows, index.tail_rows) == (80, 0)
    # k > sealed_rows seals (the sealed search could not fill its list)
    index = KeyIndex(rows[:20], ops=TailOps)
    index.extend(rows[:22])
    assert index.tail_rows == 2
    _same(index.topk(q, 21), cref.topk_cosine(q.numpy(), rows[:22].numpy(), 21))
    assert (index.sealed_rows, index.tail_rows) == (22, 0)
    # an ops object without the entry seals on extend
    index = KeyIndex(rows[:800], ops=PlainOps)
    index.extend(rows[:840])
    assert (index.sealed_rows, index.tail_rows) == (840, 0)
    _same(index.topk(q, 5), cref.topk_cosine(q.numpy(), rows[:840].numpy(), 5))
    # one shard of a sharded bank (exchange) seals first
    index = KeyIndex(rows[:800], ops=TailOps)
    index.extend(rows[:840])
    assert index.tail_rows == 40
    _same(index.topk(q, 5, exchange=lambda *_: None), cref.topk_cosine(q.numpy(), rows[:840].numpy(), 5))
    assert (index.sealed_rows, index.tail_rows) == (840, 0)
    # RAGRAPH_BANK_TAIL=0: extend seals immediately
    monkeypatch.setenv("RAGRAPH_BANK_TAIL", "0")
    index = KeyIndex(rows[:800], ops=TailOps)
    index.extend(rows[:840])
    assert (index.sealed_rows, index.tail_rows) == (840, 0)


def test_seal_drops_what_the_rows_made_and_keeps_what_the_queries_taught():
    rng = np.random.default_rng(2)
    rows = torch.from_numpy(_rows(rng, 840, 64))
    index = KeyIndex(rows[:800], ops=TailOps)
    index.extend(rows)
    index._bf16, index._packed, index._collapsed = "bf16", "packed", False
    index._i8_ok, index.i8_classes = True, {"err": 0.01}
    index._spec[10] = {"hist": [(0.3, 0.4)], "queries": 99, "off_at": None, "after": 1 << 20, "cand": 100.0, "failed": 0,
                       "used": 1, "tight_margin": 0.004}
    index._i8_off, index._filter_off, index._queries, index._overflowed = True, True, 777, 3
    index._demoted = {"i8": 5, "filter": 6}
    index._reprobe_after = {"i8": 1 << 22, "filter": 1 << 24}
    index._probed_at = {"i8": 1, "filter": 2}
    kept = copy.deepcopy((index._spec, index._i8_off, index._filter_off, index._demoted, index._reprobe_after,
                          index._probed_at, index._queries, index._overflowed))
    index.seal()
    assert (index.sealed_rows, index.tail_rows) == (840, 0)
    assert index._bf16 is None and index._packed is None and index._i8_ok is None and index.i8_classes is None
    assert index._collapsed is None          # back to undecided: the duplicates are judged again over all rows
    assert kept == (index._spec, index._i8_off, index._filter_off, index._demoted, index._reprobe_after, index._probed_at,
                    index._queries, index._overflowed)
    no_dedup = KeyIndex(rows[:800], ops=TailOps, dedup=False)
    no_dedup.extend(rows)
    no_dedup.seal()
    assert no_dedup._collapsed is False      # (an index that was told not to look for duplicates still does not)


def _grown_case(name, rng):
    """(sealed rows, tail rows, queries, k, idx_base, D)"""
    D, k, base = 64, 10, 0
    if name == "padded width":
        D = 100
    sealed = _rows(rng, 800, D)
    tail = _rows(rng, 40, D)
    q = rng.standard_normal((6, D), dtype=np.float32)
    if name == "tail copies of sealed rows":
        tail[:20] = sealed[100:120]
        q[0], q[1] = sealed[100], sealed[119] * 3.0
    elif name == "duplicates inside the tail":
        tail[10:30] = tail[5]
        q[0] = tail[5]
    elif name == "a tail row equal to a query":
        q[2] = tail[7]
    elif name == "an all-zero query":
        q[3] = 0
    elif name == "T < k":
        tail = tail[:3]
        q[0] = tail[1]
    elif name == "idx_base":
        base = 123456789012
        q[0] = tail[39]
    elif name == "padded width":
        tail[:5] = sealed[:5]
        q[0] = sealed[2]
    return sealed, tail, q, k, base, D


@pytest.mark.parametrize("name", ["tail copies of sealed rows", "duplicates inside the tail", "a tail row equal to a query",
                                  "an all-zero query", "T < k", "idx_base", "padded width"])
def test_topk_with_a_tail_is_the_search_over_all_rows(name):
    sealed, tail, q, k, base, D = _grown_case(name, np.random.default_rng(3))
    rows = np.concatenate([sealed, tail])
    ops = PaddedTailOps if D == 100 else TailOps
    index = KeyIndex(torch.from_numpy(sealed), ops=ops)
    calls = TailOps.tail_calls
    index.extend(torch.from_numpy(rows))
    assert index.tail_rows == tail.shape[0]
    got = index.topk(torch.from_numpy(q), k, idx_base=base)
    assert TailOps.tail_calls == calls + 1           # ONE seeded pass
    assert index.tail_rows == tail.shape[0]          # and no seal
    _same(got, cref.topk_cosine(q, rows, k, base))
    if D == 100:   # the index owns the padded matrix and padded the new rows only
        assert tuple(index.keys_normalized.shape) == (rows.shape[0], 128)
        assert np.array_equal(index.keys_normalized[:, :100].numpy().view(np.int32), rows.view(np.int32))
        assert not index.keys_normalized[:, 100:].any()
        more = np.concatenate([rows, _rows(np.random.default_rng(4), 30, 100)])
        index.extend(torch.from_numpy(more))
        assert index.tail_rows == tail.shape[0] + 30
        assert np.array_equal(index.keys_normalized[:, :100].numpy().view(np.int32), more.view(np.int32))
        _same(index.topk(torch.from_numpy(q), k, idx_base=base), cref.topk_cosine(q, more, k, base))


@pytest.mark.parametrize("D, k", [(64, 70), (300, 10)])
def test_calls_without_a_seeded_pass_run_over_all_rows(D, k):
    rng = np.random.default_rng(5)
    rows = _rows(rng, 840, D)
    q = rng.standard_normal((4, D), dtype=np.float32)
    q[0] = rows[830]
    index = KeyIndex(torch.from_numpy(rows[:800]), ops=PaddedTailOps)
    index.extend(torch.from_numpy(rows))
    calls = TailOps.tail_calls
    _same(index.topk(torch.from_numpy(q), k, idx_base=7), cref.topk_cosine(q, rows, k, 7))
    assert TailOps.tail_calls == calls and index.tail_rows == 40


def test_toygraphbase_caches_grow_with_the_bank(monkeypatch):
    """Three appends between reads, across the reallocation of the raw stores (1024 -> 2048 rows) and of the normalised ones:
    the caches equal the one-shot normalisation bit for bit, and an existing index is extended, not dropped."""
    from ragraph_amd import kernels as K
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    normalised = []

    def normalize_rows(x, out=None):
        normalised.append(int(x.shape[0]))
        r = torch.from_numpy(cref.normalize_rows(x.numpy()))
        if out is None:
            return r
        out.copy_(r)
        return out

    monkeypatch.setattr(K, "normalize_rows", normalize_rows)
    rng = np.random.default_rng(6)
    D, C, A = 16, 3, 10
    keys = (rng.standard_normal((1500, D)) * 3).astype(np.float32)
    pos = rng.random((1500, A), dtype=np.float32)
    pos[::7] = 0                                    # all-zero code rows stay zero
    labels = np.eye(C, dtype=np.float32)[rng.integers(0, C, 1500)]

    def add(tgb, lo, hi):
        tgb.add_resources(torch.from_numpy(keys[lo:hi]), torch.from_numpy(keys[lo:hi]), torch.from_numpy(labels[lo:hi]),
                          torch.from_numpy(pos[lo:hi]))

    tgb = ToyGraphBase(None, C, D, 3, device="cpu")
    add(tgb, 0, 600)
    assert tgb._keys_normalized is None and tgb._positions_normalized is None      # made on first use, as ever
    first = tgb.keys_normalized
    tgb.positions_normalized
    assert normalised == [600, 600]
    tgb._index = index = K.KeyIndex(first, ops=TailOps)
    assert index.keys_normalized is first
    del normalised[:]
    for lo, hi in ((600, 900), (900, 1200), (1200, 1500)):
        add(tgb, lo, hi)
    assert normalised == [300] * 6                  # the new rows only, keys and codes
    assert tgb._keys.buf.shape[0] == 2048
    for cache, raw in ((tgb.keys_normalized, keys), (tgb.positions_normalized, pos)):
        assert tuple(cache.shape) == raw.shape
        assert np.array_equal(cache.numpy().view(np.int32), cref.normalize_rows(raw).view(np.int32))
    assert tgb._keys_normalized is tgb.keys_normalized and tgb._keys_normalized.shape[0] == 1500
    # the index object survived and covers all rows (300 rows pass the limit of an eighth of the sealed rows: each append sealed)
    assert tgb._index is index and index.sealed_rows + index.tail_rows == 1500
    assert index.keys_normalized is tgb._keys_normalized
    q = rng.standard_normal((3, D), dtype=np.float32)
    _same(index.topk(torch.from_numpy(q), 4), cref.topk_cosine(q, cref.normalize_rows(keys), 4))
    # set_resources starts over
    tgb.set_resources(torch.from_numpy(keys[:50]), torch.from_numpy(keys[:50]), torch.from_numpy(labels[:50]))
    assert tgb._keys_normalized is None and tgb._positions_normalized is None and tgb._index is None
    assert tgb.keys_normalized.shape[0] == 50
