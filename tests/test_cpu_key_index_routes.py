"""KeyIndex's dispatch on one recording shim with every optional entry of the ops protocol (no GPU): which entry answers a call
and with which arguments, what the call leaves in the library's thread-local knobs, which last_* fields and counters it moves,
in which order the preparation runs -- and KeyIndex._route, which names that path without side effects.  The statistics words
by name (ragraph_amd/filter_stats.py) against the literal layout of csrc/filter_prepare.h."""
import struct

import pytest
import torch

from ragraph_amd import filter_stats as FS
from ragraph_amd.kernels_index import ROUTES, KeyIndex

D, ROWS, BASE = 8, 300, 7
RULES = ("filter_helps", "filter_wide_helps", "filter_wide128_helps", "fused_helps", "small_helps", "packed_keys_help")


def f2ord(x):
    b = struct.unpack("<i", struct.pack("<f", x))[0]
    return b if b >= 0 else b ^ 0x7FFFFFFF


def exact(q, kn, k, idx_base=0):
    """The exact top-k in canonical order (score descending, lower row first), in float64 rounded once."""
    qd = q.double()
    norm = qd.norm(dim=1, keepdim=True)
    s = (qd / torch.where(norm > 0, norm, torch.ones_like(norm))) @ kn.double().T
    vals, idx = torch.sort(s, dim=1, descending=True, stable=True)
    return vals[:, :k].float(), idx[:, :k] + idx_base


def stats_words(B, spec=0, failed=0, lo=0.25, hi=0.29, over=0, tight=0, soft=0, repair=0, cand=100.0, i8=0, keys=ROWS):
    """A call's 32 statistics words, built BY NAME: one level, 8 sampled queries."""
    w = [0] * FS.N_WORDS
    w[FS.MAGIC], w[FS.LEVELS] = FS.MAGIC_VALUE, 1
    w[FS.CAND], w[FS.SAMPLED], w[FS.IS_I8], w[FS.KEYS] = int(cand * 8), 8, i8, keys
    w[FS.QUERIES], w[FS.SPECULATIVE], w[FS.SPEC_FAILED] = B, spec, failed
    w[FS.KTH_LO], w[FS.KTH_HI], w[FS.OVERFLOW] = f2ord(lo), f2ord(hi), over
    w[FS.TIGHT], w[FS.SOFT_MISSES], w[FS.REPAIR] = tight, soft, repair
    return w


class Ops:
    """Every optional entry KeyIndex asks for.  The *_helps rules answer from self.helps (a bool, or a function of the rule's
    arguments); the kernels return the exact answer and record (entry, keyword arguments, knobs in force); the knob setters
    keep a log."""
    FILTER_STATS = True
    TOPK_TAIL_MAX = 65536

    def __init__(self, **helps):
        assert set(helps) <= set(RULES)
        self.helps = dict.fromkeys(RULES, False)
        self.helps.update(helps)
        self.small_ready = True
        self.calls, self.knobs = [], []
        self.state = {"set_max_i8_levels": -1, "set_filter_prior": None, "set_filter_tight_prior": None}
        self.over = 0            # what the filtered kernels report as their overflow count (a CPU tensor)
        self.raise_in = None     # entry that raises instead of answering
        self.i8_levels = 1

    # -- layout helpers
    @staticmethod
    def padded_dim(dim):
        return next((w for w in (8, 16, 128) if dim <= w), None)

    @staticmethod
    def pad_cols(x, width):
        out = x.new_zeros((x.shape[0], width))
        out[:, :x.shape[1]] = x
        return out

    @staticmethod
    def keys_to_bf16(kn):
        return torch.zeros((kn.shape[0], kn.shape[1]), dtype=torch.int16)

    @staticmethod
    def pack_keys(kn):
        return kn.clone()

    @staticmethod
    def gather_rows(v, idx, idx_base=0):
        return v[idx - idx_base].clone()

    @staticmethod
    def dedup_rows(kn):
        uniq, inverse = torch.unique(kn, dim=0, return_inverse=True)
        order = torch.argsort(inverse, stable=True)                 # members by group, ascending row inside a group
        counts = torch.bincount(inverse, minlength=uniq.shape[0])
        ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
        first = order[ptr[:-1]]
        return uniq.shape[0], int(counts.max()), first, ptr, order

    # -- rules
    def _rule(self, name, *args):
        v = self.helps[name]
        return bool(v(*args)) if callable(v) else v

    def filter_helps(self, B, n, dim, k):
        return self._rule("filter_helps", B, n, dim, k)

    def filter_wide_helps(self, B, n, dim, k):
        return self._rule("filter_wide_helps", B, n, dim, k)

    def filter_wide128_helps(self, B, n, dim, k):
        return self._rule("filter_wide128_helps", B, n, dim, k)

    def fused_helps(self, B, n, dim, k):
        return self._rule("fused_helps", B, n, dim, k)

    def small_helps(self, B, n, dim, k):
        return self._rule("small_helps", B, n, dim, k)

    def packed_keys_help(self, B, dim, k):
        return self._rule("packed_keys_help", B, dim, k)

    def small_state_ready(self, device):
        return self.small_ready

    def filtered_i8_levels(self, B, n, dim, k):
        return self.i8_levels

    @staticmethod
    def int8_copy_classes(kb, n):
        return {"err": 0.01, "err_heavy": 0.01, "heavy_granules": 0, "granules": 4}

    # -- knobs
    def _knob(self, name, v):
        self.knobs.append((name, v))
        old, self.state[name] = self.state[name], v
        return old

    def set_max_i8_levels(self, n):
        return self._knob("set_max_i8_levels", n)

    def set_filter_prior(self, p):
        return self._knob("set_filter_prior", p)

    def set_filter_tight_prior(self, t):
        return self._knob("set_filter_tight_prior", t)

    # -- kernels
    def _ran(self, entry, q, kw):
        self.calls.append((entry, q.shape[0], kw, dict(self.state)))
        if self.raise_in == entry:
            raise RuntimeError("boom in " + entry)

    def _filtered_out(self, q, kn, k, idx_base, return_stats):
        out = exact(q, kn, k, idx_base) + (torch.tensor([self.over], dtype=torch.int32),)
        if return_stats:
            spec = int(self.state["set_filter_prior"] is not None)
            words = stats_words(q.shape[0], spec=spec, over=self.over, tight=int(self.state["set_filter_tight_prior"] is not None))
            out += (torch.tensor(words, dtype=torch.int32),)
        return out

    def topk_cosine(self, q, kn, k, **kw):
        self._ran("topk_cosine", q, kw)
        return exact(q, kn, k, kw.get("idx_base", 0))

    def topk_cosine_fused(self, q, kn, kb, k, **kw):
        self._ran("topk_cosine_fused", q, kw)
        return exact(q, kn, k, kw.get("idx_base", 0))

    def topk_cosine_small(self, q, kn, kb, k, **kw):
        self._ran("topk_cosine_small", q, kw)
        return self._filtered_out(q, kn, k, kw.get("idx_base", 0), kw.get("return_stats", False))

    def topk_cosine_filtered(self, q, kn, kb, k, **kw):
        self._ran("topk_cosine_filtered", q, kw)
        return self._filtered_out(q, kn, k, kw.get("idx_base", 0), kw.get("return_stats", False))

    def topk_cosine_tail(self, q, kt, s, i, idx_base):
        self._ran("topk_cosine_tail", q, {"idx_base": idx_base})
        ts, ti = exact(q, kt, min(s.shape[1], kt.shape[0]), idx_base)
        vals, order = torch.sort(torch.cat([s, ts], 1), dim=1, descending=True, stable=True)
        return vals[:, :s.shape[1]], torch.gather(torch.cat([i, ti], 1), 1, order)[:, :s.shape[1]]

    def topk_expand_groups(self, su, iu, ptr, mem, k, **kw):
        self._ran("topk_expand_groups", su, kw)
        s = torch.empty(su.shape[0], k)
        i = torch.empty(su.shape[0], k, dtype=torch.int64)
        for b in range(su.shape[0]):
            rows = [(float(su[b, j]), int(m)) for j in range(su.shape[1]) for m in mem[ptr[iu[b, j]]:ptr[iu[b, j] + 1]]][:k]
            s[b] = torch.tensor([r[0] for r in rows])
            i[b] = torch.tensor([r[1] for r in rows]) + kw.get("idx_base", 0)
        return s, i


class NoStatsOps(Ops):
    """An older ops object: no FILTER_STATS, and filtered entries that take no return_stats and return three values."""
    FILTER_STATS = False

    def topk_cosine_small(self, q, kn, kb, k, idx_base=0):
        return Ops.topk_cosine_small(self, q, kn, kb, k, idx_base=idx_base)

    def topk_cosine_filtered(self, q, kn, kb, k, idx_base=0, keys_packed=None, exchange=None, plan_n=0):
        return Ops.topk_cosine_filtered(self, q, kn, kb, k, idx_base=idx_base, keys_packed=keys_packed, exchange=exchange,
                                        plan_n=plan_n)


def normalized(rows, dim=D, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(rows, dim, generator=g), dim=1)


def queries(B, dim=D, seed=1):
    return torch.randn(B, dim, generator=torch.Generator().manual_seed(seed))


def bank(ops, rows=ROWS, dim=D, dedup=False):
    return KeyIndex(normalized(rows, dim), ops=ops, dedup=dedup)


def _freeze(v):
    if isinstance(v, torch.Tensor):
        return ("tensor", id(v))
    if isinstance(v, KeyIndex):
        return ("index", id(v), _freeze(vars(v)))
    if isinstance(v, dict):
        return {key: _freeze(x) for key, x in v.items()}
    if isinstance(v, (list, tuple)):
        return (type(v).__name__,) + tuple(_freeze(x) for x in v)
    return v if isinstance(v, (int, float, str, bool, type(None))) else ("object", id(v))


def route_name(index, q, k, exchange=None, plan_n=0):
    """KeyIndex._route for the call index.topk(q, k, ...) would make now: asked twice, the same name, no attribute moved."""
    before = _freeze(vars(index))
    args = (q.shape[0], index.sealed_rows, index._width or index.dim, k, exchange, plan_n)
    first, second = index._route(*args), index._route(*args)
    assert first == second and first in ROUTES and _freeze(vars(index)) == before
    return first


def counters(index):
    return index._queries, index._overflowed


def warm(index, k, lo=0.25, hi=0.29):
    """Two polled calls with a bound pass: the next call of this k runs under a prior (and a tight bound above it)."""
    for _ in range(2):
        index._judge_prior(k, 512, stats_words(512, lo=lo, hi=hi), 0)


SENTINEL = object()


def mark(index):
    index.last_prior = index.last_tight = index.last_stats = index.last_over = SENTINEL


# ---------------------------------------------------------------------------------------------- one call per route name

PLAIN = [  # (route, rules that say yes, k, entry, keyword arguments beyond idx_base)
    ("SLAB", {}, 5, "topk_cosine", {}),
    ("SLAB", {}, 40, "topk_cosine", {}),
    ("PACKED", {"packed_keys_help": True}, 5, "topk_cosine", {"keys_packed": "_packed"}),
    ("FUSED", {"fused_helps": True, "packed_keys_help": True}, 5, "topk_cosine_fused", {}),
]


def test_the_route_names_are_a_closed_set():
    assert sorted(ROUTES) == sorted(["SLAB", "PACKED", "FUSED", "SMALL", "FILTERED", "WIDE", "WIDE128", "SHARDED", "COLLAPSED",
                                     "SLABS_OF_FILTERED"])


@pytest.mark.parametrize("route,helps,k,entry,extra", PLAIN)
def test_unguarded_routes(route, helps, k, entry, extra):
    ops = Ops(**helps)
    index, q = bank(ops), queries(6)
    mark(index)
    assert route_name(index, q, k) == route
    s, i = index.topk(q, k, idx_base=BASE)
    ws, wi = exact(q, index.keys_normalized, k, BASE)
    assert torch.equal(i, wi) and torch.equal(s, ws)
    (got, B, kw, state), = ops.calls
    want = {"idx_base": BASE, **{name: getattr(index, attr) for name, attr in extra.items()}}
    assert (got, B) == (entry, 6) and set(kw) == set(want) and all(kw[n] is want[n] or kw[n] == want[n] for n in want)
    assert ops.knobs == [] and counters(index) == (6, 0)
    assert index.last_prior is SENTINEL and index.last_tight is SENTINEL and index.last_stats is SENTINEL
    assert (index._bf16 is not None) == (route == "FUSED") and (index._packed is not None) == (route == "PACKED")


def test_a_width_without_a_fused_kernel_and_a_large_k_take_the_slabs_off_the_clock():
    ops = Ops(filter_helps=True, fused_helps=True, small_helps=True, packed_keys_help=True)
    wide = KeyIndex(normalized(ROWS, 200), ops=ops, dedup=True)         # wider than every fused kernel: nothing is judged
    q = queries(3, 200)
    assert wide._width is None and route_name(wide, q, 5) == "SLAB"
    s, i = wide.topk(q, 5, idx_base=BASE)
    assert torch.equal(i, exact(q, wide.keys_normalized, 5, BASE)[1])
    assert ops.calls == [("topk_cosine", 3, {"idx_base": BASE}, ops.state)] and counters(wide) == (0, 0)
    assert wide._collapsed is None
    del ops.calls[:]
    index, q = bank(ops), queries(3)                                    # k beyond every filtered list
    pend = index._pending = (torch.zeros(1, dtype=torch.int32), None, 3, False)    # (its event would fail if it were asked)
    assert route_name(index, q, 129) == "SLAB" and route_name(index, q, 100) == "SLAB"     # (100: the wide128 rule says no)
    for k in (129, 100):
        s, i = index.topk(q, k, idx_base=BASE)
        assert torch.equal(i, exact(q, index.keys_normalized, k, BASE)[1])
    assert [c[0] for c in ops.calls] == ["topk_cosine"] * 2 and all(c[2] == {"idx_base": BASE} for c in ops.calls)
    assert counters(index) == (0, 0) and index._pending is pend and index.last_prior is None and ops.knobs == []


def test_a_padded_width_pads_the_query_once_and_answers_over_the_padded_bank():
    ops = Ops(filter_helps=True)
    index = KeyIndex(normalized(ROWS, 5), ops=ops, dedup=False)
    q = queries(20, 5)
    assert index._width == 8 and index.keys_normalized.shape == (ROWS, 8)
    for k, route in ((5, "FILTERED"), (100, "SLAB")):
        assert route_name(index, q, k) == route
        s, i = index.topk(q, k)
        assert torch.equal(i, exact(q, index.keys_normalized[:, :5], k)[1])
    assert [c[0] for c in ops.calls] == ["topk_cosine_filtered", "topk_cosine"]
    with pytest.raises(ValueError):
        index.topk(queries(2, 8), 5)


GUARDED = [  # (route, rules that say yes, k, queries, entry)
    ("SMALL", {"small_helps": True, "filter_helps": True}, 5, 4, "topk_cosine_small"),
    ("FILTERED", {"filter_helps": True, "filter_wide_helps": True, "packed_keys_help": True}, 5, 20, "topk_cosine_filtered"),
    ("WIDE", {"filter_wide_helps": True}, 40, 20, "topk_cosine_filtered"),
    ("WIDE128", {"filter_wide128_helps": True}, 100, 20, "topk_cosine_filtered"),
]


@pytest.mark.parametrize("route,helps,k,B,entry", GUARDED)
def test_guarded_single_bank_routes(route, helps, k, B, entry):
    """The table of the guarded call, columns single-launch and filtered / wide / wide128, without a prior."""
    ops = Ops(**helps)
    ops.over = 3
    index, q = bank(ops), queries(B)
    mark(index)
    noted = []
    note = index._note_overflow
    index._note_overflow = lambda *a: noted.append(a) or note(*a)
    assert route_name(index, q, k) == route
    s, i = index.topk(q, k, idx_base=BASE)
    ws, wi = exact(q, index.keys_normalized, k, BASE)
    assert torch.equal(i, wi) and torch.equal(s, ws)
    (got, nq, kw, state), = ops.calls
    small = route == "SMALL"
    assert (got, nq) == (entry, B)
    assert kw == ({"idx_base": BASE, "return_stats": True} if small else {"idx_base": BASE, "keys_packed": None, "return_stats": True})
    assert state == {"set_max_i8_levels": -1, "set_filter_prior": None, "set_filter_tight_prior": None}
    assert ops.knobs == [("set_max_i8_levels", -1), ("set_max_i8_levels", -1)]        # capped for the bank, reset; no prior yet
    assert index.last_prior is None and index.last_over is SENTINEL
    if small:
        assert index.last_tight is SENTINEL and index.last_stats is SENTINEL          # (the single-launch route records the prior only)
    else:
        assert index.last_tight is None and index.last_stats.tolist() == stats_words(B, over=3)
    assert counters(index) == (B, 3)                                                  # _note_overflow was reached: + the shim's count
    (over, nB, had_i8, stats, nk), = noted
    assert int(over) == 3 and (nB, nk) == (B, k) and stats.tolist() == stats_words(B, over=3)
    assert had_i8 is (not small)                                                      # D = 8 is no int8 width of the single-launch kernel
    assert index._packed is None and index.i8_classes is not None


def test_had_i8_as_each_route_hands_it_on():
    def handed_on(ops, k, B, dim=D, off=False):
        index = bank(ops, dim=dim)
        index._i8_off = off
        noted = []
        index._note_overflow = lambda *a: noted.append(a)
        index.topk(queries(B, dim), k)
        return noted[0][2]

    small = Ops(small_helps=True)
    assert handed_on(small, 5, 4, dim=128) is True and handed_on(small, 5, 4, dim=8) is False
    assert handed_on(small, 5, 4, dim=128, off=True) is False
    assert small.knobs[-2:] == [("set_max_i8_levels", 0), ("set_max_i8_levels", -1)]   # a demoted bank: capped at 0 for the call
    filtered = Ops(filter_helps=True, filter_wide_helps=True)
    assert handed_on(filtered, 5, 20) is True and handed_on(filtered, 5, 20, off=True) is False
    filtered.i8_levels = 0                                         # the plan of this shape has no int8 level
    assert handed_on(filtered, 5, 20) is False
    assert handed_on(filtered, 40, 20) is True                     # a wide call under an open cap is taken to have had them
    assert handed_on(filtered, 40, 20, off=True) is False


def test_sharded_route():
    """The table's first column: the caller's prior, no tight bound, no keys_packed, last_over / last_stats / last_prior, and
    neither the clock nor _note_overflow."""
    ops = Ops(filter_helps=lambda B, n, dim, k: n >= 1000, small_helps=True, fused_helps=True)
    ops.over = 3
    index, q = bank(ops), queries(20)
    warm(index, 5)                                                 # (the index's own history plays no part in a sharded call)
    index._pending = pend = (torch.zeros(1, dtype=torch.int32), None, 3, False)
    exchange = object()
    for prior in (None, 0.125):
        mark(index)
        del ops.calls[:], ops.knobs[:]
        assert route_name(index, q, 5, exchange, 1000) == "SHARDED"                  # the rule is asked about plan_n, not this shard
        s, i = index.topk(q, 5, BASE, exchange, 1000, prior)
        assert torch.equal(i, exact(q, index.keys_normalized, 5, BASE)[1])
        (got, nq, kw, state), = ops.calls
        assert (got, nq) == ("topk_cosine_filtered", 20)
        assert kw == {"idx_base": BASE, "exchange": exchange, "plan_n": 1000, "return_stats": True}
        assert state == {"set_max_i8_levels": -1, "set_filter_prior": prior, "set_filter_tight_prior": None}
        reset = [("set_max_i8_levels", -1)] + ([("set_filter_prior", None)] if prior is not None else [])
        assert ops.knobs == [("set_max_i8_levels", -1)] + ([("set_filter_prior", prior)] if prior is not None else []) + reset
        assert index.last_prior == prior and index.last_tight is SENTINEL
        assert int(index.last_over) == 3 and index.last_stats.tolist() == stats_words(20, spec=int(prior is not None), over=3)
        assert counters(index) == (0, 0) and index._pending is pend
    # the rule says no for this plan: the shard's own exact top-k on the fp32 kernels, ON the clock (fused before small)
    index._pending = None
    del ops.calls[:]
    assert route_name(index, q, 5, exchange, 999) == "FUSED"
    index.topk(q, 5, BASE, exchange, 999)
    assert [c[0] for c in ops.calls] == ["topk_cosine_fused"] and counters(index) == (20, 0)


def test_collapsed_route_moves_only_the_inner_clock():
    ops = Ops(filter_helps=True)
    kn = normalized(60)[torch.arange(ROWS) % 60]                   # every row stored five times
    index = KeyIndex(kn, ops=ops, dedup=True)
    index.DEDUP_MIN_ROWS = 64
    q = queries(20)
    assert route_name(index, q, 5) == "FILTERED"                   # not judged yet: named as it stands
    assert index.search_rows() == 60 and index.duplicate_stats == (ROWS, 60, 5)
    inner = index.search_index
    mark(index)
    assert route_name(index, q, 5) == "COLLAPSED" and route_name(inner, q, 5) == "FILTERED"
    assert route_name(index, q, 100) == "SLAB"                     # the expansion stops at 64: the full bank on the slabs
    s, i = index.topk(q, 5, idx_base=BASE)
    ws, wi = exact(q, kn, 5, BASE)
    assert torch.equal(i, wi) and torch.equal(s, ws)
    assert [(c[0], c[2]) for c in ops.calls] == [("topk_cosine_filtered", {"idx_base": 0, "keys_packed": None, "return_stats": True}),
                                                 ("topk_expand_groups", {"idx_base": BASE})]
    assert counters(index) == (0, 0) and counters(inner) == (20, 0)
    assert index.last_prior is SENTINEL and index.last_stats is SENTINEL and inner.last_stats is not None
    assert index._bf16 is None and inner._bf16 is not None


def test_slabs_of_filtered(monkeypatch):
    monkeypatch.setattr(KeyIndex, "MAX_FILTERED_BATCH", 4)
    ops = Ops(filter_helps=True)
    index, q = bank(ops), queries(10)
    assert route_name(index, q, 5) == "SLABS_OF_FILTERED" and route_name(index, q[:4], 5) == "FILTERED"
    s, i = index.topk(q, 5, idx_base=BASE)
    ws, wi = exact(q, index.keys_normalized, 5, BASE)
    assert torch.equal(i, wi) and torch.equal(s, ws)
    assert [(c[0], c[1]) for c in ops.calls] == [("topk_cosine_filtered", 4), ("topk_cosine_filtered", 4), ("topk_cosine_filtered", 2)]
    assert all(c[2] == {"idx_base": BASE, "keys_packed": None, "return_stats": True} for c in ops.calls)
    assert counters(index) == (20, 0)                              # (the whole call and each of its slabs advance the clock)
    assert index.last_stats.tolist() == stats_words(2)             # the last slab's
    # a sharded call of more queries than one filtered call takes stays off the filter
    assert route_name(index, q, 5, object(), 1000) == "SLAB"


def test_a_tail_is_searched_behind_the_sealed_route():
    ops = Ops(filter_helps=True)
    index, q = bank(ops), queries(20)
    longer = torch.cat([index.keys_normalized, normalized(3, seed=5)])
    index.extend(longer)
    assert (index.sealed_rows, index.tail_rows) == (ROWS, 3)
    assert route_name(index, q, 5) == "FILTERED"
    s, i = index.topk(q, 5, idx_base=BASE)
    assert torch.equal(i, exact(q, longer, 5, BASE)[1])
    assert [(c[0], c[2].get("idx_base")) for c in ops.calls] == [("topk_cosine_filtered", BASE), ("topk_cosine_tail", BASE + ROWS)]
    assert counters(index) == (20, 0)


# ---------------------------------------------------------------------------------------------------------- precedence

def test_precedence_fused_small_filtered_packed_slab():
    everything = dict.fromkeys(("fused_helps", "small_helps", "filter_helps", "packed_keys_help"), True)
    order = [("fused_helps", "FUSED", "topk_cosine_fused"), ("small_helps", "SMALL", "topk_cosine_small"),
             ("filter_helps", "FILTERED", "topk_cosine_filtered"), ("packed_keys_help", "PACKED", "topk_cosine"), (None, "SLAB", "topk_cosine")]
    for rule, route, entry in order:
        ops = Ops(**everything)
        index, q = bank(ops), queries(4)
        assert route_name(index, q, 5) == route
        index.topk(q, 5)
        assert [c[0] for c in ops.calls] == [entry], route
        everything.pop(rule, None)
    ops = Ops(small_helps=True, filter_helps=True)
    ops.small_ready = False                                        # (a capture on a stream without the kernel's state buffer)
    index, q = bank(ops), queries(4)
    assert route_name(index, q, 5) == "FILTERED"
    index.topk(q, 5)
    assert [c[0] for c in ops.calls] == ["topk_cosine_filtered"]
    # a bank that defeated the filter: fused, small and filtered are out at once
    ops = Ops(fused_helps=True, small_helps=True, filter_helps=True, packed_keys_help=True)
    index = bank(ops)
    index._filter_off = True
    assert route_name(index, q, 5) == "PACKED"
    index.topk(q, 5)
    assert [c[0] for c in ops.calls] == ["topk_cosine"] and ops.calls[0][2]["keys_packed"] is index._packed


# ------------------------------------------------------------------------------------------------------------- ordering

def demoted(ops):
    """A bank whose filter demotion is due for its re-probe."""
    index = bank(ops)
    index._demote("filter")
    index._queries = KeyIndex.REPROBE_QUERIES
    return index


def test_a_due_demotion_is_lifted_by_the_call_that_then_takes_the_filter():
    ops = Ops(filter_helps=True)
    index, q = demoted(ops), queries(20)
    assert route_name(index, q, 5) == "SLAB"                       # as the bank stands
    index.topk(q, 5)
    assert [c[0] for c in ops.calls] == ["topk_cosine_filtered"]
    assert index._filter_off is False and index._demoted["filter"] is None
    assert index._probed_at["filter"] == KeyIndex.REPROBE_QUERIES and index._queries == KeyIndex.REPROBE_QUERIES + 20
    assert route_name(index, q, 5) == "FILTERED"


def test_the_same_demotion_under_a_large_k_stays():
    ops = Ops(filter_helps=True, filter_wide128_helps=True)
    index, q = demoted(ops), queries(20)
    assert route_name(index, q, 100) == "SLAB"
    index.topk(q, 100)
    assert [c[0] for c in ops.calls] == ["topk_cosine"]
    assert index._filter_off is True and index._demoted["filter"] == 0 and index._probed_at["filter"] is None
    assert index._queries == KeyIndex.REPROBE_QUERIES


class Polled:
    def query(self):
        return True


def test_the_poll_comes_before_the_route_reads_the_demotion():
    """A pending word that demotes the filter is judged at the start of the next call on the clock: that call is on fp32."""
    ops = Ops(filter_helps=True, filter_wide128_helps=True)
    for k in (5, 100):
        index, q = bank(ops), queries(20)
        word = torch.tensor([64] + [0] * 32, dtype=torch.int32)    # 64 of 64 queries overflowed, on bf16 levels
        index._pending = (word, Polled(), 64, False)
        del ops.calls[:]
        index.topk(q, k)
        assert index._filter_off is True and index._pending is None and counters(index) == (20, 64)
        assert [c[0] for c in ops.calls] == ["topk_cosine"]


# --------------------------------------------------------------------------------------------------------- knob hygiene

def guarded_call(kind, with_prior, raising=False, ops_type=Ops):
    """One guarded call of each kind; returns (ops, index, what the call ran under or the exception)."""
    ops = ops_type(small_helps=lambda B, n, dim, k: B <= 16, filter_helps=True)
    index = bank(ops)
    B = {"small": 4, "filtered": 20, "tight": KeyIndex.TIGHT_MIN_BATCH, "sharded": 20}[kind]
    if with_prior and kind != "sharded":
        warm(index, 5)
    mark(index)
    index.last_over = None
    if raising:
        ops.raise_in = "topk_cosine_small" if kind == "small" else "topk_cosine_filtered"
    q = queries(B)
    args = (q, 5, BASE, object(), 1000, 0.125 if with_prior else None) if kind == "sharded" else (q, 5, BASE)
    if raising:
        with pytest.raises(RuntimeError, match="boom"):
            index.topk(*args)
    else:
        s, i = index.topk(*args)
        assert torch.equal(i, exact(q, index.keys_normalized, 5, BASE)[1])
    return ops, index


@pytest.mark.parametrize("raising", (False, True))
@pytest.mark.parametrize("kind,with_prior", [("small", False), ("small", True), ("filtered", False), ("filtered", True),
                                             ("tight", True), ("sharded", False), ("sharded", True)])
def test_every_knob_a_guarded_call_set_is_reset(kind, with_prior, raising):
    ops, index = guarded_call(kind, with_prior, raising)
    (entry, B, kw, state), = ops.calls
    prior = {"sharded": 0.125}.get(kind, 0.25 - 0.5 * (0.29 - 0.25)) if with_prior else None     # lowest seen - half the spread
    tight = 0.25 - KeyIndex.TIGHT_MARGIN if kind == "tight" else None
    assert state["set_max_i8_levels"] == -1
    assert (state["set_filter_prior"] is None) == (prior is None) and (prior is None or abs(state["set_filter_prior"] - prior) < 1e-6)
    assert (state["set_filter_tight_prior"] is None) == (tight is None) and (tight is None or abs(state["set_filter_tight_prior"] - tight) < 1e-6)
    names = ["set_max_i8_levels"] + ["set_filter_prior"] * (prior is not None) + ["set_filter_tight_prior"] * (tight is not None)
    assert [n for n, _ in ops.knobs] == names + names                                 # set, then reset: nothing else is touched
    assert [v for _, v in ops.knobs[len(names):]] == [-1] + [None] * (len(names) - 1)
    assert ops.state == {"set_max_i8_levels": -1, "set_filter_prior": None, "set_filter_tight_prior": None}
    if raising:
        assert index.last_prior is SENTINEL and index.last_tight is SENTINEL and index.last_stats is SENTINEL
        assert index.last_over is None and index._overflowed == 0 and index._pending is None
    else:
        assert (index.last_prior is None) == (prior is None) and (prior is None or abs(index.last_prior - prior) < 1e-6)
        if kind in ("filtered", "tight"):
            assert (index.last_tight is None) == (tight is None) and (tight is None or abs(index.last_tight - tight) < 1e-6)
            assert index.last_stats[FS.SPECULATIVE] == int(with_prior) and index.last_stats[FS.TIGHT] == int(kind == "tight")
        else:
            assert index.last_tight is SENTINEL
            assert (index.last_stats is SENTINEL) == (kind == "small")


@pytest.mark.parametrize("kind", ("small", "filtered", "sharded"))
def test_an_ops_object_without_filter_stats_is_called_without_return_stats(kind):
    ops, index = guarded_call(kind, False, ops_type=NoStatsOps)
    ops.over = 2
    del ops.calls[:]
    q = queries(ops_B := {"small": 4, "filtered": 20, "sharded": 20}[kind])
    exchange = object()
    noted = []
    note = index._note_overflow
    index._note_overflow = lambda *a: noted.append(a) or note(*a)
    mark(index)
    if kind == "sharded":
        index.topk(q, 5, BASE, exchange, 1000)
        want = {"idx_base": BASE, "keys_packed": None, "exchange": exchange, "plan_n": 1000}    # (as NoStatsOps spells its defaults out)
    else:
        index.topk(q, 5, BASE)
        want = {"idx_base": BASE} if kind == "small" else {"idx_base": BASE, "keys_packed": None, "exchange": None, "plan_n": 0}
    (entry, B, kw, state), = ops.calls
    assert B == ops_B and kw == want
    if kind == "sharded":
        assert int(index.last_over) == 2 and index.last_stats is SENTINEL and noted == []     # last_stats only with FILTER_STATS
    else:
        assert noted[0][3] is None and index._overflowed == 2
        assert index.last_stats is (SENTINEL if kind == "small" else None)


# --------------------------------------------------------------------------------------------------------- filter_stats

def test_named_words_against_the_literal_layout():
    """The second, independent copy of the layout: the literal numbers of the comment in csrc/filter_prepare.h."""
    w = [0] * FS.N_WORDS
    w[FS.MAGIC], w[FS.LEVELS] = FS.MAGIC_VALUE, 3
    for l, (cand, sampled, i8, keys) in enumerate(((800, 8, 0, 1000), (0, 0, 1, 4000), (450, 9, 1, 16000))):
        w[FS.CAND + l], w[FS.SAMPLED + l], w[FS.IS_I8 + l], w[FS.KEYS + l] = cand, sampled, i8, keys
    w[FS.QUERIES], w[FS.ZERO_QUERIES], w[FS.SPECULATIVE], w[FS.SPEC_FAILED] = 512, 2, 1, 7
    w[FS.KTH_LO], w[FS.KTH_HI], w[FS.OVERFLOW] = f2ord(-0.5), f2ord(0.75), 9
    w[FS.TIGHT], w[FS.SOFT_MISSES], w[FS.REPAIR] = 1, 33, 2
    assert len(w) == 32 == FS.N_WORDS and FS.MAGIC_VALUE == 0x52414753
    assert w[0] == 0x52414753 and w[1] == 3 and w[2:5] == [800, 0, 450] and w[5:8] == [8, 0, 9] and w[8:11] == [0, 1, 1]
    assert w[11:14] == [1000, 4000, 16000] and w[14:18] == [512, 2, 1, 7] and w[20:24] == [9, 1, 33, 2] and w[24:] == [0] * 8
    assert FS.ord2f(w[18]) == -0.5 and FS.ord2f(w[19]) == 0.75
    assert FS.levels(w) == [("int8" if w[8 + l] else "bf16", w[11 + l], (w[2 + l] / w[5 + l]) if w[5 + l] else None) for l in range(3)]
    assert FS.levels(w) == [("bf16", 1000, 100.0), ("int8", 4000, None), ("int8", 16000, 50.0)]
    assert FS.candidates_per_query(w) == sum(w[2 + l] / w[5 + l] for l in range(min(w[1], 3)) if w[5 + l]) == 150.0
    w[1] = 1
    assert FS.levels(w) == [("bf16", 1000, 100.0)] and FS.candidates_per_query(w) == 100.0
    w[5] = w[7] = 0
    assert FS.candidates_per_query(w) is None                       # nothing sampled
    assert FS.levels(w[:15]) == [] and FS.levels([0] * 32) == [] and len(FS.levels(w[:16])) == 1


def test_ord2f_round_trips_the_bit_patterns():
    for bits in (0xBF800000, 0x80000000, 0x00000000, 0x00000001, 0x3F800000, 0x807FFFFF):   # -1, -0, +0, subnormals, 1
        x = struct.unpack("<f", struct.pack("<I", bits))[0]
        assert struct.pack("<f", FS.ord2f(f2ord(x))) == struct.pack("<I", bits), hex(bits)
    assert f2ord(-1.0) < f2ord(-0.0) < f2ord(0.0) < f2ord(1e-45) < f2ord(1.0)               # (the order the words rely on)


def test_the_kernels_module_forwards_its_names():
    from ragraph_amd import kernels as K

    assert K.FILTER_STATS_MAGIC == FS.MAGIC_VALUE
    w = stats_words(64, cand=12.5, i8=1)
    assert K.filter_stats_levels(w) == FS.levels(w) == [("int8", ROWS, 12.5)]
    assert K.ord2f(f2ord(-0.3)) == FS.ord2f(f2ord(-0.3))


# ------------------------------------------------------------------------------------------------------ old against new

POLLED = [  # the statistics of a polled call, and whether it had int8 levels
    (dict(spec=0, over=0), False),
    (dict(spec=0, over=3), False),                                  # overflowed lists under a bound pass: the lists' own
    (dict(spec=1, failed=2, over=2), False),                        # misses of the prior
    (dict(spec=1, over=5, cand=900.0), False),                      # lists overflowed under the prior, a flood of candidates
    (dict(spec=1, tight=1, soft=KeyIndex.TIGHT_MAX_SOFT + 1, repair=1), False),
    (dict(spec=1, tight=1, soft=4, repair=2), False),
    (dict(spec=0, over=1, cand=500.0, i8=1), True),                 # an int8 level that passes too many candidates
]


@pytest.mark.parametrize("fields,had_i8", POLLED)
def test_the_pinned_word_is_judged_like_its_words(fields, had_i8):
    """_poll_overflow on a pinned-word-shaped tensor ([0] = -1: the count is in the words) against _judge_prior / _judge_tight on
    the same words as a plain list."""
    k, B = 5, 512
    words = stats_words(B, **fields)
    polled, direct, tight_only = (bank(Ops()) for _ in range(3))
    for index in (polled, direct, tight_only):
        warm(index, k)
    polled._pending = (torch.tensor([-1] + words, dtype=torch.int32), Polled(), B, had_i8, k)
    polled._poll_overflow()
    left = direct._judge_prior(k, B, list(words), words[FS.OVERFLOW])
    direct._overflowed += left
    assert polled._pending is None and polled._spec[k] == direct._spec[k] and polled._overflowed == direct._overflowed
    assert left == (0 if fields["spec"] else fields.get("over", 0))
    st = tight_only._spec_state(k)
    tight_only._judge_tight(st, list(words))
    for key in ("soft", "tight_used", "tight_off_at", "tight_margin"):
        assert st.get(key) == (polled._spec[k].get(key) if fields["spec"] else None), key
    assert polled._seen_i8 == ([B, left] if had_i8 else [0, 0]) and polled._seen_bf16 == ([0, 0] if had_i8 else [B, left])
    if had_i8:
        assert polled.last_i8_candidates == 500.0 and polled._i8_off is True
    else:
        assert polled.last_i8_candidates is None and polled._i8_off is False
    if fields.get("tight"):
        assert polled._spec[k]["tight_margin"] == 2 * KeyIndex.TIGHT_MARGIN
        assert (polled._spec[k].get("tight_off_at") is not None) == (fields["repair"] == 2)


def test_short_words_are_polled_as_before():
    """A 4-tuple with a 1-element word (counts only), and 20-word statistics (no tight words): nothing beyond them is read."""
    index = bank(Ops())
    index._pending = (torch.tensor([2], dtype=torch.int32), Polled(), 8, False)
    index._poll_overflow()
    assert index._overflowed == 2 and index._seen_bf16 == [8, 2] and index._spec == {}
    index._pending = (torch.tensor([1] + stats_words(8, spec=1)[:20], dtype=torch.int32), Polled(), 8, False, 5)
    index._poll_overflow()
    assert index._overflowed == 2 and index._spec[5]["used"] == 1 and "tight_used" not in index._spec[5]   # (speculative: not the lists')
    index._pending = (torch.tensor([1] + stats_words(8)[:19], dtype=torch.int32), Polled(), 8, False, 5)
    index._poll_overflow()
    assert index._overflowed == 3 and index._spec[5]["used"] == 1 and index._spec[5]["hist"] == []         # too short to judge a prior
