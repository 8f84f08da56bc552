"""The workspace contract of every wrapper that asks kernels._workspace for scratch memory, on the device:

  * the host-side size query reports at least what the launches carve up and WRITE, and the result does not depend on what
    the workspace held before the call -- every case runs through its Python wrapper on a workspace of exactly the bytes the
    size query asked for, between two guard bands, filled with 0x00 / 0xFF / 0xA5 (tests/guarded_workspace.py): the result
    must be the bits of the run on the ordinary (grow-only, >= 1 MiB) workspace, that run must agree with the CPU reference the
    family's own test uses (two equally wrong runs must not pass), and no guard byte may change;
  * an entry refuses a workspace one byte shorter with RAGRAPH_EWORKSPACE (-3) before it launches anything: the guards AND
    the interior of the short workspace still hold the fill.

One table, CASES: at least one case per function of kernels.py that calls _workspace (tests/test_cpu_guarded_workspace.py
fails when a wrapper has none).  proto_cosine_grad_proto, which allocates its own scratch, is called through ctypes on a
guarded buffer; the raw scan and radix sort get theirs in tests/test_gpu_ingest.py.  Nothing here captures a HIP graph: the
guarded allocator makes a fresh allocation per request.  READS past the end of a workspace are not detected."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bank_rng_oracle as BO  # noqa: E402
import guarded_workspace as GW  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I64_MAX = np.iinfo(np.int64).max
MASK = np.float32(-1e8)
SEED = 0x0BAD_5EED_1234_567

CASES = []   # (id, wrapper name, environment {name: value or None}, factory(dev) -> (run, verify))
# The two cases whose size query is 0 (the ordered selection of rows this short runs inside LDS): the wrapper passes an empty
# workspace, no contract is exercised, and there is nothing to shorten.  Every other case also runs one byte short.
ZERO_QUERY = ("topk_rows-k-equals-N-3x65", "topk_rows-k-equals-N-4x4096")


def case(wrapper, name, env=None):
    def deco(factory):
        CASES.append((f"{wrapper}-{name}", wrapper, env or {}, factory))
        return factory
    return deco


def declared_wrappers():
    """The functions of kernels.py this table has a guarded case for (read by tests/test_cpu_guarded_workspace.py)."""
    return {c[1] for c in CASES}


def short_wrappers():
    """The functions with a case that is also run on a workspace one byte short."""
    return {c[1] for c in CASES if c[0] not in ZERO_QUERY}


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def NP(t):
    return t.detach().cpu().numpy()


def _bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def same_bits(got, want, what=""):
    """Every output: tensors bit for bit (so -0 / +0 and NaN payloads count), numpy arrays and scalars by value."""
    assert type(got) is type(want) or (isinstance(got, (tuple, list)) and isinstance(want, (tuple, list))), what
    if isinstance(want, (tuple, list)):
        assert len(got) == len(want), what
        for j, (g, w) in enumerate(zip(got, want)):
            same_bits(g, w, f"{what}[{j}]")
    elif isinstance(want, torch.Tensor):
        assert got.shape == want.shape and got.dtype == want.dtype, what
        assert torch.equal(_bits(got), _bits(want)), f"{what}: differs from the run on the ordinary workspace"
    elif isinstance(want, np.ndarray):
        assert got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8)), what
    else:
        assert got == want, what


def _set_env(monkeypatch, env):
    for name, value in env.items():
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def guarded(monkeypatch, run, fill, short=False):
    from ragraph_amd import kernels as K

    gw = GW.GuardedWorkspace(fill=fill, short=short)
    with monkeypatch.context() as m:
        m.setattr(K, "_workspace", gw)
        out = run()
    return out, gw


# ---- CPU references ---------------------------------------------------------------------------------------------------------
def _cref():
    from oracle import cref
    return cref


def _bank(rng, N, D):
    return _cref().normalize_rows(rng.standard_normal((N, D), dtype=np.float32))


def _verify_topk(q, kn, k, idx_base=0, rows=None):
    """(scores, idx, ...) against oracle.cref.topk_cosine, bit for bit; `rows`: a subset of the queries of a large batch."""
    cref = _cref()
    r = np.arange(q.shape[0]) if rows is None else rows
    rs, ri = cref.topk_cosine(q[r], kn, k, idx_base=idx_base)

    def verify(out):
        assert np.array_equal(NP(out[1])[r], ri), "indices differ from the oracle"
        assert np.array_equal(NP(out[0])[r].view(np.int32), rs.view(np.int32)), "score bits differ from the oracle"
    return verify


# ---- exact top-k: one shape per layout of tests/test_cpu_topk_workspace.py, at the smallest N that reaches it -----------------
def _exact(B, N, D, k, packed=False):
    def factory(dev):
        from ragraph_amd import kernels as K

        rng = np.random.default_rng(B * 7 + N + D + k)
        kn = _bank(rng, N, D)
        if N > 100:
            kn[N // 2:N // 2 + 20] = kn[:20]          # exact duplicates: ties in canonical order
        q = rng.standard_normal((B, D), dtype=np.float32)
        if B > 2:
            q[2] = 0.0
        qd, knd = T(q, dev), T(kn, dev)
        kp = K.pack_keys(knd) if packed else None
        return (lambda: K.topk_cosine(qd, knd, k, idx_base=5, keys_packed=kp)), _verify_topk(q, kn, k, 5)
    return factory


SLAB0, SLAB_RULE = {"RAGRAPH_TOPK_SLAB": "0"}, {"RAGRAPH_TOPK_SLAB": None}
case("topk_cosine", "streaming-16x1000x256", SLAB0)(_exact(16, 1000, 256, 10))
case("topk_cosine", "streaming-by-shape-7x8200x64", SLAB_RULE)(_exact(7, 8200, 64, 5))
case("topk_cosine", "streaming-largest-k-4x3000x256", SLAB0)(_exact(4, 3000, 256, 31))
case("topk_cosine", "tile-k32-50x3000x256", SLAB0)(_exact(50, 3000, 256, 32))
case("topk_cosine", "tile-129x3001x128", SLAB0)(_exact(129, 3001, 128, 10))
case("topk_cosine", "tile-packed-bank-129x3000x256", SLAB0)(_exact(129, 3000, 256, 10, packed=True))
case("topk_cosine", "slabs-by-rule-16x1000x256", SLAB_RULE)(_exact(16, 1000, 256, 10))
case("topk_cosine", "slabs-by-width-3x10x8", SLAB_RULE)(_exact(3, 10, 8, 1))
case("topk_cosine", "slabs-by-width-17x333x96", SLAB_RULE)(_exact(17, 333, 96, 10))
case("topk_cosine", "slabs-by-k-9x500x256", SLAB_RULE)(_exact(9, 500, 256, 33))
case("topk_cosine", "large-k-3x300x64", SLAB_RULE)(_exact(3, 300, 64, 65))
case("topk_cosine", "large-k-one-query-1x1000x64", SLAB_RULE)(_exact(1, 1000, 64, 200))


def _mix(B, N, D, A, k, w=(0.3, 0.7)):
    def factory(dev):
        from ragraph_amd import kernels as K

        cref = _cref()
        rng = np.random.default_rng(B + N + D + A + k)
        kn = _bank(rng, N, D)
        q = rng.standard_normal((B, D), dtype=np.float32)

        def codes(n):   # the reference's form: 1 / (d + 1), 0 for an anchor out of reach, some rows all zero
            c = (1.0 / (rng.integers(0, 7, (n, A)).astype(np.float32) + 1.0)).astype(np.float32)
            c[rng.random((n, A)) < 0.3] = 0.0
            c[rng.random(n) < 0.03] = 0.0
            return c
        pq, pnn = codes(B), cref.normalize_rows(codes(N))
        s = cref.axpby(cref.linear(cref.normalize_rows(pq), pnn), np.float32(w[0]), cref.linear(cref.normalize_rows(q), kn),
                       np.float32(w[1]))
        rs, ri = cref.topk_rows(s, k)
        qd, knd, pqd, pnd = T(q, dev), T(kn, dev), T(pq, dev), T(pnn, dev)

        def verify(out):
            assert np.array_equal(NP(out[1]), ri + 1000) and np.array_equal(NP(out[0]).view(np.int32), rs.view(np.int32))
        return (lambda: K.topk_cosine_mix(qd, knd, pqd, pnd, w[0], w[1], k, idx_base=1000)), verify
    return factory


case("topk_cosine_mix", "streaming-16x1000x256", SLAB0)(_mix(16, 1000, 256, 10, 10))
case("topk_cosine_mix", "tile-129x3001x128", SLAB0)(_mix(129, 3001, 128, 16, 5))
case("topk_cosine_mix", "tile-k32-50x3000x64", SLAB0)(_mix(50, 3000, 64, 1, 32))
case("topk_cosine_mix", "slabs-by-rule-16x1000x256", SLAB_RULE)(_mix(16, 1000, 256, 10, 10))
case("topk_cosine_mix", "slabs-by-width-17x333x96", SLAB_RULE)(_mix(17, 333, 96, 16, 10))
case("topk_cosine_mix", "slabs-by-k-9x500x256", SLAB_RULE)(_mix(9, 500, 256, 1, 33))
case("topk_cosine_mix", "large-k-3x300x64", SLAB_RULE)(_mix(3, 300, 64, 4, 65))


def _masked(B, N, D, k, hist_kind):
    def factory(dev):
        from ragraph_amd import kernels as K

        cref = _cref()
        rng = np.random.default_rng(B + N + D + k)
        nU = B + 7
        ue = rng.standard_normal((nU, D)).astype(np.float32)
        ie = rng.standard_normal((N, D)).astype(np.float32)
        if N > 8:
            ie[5] = ie[3]
            ie[N - 1] = ie[3]
        users = rng.integers(0, nU, B)
        if hist_kind == "empty":
            hist = [[] for _ in range(B)]
        elif hist_kind == "one-user":          # one user holds the whole history: all but 3 items, descending, some twice
            hist = [[] for _ in range(B)]
            keep = rng.choice(N, min(3, N - 1), replace=False)
            h = np.setdiff1d(np.arange(N), keep)[::-1].tolist()
            hist[B // 2] = h + h[: len(h) // 3]
        else:                                   # unsorted, duplicates, every query some
            hist = [rng.integers(0, N, int(rng.integers(0, min(N, 30)))).tolist() for _ in range(B)]
            hist[0] = []
        rowptr = np.concatenate([[0], np.cumsum([len(x) for x in hist])]).astype(np.int64)
        items = np.concatenate([np.asarray(x, dtype=np.int64) for x in hist]) if rowptr[-1] else np.zeros(0, np.int64)
        S = cref.linear(ue[users], ie)
        for b in range(B):
            S[b, np.asarray(hist[b], dtype=np.int64)] = MASK
        rs, ri = cref.topk_rows(S, k)
        args = (T(ue, dev), T(ie, dev), k, T(rowptr, dev), T(items, dev))
        ud = T(users, dev)

        def verify(out):
            assert np.array_equal(NP(out[1]), ri) and np.array_equal(NP(out[0]).view(np.int32), rs.view(np.int32))
        return (lambda: K.topk_dot_masked(*args, users=ud)), verify
    return factory


for _env, _tag in ((SLAB_RULE, "slab-rule"), (SLAB0, "fused")):
    case("topk_dot_masked", f"empty-history-7x4099x64-{_tag}", _env)(_masked(7, 4099, 64, 20, "empty"))
    case("topk_dot_masked", f"one-user-holds-the-history-33x2000x64-{_tag}", _env)(
        _masked(33, 2000, 64, 20, "one-user"))
    case("topk_dot_masked", f"more-queries-than-keys-300x10x64-{_tag}", _env)(_masked(300, 10, 64, 10, "mixed"))
    case("topk_dot_masked", f"tile-513x3001x128-{_tag}", _env)(_masked(513, 3001, 128, 20, "mixed"))
case("topk_dot_masked", "slabs-by-width-33x2000x48", SLAB_RULE)(_masked(33, 2000, 48, 20, "mixed"))
case("topk_dot_masked", "slabs-by-k-7x4099x64", SLAB_RULE)(_masked(7, 4099, 64, 64, "mixed"))


# ---- filtered top-k: one case per entry and per class of plan (tests/test_gpu_filter_call_plans.py names the shapes) ----------
def _filtered(B, N, D, k, bank="random", zero_queries=False, exchange_shards=0, stats=True, idx_base=9, ref_rows=256,
              prior=None, tight=None, repair=None, levels=None, level0=None):
    """levels: the class of plan the case is named after -- the dtype of every level the call must have run (decoded from its
    statistics words); level0: what the plan query must report as the first bound (0 the tile kernel's exact level 0, 1 an
    exact level 0 as a slab, 2 the bound pass).  A schedule change that moves a case off its class fails here.
    prior: "low" (just below every query's k-th best: no miss) or "median" (half of the queries miss and take the exact
    scan); tight: with a low prior, the tight bound at the tight-th lowest k-th best (so many soft misses: up to 256 are
    repaired by a compact call that carves its buffers from the idle lists, more by one more level) -- `repair` = the
    statistics word [23] that names which."""
    def factory(dev):
        from ragraph_amd import kernels as K

        cref = _cref()
        rng = np.random.default_rng(B + N + D + k)
        if bank == "near-duplicates":          # thousands of keys within eps of every query's k-th best: the lists overflow
            base = rng.standard_normal((1, D), dtype=np.float32)
            kn = cref.normalize_rows(base + 1e-3 * rng.standard_normal((N, D), dtype=np.float32))
            q = np.concatenate([base + 1e-3 * rng.standard_normal((B - 51, D), dtype=np.float32), np.zeros((1, D), np.float32),
                                rng.standard_normal((50, D), dtype=np.float32)]).astype(np.float32)
        else:
            kn = _bank(rng, N, D)
            kn[N // 2:N // 2 + 40] = kn[:40]
            q = rng.standard_normal((B, D), dtype=np.float32)
            q[0] = 2.5 * kn[N - 1]
            if zero_queries:
                q[:] = 0.0
            elif B > 1:
                q[B - 1] = 0.0
        qd, knd = T(q, dev), T(kn, dev)
        kb = K.keys_to_bf16(knd)
        kw = {}
        if exchange_shards:
            def exchange(phase, theta, scores):   # the no-op exchange: this shard alone sharpens its bounds
                pass
            exchange.n_shards = exchange_shards
            kw = {"exchange": exchange}

        rows = None if B <= ref_rows else np.unique(np.concatenate([[0, 1, 2, B - 1], rng.integers(0, B, ref_rows)]))
        vt = _verify_topk(q, kn, k, idx_base, rows)
        p = t = None
        if prior is not None:
            assert rows is None
            kth = np.sort(cref.topk_cosine(q[np.abs(q).sum(1) > 0], kn, k)[0][:, k - 1])
            p = float(kth[0]) - 0.01 if prior == "low" else float(kth[kth.size // 2])
            t = None if tight is None else float(kth[tight])

        def run():
            K.set_filter_prior(p)
            K.set_filter_tight_prior(t)
            try:
                out = K.topk_cosine_filtered(qd, knd, kb, k, idx_base=idx_base, return_stats=stats, **kw)
                if not stats:
                    return out
                s, i, over, st = out
                words = st.cpu().tolist()        # THIS call's statistics words, read before the next call
            finally:
                K.set_filter_prior(None)
                K.set_filter_tight_prior(None)
            return (s, i, over, [(dt, keys) for dt, keys, _ in K.filter_stats_levels(words)], words[:2],
                    [words[16], words[17], words[21], words[22], words[23]])

        def verify(out):
            vt(out)
            if bank == "near-duplicates":
                assert int(out[2]) >= B - 50
            if stats:
                assert out[4][0] == K.FILTER_STATS_MAGIC and 1 <= out[4][1] <= 3
                ran = tuple(dt for dt, _ in out[3])
                assert ran == tuple(levels) and out[4][1] == len(levels), f"the call ran levels {ran}, the case declares {levels}"
                if level0 is not None:
                    L = K.N.lib()
                    plan = (ctypes.c_int64 * 7)()
                    assert L.ragraph_topk_cosine_filtered_plan(B, N, D, k, plan) == len(levels) and plan[1] == level0, list(plan)
                spec, hard, tight_on, soft, repaired = out[5]
                if not exchange_shards:
                    assert spec == (prior is not None) and tight_on == (tight is not None)
                if prior == "low":
                    assert hard == 0
                if prior == "median":
                    assert hard >= B // 2 - 2 and int(out[2]) >= hard
                if tight is not None:
                    assert soft == tight and repaired == repair
        return run, verify
    return factory


I8, BF = ("int8",), ("bf16",)
case("topk_cosine_filtered", "direct-one-i8-level-7x70000x256")(_filtered(7, 70000, 256, 10, levels=I8, level0=2))
case("topk_cosine_filtered", "direct-two-i8-levels-64x100000x128")(_filtered(64, 100000, 128, 10, levels=I8 * 2, level0=2))
case("topk_cosine_filtered", "direct-three-bf16-levels-k32-1x65536x256")(_filtered(1, 65536, 256, 32, levels=BF * 3, level0=2))
case("topk_cosine_filtered", "direct-scored-one-i8-level-200x70000x256")(_filtered(200, 70000, 256, 10, levels=I8, level0=2))
case("topk_cosine_filtered", "ring-one-bf16-level-300x40000x256")(_filtered(300, 40000, 256, 10, levels=BF, level0=2))
case("topk_cosine_filtered", "ring-two-bf16-levels-3000x20000x128")(_filtered(3000, 20000, 128, 10, levels=BF * 2, level0=2))
case("topk_cosine_filtered", "ring-one-i8-level-scored-2100x70000x256")(_filtered(2100, 70000, 256, 10, levels=I8, level0=2))
case("topk_cosine_filtered", "exact-level0-tile-300x5000x256")(_filtered(300, 5000, 256, 10, levels=BF, level0=0))
case("topk_cosine_filtered", "exact-level0-slab-two-bf16-levels-300x20000x64")(
    _filtered(300, 20000, 64, 32, levels=BF * 2, level0=1))
case("topk_cosine_filtered", "one-i8-level-forced-513x33000x128", {"RAGRAPH_FILTER_I8": "3"})(
    _filtered(513, 33000, 128, 7, levels=I8))
# (three levels, the last two int8: the most int8 levels of any recorded plan -- tests/test_gpu_filter_call_plans.py; forcing
# int8 on every level, as above, collapses the schedule of a small shape to one level)
case("topk_cosine_filtered", "three-levels-two-i8-17000x200000x128")(
    _filtered(17000, 200000, 128, 10, levels=BF + I8 * 2, level0=2))
case("topk_cosine_filtered", "overflowing-bank-two-bf16-levels-351x20000x256")(
    _filtered(351, 20000, 256, 10, bank="near-duplicates", idx_base=0, ref_rows=400, levels=BF * 2, level0=2))
case("topk_cosine_filtered", "all-zero-queries-40x70000x256")(
    _filtered(40, 70000, 256, 10, zero_queries=True, levels=I8, level0=2))
case("topk_cosine_filtered", "ring-under-a-prior-300x40000x256")(
    _filtered(300, 40000, 256, 10, prior="low", ref_rows=600, levels=BF))
case("topk_cosine_filtered", "direct-under-a-prior-7x70000x256")(
    _filtered(7, 70000, 256, 10, prior="low", ref_rows=600, levels=I8))
case("topk_cosine_filtered", "prior-too-high-for-half-of-the-queries-300x40000x256")(
    _filtered(300, 40000, 256, 10, prior="median", ref_rows=600, levels=BF))
case("topk_cosine_filtered", "tight-bound-compact-repair-300x70000x256")(
    _filtered(300, 70000, 256, 10, prior="low", tight=100, repair=1, ref_rows=600, levels=BF))
case("topk_cosine_filtered", "tight-bound-one-more-level-600x70000x256")(
    _filtered(600, 70000, 256, 10, prior="low", tight=300, repair=2, ref_rows=600, levels=BF))
case("topk_cosine_filtered", "wide-direct-one-i8-level-9x70000x256-k33")(_filtered(9, 70000, 256, 33, levels=I8, level0=2))
case("topk_cosine_filtered", "wide-ring-two-bf16-levels-700x20000x128-k64")(
    _filtered(700, 20000, 128, 64, levels=BF * 2, level0=1))
case("topk_cosine_filtered", "wide-ring-one-bf16-level-300x70000x256-k48")(_filtered(300, 70000, 256, 48, levels=BF, level0=2))
case("topk_cosine_filtered", "wide128-direct-one-i8-level-9x70000x256-k65")(_filtered(9, 70000, 256, 65, levels=I8, level0=2))
case("topk_cosine_filtered", "wide128-ring-two-bf16-levels-700x20000x128-k128")(
    _filtered(700, 20000, 128, 128, levels=BF * 2, level0=0))
case("topk_cosine_filtered", "sharded-noop-exchange-1-shard-300x40000x256")(
    _filtered(300, 40000, 256, 10, exchange_shards=1, levels=BF))
case("topk_cosine_filtered", "sharded-noop-exchange-2-shards-300x40000x256")(
    _filtered(300, 40000, 256, 10, exchange_shards=2, levels=BF))
case("topk_cosine_filtered", "sharded-noop-exchange-2-shards-direct-7x70000x256")(
    _filtered(7, 70000, 256, 10, exchange_shards=2, levels=I8))


def _fused(B, N, D, k, bank="random"):
    def factory(dev):
        from ragraph_amd import kernels as K

        cref = _cref()
        rng = np.random.default_rng(D + B + N + k)
        if bank == "near-duplicates":
            base = rng.standard_normal((1, D), dtype=np.float32)
            kn = cref.normalize_rows(base + 1e-3 * rng.standard_normal((N, D), dtype=np.float32))
            q = np.concatenate([base + 1e-3 * rng.standard_normal((B - 31, D), dtype=np.float32), np.zeros((1, D), np.float32),
                                rng.standard_normal((30, D), dtype=np.float32)]).astype(np.float32)
        else:
            kn = _bank(rng, N, D)
            kn[N // 2:N // 2 + 40] = kn[:40]
            q = rng.standard_normal((B, D), dtype=np.float32)
            q[B // 2] = 3.0 * kn[7]
        qd, knd = T(q, dev), T(kn, dev)
        kb = K.keys_to_bf16(knd)
        return (lambda: K.topk_cosine_fused(qd, knd, kb, k, idx_base=11)), _verify_topk(q, kn, k, 11)
    return factory


case("topk_cosine_fused", "one-query-1x640x64")(_fused(1, 640, 64, 1))
case("topk_cosine_fused", "ragged-33x1113x256")(_fused(33, 1113, 256, 3))
case("topk_cosine_fused", "largest-k-300x4100x256")(_fused(300, 4100, 256, 16))
case("topk_cosine_fused", "overflowing-bank-71x6000x128")(_fused(71, 6000, 128, 10, bank="near-duplicates"))


def _small(B, N, D, k, cap):
    def factory(dev):
        from ragraph_amd import kernels as K

        rng = np.random.default_rng(7 * D + B + N + k)
        kn = _bank(rng, N, D)
        kn[N // 2:N // 2 + 40] = kn[:40]
        q = rng.standard_normal((B, D), dtype=np.float32)
        q[0] = 2.5 * kn[11]
        if B > 2:
            q[B - 1] = 0.0
        qd, knd = T(q, dev), T(kn, dev)
        kb = K.keys_to_bf16(knd)

        def run():
            old = K.set_max_i8_levels(cap)
            try:
                s, i, over, st = K.topk_cosine_small(qd, knd, kb, k, idx_base=5, return_stats=True)
                words = st.cpu().tolist()
            finally:
                K.set_max_i8_levels(old)
            assert int(K._small_state_buf(qd.device).abs().sum()) == 0     # every call leaves the state words zero
            return s, i, over, words[16:18]

        vt = _verify_topk(q, kn, k, 5)

        def verify(out):
            vt(out)
            assert int(out[2]) == 0
        return run, verify
    return factory


case("topk_cosine_small", "one-query-i8-1x65536x256")(_small(1, 65536, 256, 10, -1))
case("topk_cosine_small", "32-queries-k32-bf16-32x70001x256")(_small(32, 70001, 256, 32, 0))
case("topk_cosine_small", "d64-20x70000x64")(_small(20, 70000, 64, 10, -1))
case("topk_cosine_small", "d128-9x70000x128")(_small(9, 70000, 128, 7, -1))


def _tail(D, k, B, Tn, padded=False):
    def factory(dev):
        from ragraph_amd import kernels as K

        cref = _cref()
        rng = np.random.default_rng(D * 1000 + k * 10 + B + Tn)
        n_seed = 5 if padded else 3000
        other = _bank(rng, n_seed, D)
        q = rng.standard_normal((B, D), dtype=np.float32)
        q[0] = other[3] * 2.5
        if B > 2:
            q[2] = 0
        tail = _bank(rng, Tn, D)
        tail[0] = other[3]                              # a copy of query 0's best seed row: ties it, loses on the index
        if Tn > 1:
            tail[1] = cref.normalize_rows(q[B - 1:B])[0]
        if Tn > 2:
            tail[2] = 0
        ks = min(k, n_seed)
        s0, i0 = cref.topk_cosine(q, other, ks, idx_base=5)        # the seed: the oracle's list over the other rows
        seed_s = np.full((B, k), -np.inf, dtype=np.float32)
        seed_i = np.full((B, k), I64_MAX, dtype=np.int64)
        seed_s[:, :ks], seed_i[:, :ks] = s0, i0
        n = min(k, n_seed + Tn)
        rs, ri = cref.topk_cosine(q, np.concatenate([other, tail]), n, idx_base=5)
        qd, td, ssd, sid = T(q, dev), T(tail, dev), T(seed_s, dev), T(seed_i, dev)

        def verify(out):
            s, i = NP(out[0]), NP(out[1])
            assert np.array_equal(i[:, :n], ri) and np.array_equal(s[:, :n].view(np.int32), rs.view(np.int32))
            assert (i[:, n:] == I64_MAX).all() and np.isneginf(s[:, n:]).all()
        return (lambda: K.topk_cosine_tail(qd, td, ssd, sid, 5 + n_seed)), verify
    return factory


case("topk_cosine_tail", "T1-1x1-d64")(_tail(64, 1, 1, 1))
case("topk_cosine_tail", "T40-17x10-d128")(_tail(128, 10, 17, 40))
case("topk_cosine_tail", "T40-padded-seed-17x10-d128")(_tail(128, 10, 17, 40, padded=True))
case("topk_cosine_tail", "T3-padded-seed-17x10-d128")(_tail(128, 10, 17, 3, padded=True))
case("topk_cosine_tail", "T4097-k64-300-d256")(_tail(256, 64, 300, 4097))
case("topk_cosine_tail", "T4097-k33-3-d64-slices")(_tail(64, 33, 3, 4097))


# ---- dedup --------------------------------------------------------------------------------------------------------------------
def _dedup(N, D, kind):
    def factory(dev):
        from ragraph_amd import kernels as K

        cref = _cref()
        rng = np.random.default_rng(N + D)
        if kind == "identical":
            kn = np.repeat(_bank(rng, 1, D), N, axis=0)
        elif kind == "distinct":
            kn = _bank(rng, N, D)
        else:                                            # groups of every size, -0.0 against +0.0 (different bits)
            kn = _bank(rng, N // 7 + 1, D)[rng.integers(0, N // 7 + 1, N)]
            kn[3] = 0.0
            kn[4] = -0.0
        U, largest, uniq, gptr, members = cref.dedup_rows(kn)
        knd = T(kn, dev)

        def verify(out):
            assert (out[0], out[1]) == (U, largest)
            assert np.array_equal(NP(out[2]), uniq) and np.array_equal(NP(out[3]), gptr) and np.array_equal(NP(out[4]), members)
        return (lambda: K.dedup_rows(knd)), verify
    return factory


case("dedup_rows", "all-rows-identical-4097x64")(_dedup(4097, 64, "identical"))
case("dedup_rows", "all-rows-distinct-4097x64")(_dedup(4097, 64, "distinct"))
case("dedup_rows", "groups-2049x8")(_dedup(2049, 8, "groups"))
case("dedup_rows", "one-row-1x256")(_dedup(1, 256, "distinct"))


# ---- dense ----------------------------------------------------------------------------------------------------------------------
def _linear_tn(n, M, Nn):
    def factory(dev):
        from ragraph_amd import kernels as K

        g = torch.Generator().manual_seed(n + M + Nn)
        a, b = torch.randn(n, M, generator=g), torch.randn(n, Nn, generator=g)
        ref = a.double().t() @ b.double()
        ad, bd = a.to(dev), b.to(dev)

        def verify(out):     # (tests/test_gpu_backward.py's bound: 1e-5 of the largest entry x sqrt of the rows summed / 8)
            err = float((out[0].cpu().double() - ref).abs().max())
            assert err <= 1e-5 * max(1.0, float(ref.abs().max())) * max(1.0, n ** 0.5 / 8), err
        return (lambda: (K.linear_tn(ad, bd),)), verify
    return factory


for _n in (2048, 2049, 4097):
    case("linear_tn", f"{_n}x1x1")(_linear_tn(_n, 1, 1))
    case("linear_tn", f"{_n}x130x70")(_linear_tn(_n, 130, 70))


# ---- sparse: long rows ------------------------------------------------------------------------------------------------------------
_long_graphs = {}


def _long_graph():
    """Every row exactly 4097 edges (the most long rows and block tasks per non-zero the layout allows), and one of
    3 * 4096 + 5."""
    if "g" not in _long_graphs:
        rng = np.random.default_rng(41)
        deg = np.full(24, 4097, dtype=np.int64)
        deg[11] = 3 * 4096 + 5
        rowptr = np.zeros(deg.size + 1, dtype=np.int64)
        rowptr[1:] = np.cumsum(deg)
        nnz, ncols = int(rowptr[-1]), 700
        col = rng.integers(0, ncols, nnz).astype(np.int32)
        val = rng.random(nnz, dtype=np.float32) - 0.3
        _long_graphs["g"] = (rowptr, col, val, ncols)
    return _long_graphs["g"]


def _spmm_long(D):
    def factory(dev):
        from ragraph_amd import kernels as K

        cref = _cref()
        rowptr, col, val, ncols = _long_graph()
        n = rowptr.size - 1
        rng = np.random.default_rng(500 + D)
        X = rng.standard_normal((ncols, D), dtype=np.float32)
        b = rng.standard_normal(D, dtype=np.float32)
        Yin = rng.standard_normal((n, D), dtype=np.float32)
        ref = cref.spmm_csr(rowptr, col, val, X, bias=b, act=2, alpha=0.25, beta=0.5, Y_in=Yin)
        args = (T(rowptr, dev), T(col, dev), T(val, dev), T(X, dev))
        bd, yd = T(b, dev), T(Yin, dev)

        def verify(out):
            assert np.array_equal(NP(out[0]).view(np.int32), ref.view(np.int32))
        return (lambda: (K.spmm_csr(*args, bias=bd, act=2, alpha=0.25, beta=0.5, y_in=yd, long_rows=True),)), verify
    return factory


def _spmm_prelu_dev(D):
    def factory(dev):
        from ragraph_amd import kernels as K

        cref = _cref()
        rowptr, col, val, ncols = _long_graph()
        rng = np.random.default_rng(600 + D)
        X = rng.standard_normal((ncols, D), dtype=np.float32)
        b = rng.standard_normal(D, dtype=np.float32)
        ref_y = cref.spmm_csr(rowptr, col, val, X, bias=b, act=2, alpha=0.25)
        ref_z = cref.spmm_csr(rowptr, col, val, X, bias=b, act=0)
        args = (T(rowptr, dev), T(col, dev), T(val, dev), T(X, dev), T(b, dev), torch.tensor([0.25], device=dev))

        def verify(out):
            assert np.array_equal(NP(out[0]).view(np.int32), ref_y.view(np.int32))
            assert np.array_equal(NP(out[1]).view(np.int32), ref_z.view(np.int32))
        return (lambda: K.spmm_csr_prelu_dev(*args, want_z=True, long_rows=True)), verify
    return factory


for _D in (4, 64, 256):
    case("spmm_csr", f"all-rows-4097-edges-D{_D}")(_spmm_long(_D))
    case("spmm_csr_prelu_dev", f"all-rows-4097-edges-D{_D}")(_spmm_prelu_dev(_D))


@case("segment_softmax", "all-rows-4097-edges")
def _segment_softmax_long(dev):
    from ragraph_amd import kernels as K

    cref = _cref()
    rowptr, col, val, ncols = _long_graph()
    x = np.random.default_rng(7).standard_normal(int(rowptr[-1])).astype(np.float32)
    ref = cref.segment_softmax(rowptr, x)
    rp, xd = T(rowptr, dev), T(x, dev)

    def verify(out):     # (expf: host and device libm differ -- the existing test's tolerance)
        got = NP(out[0])
        assert np.allclose(got, ref, rtol=1e-6, atol=1e-9)
        assert np.allclose(np.add.reduceat(got, rowptr[:-1]), 1.0, atol=1e-4)
    return (lambda: (K.segment_softmax(rp, xd, long_rows=True),)), verify


_rows_graphs = {}


def _rows_graph():
    """2000 rows: lengths at and around the 16-edge chunk and the 4096-edge block at known rows, 0-8 edges elsewhere."""
    if "g" not in _rows_graphs:
        rng = np.random.default_rng(1)
        n = 2000
        deg = rng.integers(0, 9, n)
        at = (1801, 17, 842, 0, 1999, 311, 1000, 1555, 520)
        deg[list(at)] = (0, 1, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 5)
        rowptr = np.zeros(n + 1, dtype=np.int64)
        rowptr[1:] = np.cumsum(deg)
        col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
        val = rng.standard_normal(col.size).astype(np.float32)
        _rows_graphs["g"] = (rowptr, col, val, n)
    return _rows_graphs["g"]


def _spmm_rows(rows, D):
    def factory(dev):
        from ragraph_amd import kernels as K

        cref = _cref()
        rowptr, col, val, n = _rows_graph()
        X = np.random.default_rng(D).standard_normal((n, D)).astype(np.float32)
        ref = cref.spmm_csr(rowptr, col, val, X)[np.asarray(rows)]
        if len(rows) == 40:
            assert 40 + col.size // 4096 + 1 < 3 * 40      # more block sums asked than the partial-sum area holds
        args = (T(rowptr, dev), T(col, dev), T(val, dev), T(X, dev), torch.tensor(rows, device=dev))

        def verify(out):
            assert np.array_equal(NP(out[0]).view(np.int32), ref.view(np.int32))
        return (lambda: (K.spmm_csr_rows(*args, long_rows=True),)), verify
    return factory


case("spmm_csr_rows", "same-hub-40-times-D64")(_spmm_rows([520] * 40, 64))
case("spmm_csr_rows", "one-hub-row-D64")(_spmm_rows([520], 64))
case("spmm_csr_rows", "one-empty-row-D8")(_spmm_rows([1801], 8))
case("spmm_csr_rows", "scrambled-rows-D256")(
    _spmm_rows([1555, 17, 520, 1801, 0, 520, 311, 1000, 1999, 842], 256))


# ---- the scan and what sits on it ---------------------------------------------------------------------------------------------
SCAN_SIZES = (1024, 1025, 1024 * 1024, 1024 * 1024 + 1)      # the last one reaches the third level of sums


def _mask_positions(E, p):
    def factory(dev):
        from ragraph_amd import kernels as K

        rng = np.random.default_rng(E + 7)
        mask = (rng.random(E) < p) if p < 1 else np.ones(E, dtype=bool)
        ref = np.nonzero(mask)[0].astype(np.int64)
        md = T(mask, dev)

        def verify(out):
            assert np.array_equal(NP(out[0]), ref)
        return (lambda: (K.mask_positions(md),)), verify
    return factory


for _E in SCAN_SIZES:
    case("mask_positions", f"E{_E}")(_mask_positions(_E, 0.5))
case("mask_positions", "E1-set")(_mask_positions(1, 1.0))
case("mask_positions", f"E{SCAN_SIZES[3]}-all-set")(_mask_positions(SCAN_SIZES[3], 1.0))


def _csr_rows_edges(R):
    def factory(dev):
        from ragraph_amd import kernels as K

        rng = np.random.default_rng(R)
        n = 3000
        deg = rng.integers(0, 3, n)
        deg[5] = 70
        rowptr = np.zeros(n + 1, dtype=np.int64)
        rowptr[1:] = np.cumsum(deg)
        col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
        val = rng.standard_normal(col.size).astype(np.float32)
        rows = rng.integers(0, n, R)
        rows[R // 2] = 5
        lens = deg[rows]
        off = np.concatenate([[0], np.cumsum(lens)])
        r = np.repeat(np.arange(R), lens)
        slot = rowptr[rows][r] + (np.arange(off[-1]) - off[:-1][r])       # CSR order inside a row, ascending position
        args = (T(rowptr, dev), T(col, dev), T(val, dev), T(rows, dev))

        def verify(out):
            assert np.array_equal(NP(out[0]), col[slot].astype(np.int64)) and np.array_equal(NP(out[1]), r)
            assert np.array_equal(NP(out[2]).view(np.int32), val[slot].view(np.int32))
        return (lambda: K.csr_rows_edges(*args)), verify
    return factory


for _R in SCAN_SIZES:
    case("csr_rows_edges", f"R{_R}")(_csr_rows_edges(_R))
case("csr_rows_edges", "R1")(_csr_rows_edges(1))


# ---- radix sort behind ingestion ------------------------------------------------------------------------------------------------
def _coo_to_csr(E, n, sort_cols):
    def factory(dev):
        from ragraph_amd import kernels as K

        rng = np.random.default_rng(E + n)
        rows = rng.integers(0, n, E)
        cols = rng.integers(0, n, E)
        if E > 100:
            rows[E // 2:E // 2 + 5] = rows[E // 2]       # duplicate pairs: the stable order decides
            cols[E // 2:E // 2 + 5] = cols[E // 2]
        key = rows * n + cols if sort_cols else rows
        perm = np.argsort(key, kind="stable").astype(np.int64)
        rowptr = np.zeros(n + 1, dtype=np.int64)
        rowptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
        rd, cd = T(rows, dev), T(cols, dev)

        def verify(out):
            assert np.array_equal(NP(out[0]), rowptr) and np.array_equal(NP(out[2]), perm)
            assert np.array_equal(NP(out[1]), cols[perm].astype(np.int32))
        return (lambda: K.coo_to_csr(rd, cd, n, sort_cols=sort_cols)), verify
    return factory


for _sc in (False, True):
    case("coo_to_csr", f"E1-n1-sort_cols={_sc}")(_coo_to_csr(1, 1, _sc))
    case("coo_to_csr", f"E-much-larger-than-n-{2048 * 40 + 1}x37-sort_cols={_sc}")(_coo_to_csr(2048 * 40 + 1, 37, _sc))
    case("coo_to_csr", f"n-much-larger-than-E-{2048 - 1}x300000-sort_cols={_sc}")(_coo_to_csr(2048 - 1, 300_000, _sc))
    case("coo_to_csr", f"E{2048 * 3 + 1}-n1025-sort_cols={_sc}")(_coo_to_csr(2048 * 3 + 1, 1025, _sc))


def _sym_normalized(E, n):
    def factory(dev):
        from ragraph_amd import kernels as K
        from ragraph_amd.graph import CSRGraph

        rng = np.random.default_rng(E * 3 + n)
        ei = rng.integers(0, n, (2, E))
        if E > 100:
            ei[:, E // 2:E // 2 + 50] = ei[:, :50]       # duplicates: multiplicity 2 entries
        ref = CSRGraph.from_edge_index_sym_normalized(torch.from_numpy(ei), n)     # CPU tensors: the torch restatement
        eid = T(ei, dev)

        def verify(out):
            assert torch.equal(out[0].cpu(), ref.rowptr) and torch.equal(out[1].cpu(), ref.col)
            assert torch.equal(_bits(out[2].cpu()), _bits(ref.val))
        return (lambda: K.csr_sym_normalized_from_edges(eid, n)), verify
    return factory


case("csr_sym_normalized_from_edges", f"E{2048 * 4 - 1 - 1000}-n1000")(_sym_normalized(2048 * 4 - 1 - 1000, 1000))   # E + n = 2048 m - 1
case("csr_sym_normalized_from_edges", f"E{2048 * 4 + 1 - 1000}-n1000")(_sym_normalized(2048 * 4 + 1 - 1000, 1000))
case("csr_sym_normalized_from_edges", "E0-n5")(_sym_normalized(0, 5))
case("csr_sym_normalized_from_edges", "E1-n70000")(_sym_normalized(1, 70_000))


def _binorm(E, U, I, every_pair_twice):
    def factory(dev):
        from ragraph_amd import kernels as K
        from ragraph_amd.edge_data import binorm_edges

        rng = np.random.default_rng(E + U + I)
        u, i, step = rng.integers(0, U, E), rng.integers(0, I, E), rng.integers(1, 700, E)
        if every_pair_twice:
            u, i = np.concatenate([u, u]), np.concatenate([i, i])
            step = np.concatenate([step, rng.integers(1, 700, E)])
        e_ref, n_ref, t_ref = binorm_edges(U, I, u, i, step)                       # the numpy restatement
        args = (T(u, dev), T(i, dev), T(step, dev), U, I)

        def verify(out):
            assert np.array_equal(NP(out[0]), e_ref) and np.array_equal(NP(out[2]), t_ref)
            assert np.array_equal(NP(out[1]).view(np.int32), np.asarray(n_ref, dtype=np.float32).view(np.int32))
        return (lambda: K.binorm_edges(*args)), verify
    return factory


case("binorm_edges", "every-pair-duplicated-2x2049")(_binorm(2049, 300, 200, True))
case("binorm_edges", "E1")(_binorm(1, 3, 2, False))
case("binorm_edges", f"2E-at-2048m-minus-1-E{(2048 * 6) // 2 - 1}")(_binorm((2048 * 6) // 2 - 1, 3000, 2000, False))


# ---- row top-k ------------------------------------------------------------------------------------------------------------------
def _scores(B, N, seed):
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((B, N)).astype(np.float32)
    S[:, N // 3:N // 3 + 9] = S[:, :9]                  # ties
    return S


def _topk_rows_large(B, N, k):
    def factory(dev):
        from ragraph_amd import kernels as K

        S = _scores(B, N, B + N + k)
        rs, ri = _cref().topk_rows(S, k)
        Sd = T(S, dev)

        def verify(out):
            assert np.array_equal(NP(out[1]), ri) and np.array_equal(NP(out[0]).view(np.int32), rs.view(np.int32))
        return (lambda: K.topk_rows(Sd, k)), verify
    return factory


# (the first two select inside LDS: their size query is 0 and the wrapper passes an empty workspace)
case("topk_rows", "k-equals-N-3x65")(_topk_rows_large(3, 65, 65))
case("topk_rows", "k-equals-N-4x4096")(_topk_rows_large(4, 4096, 4096))
case("topk_rows", "long-rows-9x70001-k1000")(_topk_rows_large(9, 70001, 1000))


def _topk_select(B, N, k):
    def factory(dev):
        from ragraph_amd import kernels as K

        S = _scores(B, N, B + N + k + 1)
        kth, idx = _cref().topk_select_rows(S, k)
        Sd = T(S, dev)

        def verify(out):
            assert np.array_equal(NP(out[1]), idx) and np.array_equal(NP(out[0]).view(np.int32), kth.view(np.int32))
        return (lambda: K.topk_select_rows(Sd, k)), verify
    return factory


# (rows shorter than 65536 scores take the kernel without a workspace: (3, 65) and (4, 4096) stay on topk_rows above)
case("topk_select_rows", "k-equals-N-9x70001")(_topk_select(9, 70001, 70001))
case("topk_select_rows", "k1000-9x70001")(_topk_select(9, 70001, 1000))
case("topk_select_rows", "k-equals-N-1x65536")(_topk_select(1, 65536, 65536))


# ---- edge evaluation ------------------------------------------------------------------------------------------------------------
def _np_metrics(ranked, gt, ks, batch):
    """metrics.py:12-46 + 60-80 + 131-133 in float64 numpy (tests/test_gpu_edge_metric.py's reference)."""
    n = len(gt)
    out = {mm: np.zeros(len(ks)) for mm in ("recall", "ndcg", "precision")}
    for s in range(0, n, batch):
        rk, g = ranked[s:s + batch], gt[s:s + batch]
        r = np.array([[float(x in gg) for x in row] for row, gg in zip(rk, g)])
        rn = np.array([len(gg) for gg in g])
        for t, k in enumerate(ks):
            right = r[:, :k].sum(1)
            disc = 1. / np.log2(np.arange(2, k + 2))
            idcg = np.array([disc[:min(k, len(gg))].sum() for gg in g])
            idcg[idcg == 0.] = 1.
            out["recall"][t] += np.sum(right / rn) / n
            out["ndcg"][t] += np.sum((r[:, :k] * disc).sum(1) / idcg) / n
            out["precision"][t] += np.sum(right) / k / n
    return out


def _rank_metrics(U, ks, batch):
    def factory(dev):
        from ragraph_amd import kernels as K

        rng = np.random.default_rng(U + len(ks))
        n_items, kmax = 400, max(ks)
        ranked = np.stack([rng.permutation(n_items)[:kmax] for _ in range(U)]).astype(np.int64)
        gt = [set(rng.choice(n_items, int(rng.integers(1, 12)), replace=False).tolist()) for _ in range(U)]
        gt[0] = set(ranked[0, :3].tolist())             # a user whose whole ground truth is ranked first
        rowptr = np.concatenate([[0], np.cumsum([len(g) for g in gt])]).astype(np.int64)
        items = np.concatenate([np.sort(np.fromiter(g, dtype=np.int64)) for g in gt])
        ref = _np_metrics(ranked.tolist(), gt, ks, batch)
        args = (T(ranked, dev), T(rowptr, dev), T(items, dev), ks)

        def verify(out):
            for r, mm in enumerate(K.RANK_METRICS):
                assert np.allclose(out[0][r], ref[mm], rtol=0, atol=1e-12), mm
        return (lambda: (K.rank_metrics(*args, batch=batch),)), verify
    return factory


case("rank_metrics", "one-user")(_rank_metrics(1, [1, 5], 512))
case("rank_metrics", "257-users-batch-128-16-ks")(_rank_metrics(257, list(range(1, 32, 2)), 128))


# ---- bank construction ----------------------------------------------------------------------------------------------------------
def _pagerank(sizes):
    def factory(dev):
        from ragraph_amd import kernels as K

        cref = _cref()
        rng = np.random.default_rng(len(sizes))
        n = sum(sizes)
        a = np.zeros((n, n), np.float32)
        off = 0
        for gi, s in enumerate(sizes):
            if s == 1:
                b = np.full((1, 1), float(gi % 2), np.float32)      # a self loop, or a dangling node alone
            else:
                b = (rng.random((s, s)) < 0.1).astype(np.float32)
                b[rng.integers(0, s)] = 0                           # a dangling node
            a[off:off + s, off:off + s] = b
            off += s
        gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        rowptr, col, val = cref.dense_to_csr(a)
        rt, ct, vt = cref.dense_to_csr_t(a)
        out_deg = cref.csr_row_sums(rowptr, val)
        p_ref, it_ref = cref.pagerank(rt, ct, vt, out_deg, gp)
        args = (T(rt, dev), T(ct, dev), T(vt, dev), T(out_deg, dev), T(gp, dev))

        def verify(out):
            assert np.array_equal(NP(out[1]), it_ref) and np.array_equal(NP(out[0]).view(np.int32), p_ref.view(np.int32))
        return (lambda: K.pagerank(*args)), verify
    return factory


case("pagerank", "one-graph-300")(_pagerank([300]))
case("pagerank", "many-one-node-graphs-513")(_pagerank([1] * 513))
case("pagerank", "mixed-batch")(_pagerank([41, 1, 33, 7, 120, 2, 64]))


def _position_codes(n, A, rounds=None):
    def factory(dev):
        from ragraph_amd import kernels as K

        cref = _cref()
        rng = np.random.default_rng(n)
        a = (rng.random((n, n)) < 0.01).astype(np.float32) * rng.random((n, n)).astype(np.float32)
        a = np.maximum(a, a.T)
        np.fill_diagonal(a, 0.3)
        a[n // 2:, : n // 2] = 0                         # an unreachable half
        rowptr, col, val = cref.dense_to_csr(a)
        val = val.copy()
        val[::17] = 0.0
        anchors = rng.integers(0, n, A)
        if A > 3:
            anchors[3] = anchors[2]
        oc, od = cref.position_codes_csr(rowptr, col, val, anchors, 10.0)
        args = (T(rowptr, dev), T(col, dev), T(val, dev), T(anchors, dev), 10.0)

        def verify(out):
            assert np.array_equal(NP(out[1]).view(np.int32), od.view(np.int32))
            assert np.array_equal(NP(out[0]).view(np.int32), oc.view(np.int32))
            if rounds is not None:
                assert int(out[2]) == 1
        kw = {"method": "global", "return_dist": True}
        if rounds is not None:
            kw.update(rounds=rounds, return_converged=True)
        return (lambda: K.position_codes_csr(*args, **kw)), verify
    return factory


# (the global path takes any A >= 1 in chunks of 16 anchors: one anchor, a full chunk, one past it, three chunks)
case("position_codes_csr", "global-A1-n528")(_position_codes(528, 1))
case("position_codes_csr", "global-A16-n528")(_position_codes(528, 16))
case("position_codes_csr", "global-A17-n528")(_position_codes(528, 17))
case("position_codes_csr", "global-A48-n300-fixed-rounds")(_position_codes(300, 48, rounds=300))


def _edge_rewrite(sizes, kind):
    def factory(dev):
        from ragraph_amd import kernels as K

        rng = np.random.default_rng(len(sizes))
        gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n = int(gp[-1])
        prob = {"ones": np.ones(n, np.float32), "zeros": np.zeros(n, np.float32)}.get(kind)
        if prob is None:
            prob = (rng.random(n).astype(np.float32) ** 2 * 0.3).astype(np.float32)
        want_rowptr, want_col = BO.edge_rewrite(SEED, prob, gp)
        args = (T(prob, dev), T(gp, dev), torch.tensor([SEED], dtype=torch.int64, device=dev))

        def verify(out):
            assert np.array_equal(NP(out[0]), want_rowptr) and np.array_equal(NP(out[1]), want_col)
            assert out[2].numel() == out[1].numel() and bool((out[2] == 1.0).all())
        return (lambda: K.edge_rewrite_csr(*args)), verify
    return factory


case("edge_rewrite_csr", "one-node")(_edge_rewrite([1], "ones"))
case("edge_rewrite_csr", "wave-boundaries-random")(_edge_rewrite([1, 2, 63, 64, 65, 200], "random"))
case("edge_rewrite_csr", "wave-boundaries-every-slot")(_edge_rewrite([1, 2, 63, 64, 65, 200], "ones"))
case("edge_rewrite_csr", "no-slot-kept")(_edge_rewrite([1, 2, 63, 64, 65, 200], "zeros"))
case("edge_rewrite_csr", "n1025-one-graph")(_edge_rewrite([1025], "random"))


def _multinomial(sizes, S):
    def factory(dev):
        from ragraph_amd import kernels as K

        rng = np.random.default_rng(5)
        ps = []
        for s in sizes:
            p = rng.random(s).astype(np.float32)
            if s >= 64:
                p[rng.integers(0, s, s // 8)] = 0
                p[60:70] = 0
                p[0] = p[-1] = 0
            elif s == 2:
                p[0] = 0
            ps.append((p / max(p.sum(), 1e-30)).astype(np.float32))
        p, sp = np.concatenate(ps), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        want = BO.multinomial_segments(SEED, p, sp, S)
        args = (T(p, dev), T(sp, dev), S, torch.tensor([SEED], dtype=torch.int64, device=dev))

        def verify(out):
            assert np.array_equal(NP(out[0]), want)
        return (lambda: (K.multinomial_segments(*args),)), verify
    return factory


case("multinomial_segments", "one-entry-S1")(_multinomial([1], 1))
case("multinomial_segments", "segments-S10")(_multinomial([1, 2, 64, 65, 1000, 5000], 10))
case("multinomial_segments", "segments-S257")(_multinomial([1, 2, 64, 65, 1000, 5000], 257))
case("multinomial_segments", "n1025-one-segment-S257")(_multinomial([1025], 257))


def _blocks_to_csr(G, S):
    def factory(dev):
        from ragraph_amd import kernels as K

        rng = np.random.default_rng(G * 100 + S)
        b = (rng.random((G, S, S)) < 0.2).astype(np.float32) * (rng.random((G, S, S)).astype(np.float32) - 0.5)
        b[0] = 0                                         # an all-zero block
        b[1] = rng.random((S, S)).astype(np.float32) + 1   # a full block
        b[2, 0, 0] = -0.0                                # not an entry
        g, r, c = np.nonzero(b)                          # row-major: block, row, column
        rowptr = np.zeros(G * S + 1, dtype=np.int64)
        rowptr[1:] = np.cumsum(np.bincount(g * S + r, minlength=G * S))
        bd = T(b, dev)

        def verify(out):
            assert np.array_equal(NP(out[0]), rowptr) and np.array_equal(NP(out[1]), (g * S + c).astype(np.int32))
            assert np.array_equal(NP(out[2]).view(np.int32), b[g, r, c].view(np.int32))
        return (lambda: K.blocks_to_csr(bd)), verify
    return factory


for _G, _S in ((3, 1), (60, 64), (70, 64), (409, 10), (411, 10)):      # both sides of the 4096-row boundary, at both widths
    case("blocks_to_csr", f"G{_G}-S{_S}")(_blocks_to_csr(_G, _S))


# ---- link prediction and the edge flavour's pre-training ------------------------------------------------------------------------
def _lp_sample(n, n_neg, kind):
    def factory(dev):
        from ragraph_amd import kernels as K

        cref = _cref()
        rng = np.random.default_rng(n + n_neg)
        a = np.zeros((n, n), np.float32)
        if kind == "exact-complement":                   # row 0: exactly n_neg non-neighbours (0 .. n_neg - 1)
            a[0, n_neg:] = 1.0
            a[n_neg:, 0] = 1.0
        else:
            a = (rng.random((n, n)) < 0.05).astype(np.float32)
            a = np.maximum(a, a.T)
            np.fill_diagonal(a, 1.0)                     # self loops are ignored
            a[1, :] = a[:, 1] = 0                        # an isolated node
        rowptr, col, _ = cref.dense_to_csr(a)
        nb = a.astype(bool)
        np.fill_diagonal(nb, False)
        args = (T(rowptr, dev), T(col, dev), n_neg, torch.tensor([77], dtype=torch.int64, device=dev))

        def verify(out):     # (the sampler has no bit oracle: the rules of tests/test_gpu_lp_pretrain.py::test_sampler_rules)
            t = NP(out[0])
            assert t.shape == (n, 1 + n_neg) and ((t >= 0) & (t < n)).all()
            rows = np.arange(n)
            has = nb.any(1)
            assert nb[rows[has], t[has, 0]].all() and np.array_equal(t[~has, 0], rows[~has])
            neg = t[:, 1:]
            assert not nb[rows[:, None].repeat(n_neg, 1), neg].any()
            srt = np.sort(neg, axis=1)
            assert (srt[:, 1:] != srt[:, :-1]).all()
            if kind == "exact-complement":
                assert sorted(neg[0].tolist()) == list(range(n_neg))
        return (lambda: (K.lp_sample(*args),)), verify
    return factory


case("lp_sample", "three-nodes-one-negative")(_lp_sample(3, 1, "random"))
case("lp_sample", "exact-complement-300x100")(_lp_sample(300, 100, "exact-complement"))
case("lp_sample", "random-400x50")(_lp_sample(400, 50, "random"))


def _lp_compare_loss(n, S, D):
    def factory(dev):
        import torch.nn.functional as F

        from ragraph_amd import kernels as K

        g = torch.Generator().manual_seed(n + S + D)
        h = torch.randn(n, D, generator=g)
        t = torch.randint(0, n, (n, S), generator=g)
        if n > 8:
            h[3] = 0.0                                   # a zero row, also a partner
            t[:, 2] = 7                                  # a hub target
            t[::5, 1] = 3
        temperature = 1.5
        hd_ = h.double()
        sim = F.cosine_similarity(hd_[:, None, :].expand(n, S, D), hd_[t], dim=2)      # the reference's op chain, float64
        e = torch.exp(sim) / temperature
        Li = -torch.log(e[:, 0] / e[:, 1:].sum(1))
        nrm = hd_.norm(dim=1)
        hd, td = h.to(dev), t.to(dev)

        def verify(out):     # (loss, L [n], coef, csim, hhat, nrm): the existing test holds the loss to rel 1e-5
            assert float(out[0]) == pytest.approx(float(Li.mean()), rel=1e-5)
            assert torch.allclose(out[1].cpu().double(), Li, rtol=1e-5, atol=1e-6)
            # (a float32 chain over D terms: at most D * 2^-24 relative, 1.5e-5 at D = 256)
            assert torch.allclose(out[5].cpu().double(), nrm, rtol=2e-5, atol=0)
            assert torch.allclose(out[4].cpu().double(), hd_ / nrm.clamp_min(1e-8)[:, None], rtol=2e-5, atol=1e-7)
            assert all(bool(torch.isfinite(o).all()) for o in out)
        return (lambda: K.lp_compare_loss_fwd(hd, td, temperature)), verify
    return factory


case("lp_compare_loss_fwd", "two-rows-two-partners")(_lp_compare_loss(2, 2, 8))
case("lp_compare_loss_fwd", "hub-target-zero-row-500x101x256")(_lp_compare_loss(500, 101, 256))


def _edge_history(I=60):
    """User 0: every item but 7; user 1: one item; user 2: none (tests/test_gpu_edge_pretrain.py::_law_history)."""
    rng = np.random.default_rng(11)
    free = np.sort(rng.choice(I, 7, replace=False))
    rows = [np.setdiff1d(np.arange(I), free), np.array([23]), np.zeros(0, np.int64)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rowptr, np.concatenate(rows).astype(np.int64), rows, I


@case("edge_hist_check", "three-users")
def _edge_hist_check(dev):
    from ragraph_amd import kernels as K

    rowptr, items, rows, I = _edge_history()
    rp, it = T(rowptr, dev), T(items, dev)
    bad = T(np.array([5, 1], np.int64), dev)

    def run():
        K.edge_hist_check(rp, it, I)                      # a valid history passes ...
        return ()

    def verify(out):
        with pytest.raises(K.RagraphNativeError, match="ascending"):     # ... and an unsorted row is still refused
            K.edge_hist_check(torch.tensor([0, 2], device=dev), bad, 10)
    return run, verify


def _edge_neg_sample(users, n_negs):
    def factory(dev):
        from ragraph_amd import kernels as K

        rowptr, items, rows, I = _edge_history()
        args = (T(rowptr, dev), T(items, dev), I, T(np.asarray(users, np.int64), dev), n_negs,
                torch.tensor([12345], dtype=torch.int64, device=dev))

        def verify(out):     # (no bit oracle: the law's rules -- never a history item, in range, slot b * n_negs + j is users[b]'s)
            blocks = NP(out[0]).reshape(len(users), n_negs)
            assert ((blocks >= 0) & (blocks < I)).all()
            for b, u in enumerate(users):
                assert not np.isin(blocks[b], rows[u]).any()
            if len(users) >= 1000:
                assert set(np.unique(blocks[0::5])) == set(np.setdiff1d(np.arange(I), rows[0]))
        return (lambda: (K.edge_neg_sample(*args),)), verify
    return factory


case("edge_neg_sample", "one-user-one-negative")(_edge_neg_sample([1], 1))
case("edge_neg_sample", "2000-users-16-negatives")(_edge_neg_sample([0, 1, 2, 0, 1] * 400, 16))


# ---- the table's tests --------------------------------------------------------------------------------------------------------
IDS = [c[0] for c in CASES]
assert len(set(IDS)) == len(IDS)


def _build(cid, dev, monkeypatch):
    _, wrapper, env, factory = CASES[IDS.index(cid)]
    _set_env(monkeypatch, env)
    return factory(dev)


@pytest.mark.parametrize("cid", IDS)
def test_exact_guarded_workspace_gives_the_ordinary_bits(dev, monkeypatch, cid):
    run, verify = _build(cid, dev, monkeypatch)
    want = run()
    torch.cuda.synchronize()
    verify(want)
    for fill in GW.FILLS:
        got, gw = guarded(monkeypatch, run, fill)
        n = gw.check()                                    # (synchronises)
        assert n >= 1, f"{cid}: the path under test asked for no workspace"
        same_bits(got, want, f"{cid} [fill 0x{fill:02X}]")
        assert all(nbytes == 0 for _, nbytes, _ in gw.requests) == (cid in ZERO_QUERY)


@pytest.mark.parametrize("cid", [c[0] for c in CASES if c[0] not in ZERO_QUERY])
def test_a_workspace_one_byte_short_is_refused_before_any_launch(dev, monkeypatch, cid):
    from ragraph_amd import kernels as K

    run, _ = _build(cid, dev, monkeypatch)
    gw = GW.GuardedWorkspace(fill=0xA5, short=True)
    with monkeypatch.context() as m:
        m.setattr(K, "_workspace", gw)
        with pytest.raises(K.RagraphNativeError, match=r"\(code -3\)"):
            run()
    assert gw.check() >= 1 and any(nbytes > 0 for _, nbytes, _ in gw.requests)
    assert gw.interior_untouched(), f"{cid}: the refused call wrote into its workspace"


# ---- entries that allocate their own scratch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,C,D,mode", [(1, 1, 30, 0), (257, 5, 64, 2), (1000, 3, 256, 1), (512, 64, 128, 1)])
def test_proto_cosine_grad_proto_on_a_guarded_buffer(dev, G, C, D, mode):
    """kernels.proto_cosine_grad_proto sizes a torch.empty of its own: the entry through ctypes on a guarded buffer of exactly
    ragraph_proto_cosine_grad_proto_workspace_bytes, the three fills; against torch autograd in float64 (the bound of
    tests/test_gpu_backward.py); one byte short: RAGRAPH_EWORKSPACE, nothing written."""
    import torch.nn.functional as F

    from ragraph_amd import kernels as K

    L = K._ready()
    g = torch.Generator().manual_seed(G + C)
    emb, proto, go = torch.randn(G, D, generator=g), torch.randn(C, D, generator=g), torch.randn(G, C, generator=g)
    pr = proto.double().clone().requires_grad_(True)
    cos = F.cosine_similarity(emb.double()[:, None, :], pr[None, :, :], dim=-1, eps=1e-8)
    f = cos if mode == 0 else (F.softmax(cos, 1) if mode == 1 else F.log_softmax(cos, 1))
    (f * go.double()).sum().backward()
    ref = pr.grad.float()
    ed, pd, gd = emb.to(dev), proto.to(dev), go.to(dev)
    out = K.proto_cosine(ed, pd, mode)
    want = K.proto_cosine_grad_proto(ed, pd, mode, out, gd)
    assert torch.allclose(want.cpu(), ref, atol=1e-5 + 2e-4 * float(ref.abs().max())), (want.cpu() - ref).abs().max()
    nbytes = int(L.ragraph_proto_cosine_grad_proto_workspace_bytes(G, C, D))
    assert nbytes > 0

    def call(ws):
        gproto = torch.full_like(pd, float("nan"))
        rc = L.ragraph_proto_cosine_grad_proto_f32(ed.data_ptr(), G, D, pd.data_ptr(), C, mode, out.data_ptr(), gd.data_ptr(),
                                                   gproto.data_ptr(), ws.data_ptr(), ws.numel(), K._stream())
        return rc, gproto

    for fill in GW.FILLS:
        gw = GW.GuardedWorkspace(fill=fill)
        rc, got = call(gw(nbytes, dev))
        assert rc == 0 and gw.check() == 1
        assert torch.equal(_bits(got), _bits(want)), f"fill 0x{fill:02X}"
    gw = GW.GuardedWorkspace(fill=0xFF, short=True)
    rc, got = call(gw(nbytes, dev))
    assert rc == K.N.EWORKSPACE and "workspace" in K.N.last_error()
    assert gw.check() == 1 and gw.interior_untouched() and bool(torch.isnan(got).all())


# ---- the statistics view ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,D,k,shards", [(7, 70000, 256, 10, 0), (300, 40000, 256, 10, 0), (64, 100000, 128, 10, 0),
                                            (9, 70000, 256, 33, 0), (9, 70000, 256, 65, 0), (300, 40000, 256, 10, 2)])
def test_statistics_view_lies_inside_the_exact_workspace(dev, monkeypatch, B, N, D, k, shards):
    """topk_cosine_filtered(return_stats=True): the [32] int32 view is the workspace's last 16-byte aligned 128 bytes, inside the
    exact workspace, and decodes (filter_stats_levels) to the levels of the run on the ordinary workspace."""
    from ragraph_amd import kernels as K

    g = torch.Generator(device=dev).manual_seed(B + N)
    kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
    kb = K.keys_to_bf16(kn)
    q = torch.randn(B, D, device=dev, generator=g)
    kw = {}
    if shards:
        def exchange(phase, theta, scores):
            pass
        exchange.n_shards = shards
        kw = {"exchange": exchange}
    want = K.filter_stats_levels(K.topk_cosine_filtered(q, kn, kb, k, return_stats=True, **kw)[3].cpu().tolist())
    assert 1 <= len(want) <= 3 and all(keys > 0 for _, keys, _ in want)
    (s, i, over, st), gw = guarded(monkeypatch, lambda: K.topk_cosine_filtered(q, kn, kb, k, return_stats=True, **kw), 0xFF)
    assert gw.check() == 1
    buf, nbytes, _ = gw.requests[0]
    lo = st.data_ptr() - buf.data_ptr() - GW.G
    assert st.numel() == 32 and 0 <= lo and lo + 128 <= nbytes and nbytes - lo - 128 < 16 and lo % 16 == 0
    assert K.filter_stats_levels(st.cpu().tolist()) == want


# ---- end-to-end flows under the guarded allocator -----------------------------------------------------------------------------
def _flow(monkeypatch, run):
    """run() on the ordinary workspace, then under the guarded allocator (fill 0xFF): the same bits, clean guards."""
    want = run()
    torch.cuda.synchronize()
    got, gw = guarded(monkeypatch, run, 0xFF)
    n = gw.check()
    assert n >= 1
    same_bits(got, want, "flow")
    return want, n


def test_flow_node_forward_through_key_index(dev, monkeypatch):
    from ragraph_amd.data import DataLoader, synthetic_tu_dataset
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph import RAGraph
    from ragraph_amd.ragraph_utils import process_tu_dataset

    torch.manual_seed(0)
    F_in, C, D, N = 18, 3, 256, 5000
    ds = synthetic_tu_dataset(num_graphs=8, num_node_attributes=F_in, num_node_labels=C, seed=3)
    pre = PrePrompt(F_in, D, "prelu", 1, 0.3).to(dev)
    model = RAGraph(pre, None, F_in, C, D, finetune=True, device=dev).eval()
    g = torch.Generator().manual_seed(1)
    keys = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    vals = torch.randn(N, D, generator=g)
    labs = torch.nn.functional.one_hot(torch.randint(0, C, (N,), generator=g), C).float()
    model.toy_graph_base.add_resources(keys.to(dev), vals.to(dev), labs.to(dev))
    feats, adj, _ = process_tu_dataset(next(iter(DataLoader(ds, batch_size=8))), F_in, device=dev)

    def run():
        with torch.no_grad():
            logits = model(feats, adj)
            h = pre.inference(feats, adj)
            s, i = model.toy_graph_base.topk(h, model.toy_graph_base.retrieve_num)
        return logits, s, i, h

    (logits, s, i, h), _ = _flow(monkeypatch, run)
    assert bool(torch.isfinite(logits).all())
    # (the bank keeps normalize_rows(keys): the oracle's rows, bit for bit)
    rs, ri = _cref().topk_cosine(NP(h), _cref().normalize_rows(keys.numpy()), model.toy_graph_base.retrieve_num)
    assert np.array_equal(NP(i), ri) and np.array_equal(NP(s).view(np.int32), rs.view(np.int32))


def test_flow_edge_cal_loss_step_with_edge_dropout(dev, monkeypatch):
    from ragraph_amd.data import synthetic_bipartite
    from ragraph_amd.RAGraph_edge import RAGraph as RAGraphEdge

    U, I, D = 300, 200, 64
    edges, norm, times = synthetic_bipartite(U, I, edges_per_user=6, seed=12, device=dev)

    class DS:
        num_users, num_items = U, I
    DS.edges, DS.edge_norm, DS.edge_times = edges, norm, times

    class Pre:
        def generate(self):
            g = torch.Generator(device=dev).manual_seed(5)
            return 0.1 * torch.randn(U, D, device=dev, generator=g), 0.1 * torch.randn(I, D, device=dev, generator=g)

    names = ("user_embedding", "item_embedding", "gating_weight", "gating_bias")

    def run():
        torch.manual_seed(3)
        m = RAGraphEdge(DS, Pre(), phase="finetune", use_RAG=False, use_LoRA=False, retrieve_num=5, device=dev).train()
        m.edge_dropout, m.dropout_rng = 0.5, "device"
        batch = (torch.randint(0, U, (64,)), torch.randint(0, I, (64,)), torch.randint(0, I, (64,)))
        loss, _ = m.cal_loss(batch)
        loss.backward()
        return (loss.detach(),) + tuple(getattr(m, k).grad.clone() for k in names)

    out, _ = _flow(monkeypatch, run)
    assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in out)


def test_flow_bank_build_on_device_draws(dev, monkeypatch):
    from ragraph_amd.data import synthetic_tu_dataset
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.ragraph_utils import ToyGraphBase, seed_everything

    seed_everything(1)
    ds = synthetic_tu_dataset(num_graphs=20, num_node_attributes=18, num_node_labels=3, num_classes=2, seed=5)
    pre = PrePrompt(18, 256, "prelu", 1, 0.3).to(dev)

    def run():
        torch.manual_seed(3)
        tgb = ToyGraphBase(pre, 3, 256, 3, device=dev, flavour="node")
        tgb.build_rng = "device"
        tgb.build_toy_graph(ds)
        return tgb.last_build_seed, tgb.resource_keys, tgb.resource_values, tgb.resource_labels, tgb.resource_positions

    out, _ = _flow(monkeypatch, run)
    assert out[1].shape[1] == 256 and bool(torch.isfinite(out[2]).all())


def test_flow_metric_eval_g17(dev, monkeypatch):
    from ragraph_amd.edge_eval import Metric

    g = dict(np.load(os.path.join(GOLD, "g17_metric_eval.npz")))
    rows = lambda rp, it: [it[rp[u]:rp[u + 1]].tolist() for u in range(len(rp) - 1)]   # noqa: E731

    users = g["eval_users"].tolist()
    hist = rows(g["eval_hist_rowptr"], g["eval_hist_items"])
    gt = rows(g["eval_gt_rowptr"], g["eval_gt_items"])

    class Loader:
        pass
    Loader.test_user_dict = {u: gt[i] for i, u in enumerate(users)}
    Loader.user_hist_dict = {u: hist[i] for i, u in enumerate(users)}
    Loader.train_user_dict = {int(u): Loader.user_hist_dict.get(int(u), []) for u in g["train_users"]}

    class Model:
        def generate(self):
            return T(g["user_emb"], dev), T(g["item_emb"], dev)

    def run():
        m = Metric("recall;ndcg;precision", ";".join(str(k) for k in g["ks"]), int(g["eval_batch_size"]))
        res = m.eval(Model(), Loader)
        return (m.last_ranked,) + tuple(np.asarray(res[mm], dtype=np.float64) for mm in ("recall", "ndcg", "precision")) + \
            tuple(np.asarray(m.last_values[mm], dtype=np.float64) for mm in ("recall", "ndcg", "precision"))

    out, _ = _flow(monkeypatch, run)
    assert np.array_equal(NP(out[0]), g["eval_ranked"])
    for j, mm in enumerate(("recall", "ndcg", "precision")):
        assert np.array_equal(out[1 + j], g[f"eval_{mm}"]) and np.allclose(out[4 + j], g[f"eval_{mm}_raw"], rtol=0, atol=1e-9)
