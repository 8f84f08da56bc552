"""Mixed retrieval through the filter on the GPU: K.topk_mix_rerank (ragraph_topk_mix_rerank_f32) and the route
KeyIndex.topk_mix behind ToyGraphBase.topk.

Every comparison is bit-exact (scores and indices) against the CPU oracle (cref) or the exact K.topk_cosine_mix -- the path
every mixed call took before this route existed; nothing is compared with the new code itself.  The unproven counts the
route must report are the ones tests/test_cpu_topk_mix_filtered.py derives from the numpy restatement."""
import numpy as np
import pytest
import torch

import mix_rerank_reference as R
from oracle import cref

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _same(got, want):
    return torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))


# ---- 1: the kernel alone -------------------------------------------------------------------------------------------------
_KERNEL_BANKS = {}


def _kernel_bank(A):
    """B = 70 queries, N = 1000 keys with exact duplicate rows (keys AND codes: ties in the mixed score), all-zero code rows
    and one all-zero query code row; the semantic matrix from cref, once per A."""
    if A not in _KERNEL_BANKS:
        rng = np.random.default_rng(100 + A)
        B, N, D = 70, 1000, 64
        keys = rng.standard_normal((N, D), dtype=np.float32)
        codes = R.make_codes(rng, N, A)
        for b in range(0, 40):                           # every listed region holds copies: rows 5 b + 1 .. 5 b + 3 copy row 5 b
            keys[5 * b + 1:5 * b + 4] = keys[5 * b]
            codes[5 * b + 1:5 * b + 4] = codes[5 * b]
        codes[::7] = 0.0
        q = rng.standard_normal((B, D), dtype=np.float32)
        q[:40] = keys[0:200:5] + 0.3 * rng.standard_normal((40, D), dtype=np.float32)   # query b is near the copies of row 5 b
        pq = R.make_codes(rng, B, A, zero_rows=0.0)
        pq[3] = 0.0
        kn, pnn = cref.normalize_rows(keys), cref.normalize_rows(codes)
        sem = cref.linear(cref.normalize_rows(q), kn)
        _KERNEL_BANKS[A] = (pq, pnn, sem)
    return _KERNEL_BANKS[A]


@pytest.mark.parametrize("A", [1, 10, 16])
@pytest.mark.parametrize("kl", [32, 64, 128])
def test_kernel_equals_the_numpy_restatement(dev, kl, A):
    from ragraph_amd import kernels as K

    pq, pnn, sem = _kernel_bank(A)
    sem_s, sem_i = cref.topk_rows(sem, kl)
    ties = 0
    for k in (1, 10, kl // 2):
        for (ws, wm), base in (((0.05, 0.95), 0), ((0.3, 0.7), 1000), ((-0.01, 1.0), 0)):
            want_s, want_i, want_u = R.np_rerank(sem_s, sem_i + base, pq, pnn, ws, wm, k, idx_base=base)
            s, i, flags, count = K.topk_mix_rerank(T(sem_s, dev), T(sem_i + base, dev), T(pq, dev), T(pnn, dev), ws, wm, k,
                                                   idx_base=base)
            assert flags.dtype == torch.int32 and count.dtype == torch.int32
            assert np.array_equal(i.cpu().numpy(), want_i), (k, ws, "indices")
            assert np.array_equal(_bits(s), want_s.view(np.int32)), (k, ws, "scores")
            assert np.array_equal(flags.cpu().numpy(), want_u), (k, ws, "flags")
            assert int(count.item()) == int(want_u.sum())
            tied = want_s[:, 1:] == want_s[:, :-1]
            ties += int(tied.sum())
            assert (want_i[:, 1:][tied] > want_i[:, :-1][tied]).all()
    assert ties > 0                                       # the duplicate rows did show the index order
    # both verdicts occur on this bank
    u_small = R.np_rerank(sem_s, sem_i, pq, pnn, 0.001, 0.999, 1)[2]
    u_large = R.np_rerank(sem_s, sem_i, pq, pnn, 0.3, 0.7, kl // 2)[2]
    assert (u_small == 0).any() and (u_large == 1).any()


def test_kernel_flags_rows_with_indices_outside_the_bank_or_non_finite_scores(dev):
    from ragraph_amd import kernels as K

    pq, pnn, sem = _kernel_bank(10)
    sem_s, sem_i = cref.topk_rows(sem, 32)
    clean = R.np_rerank(sem_s, sem_i, pq, pnn, 0.001, 0.999, 5)[2]
    assert clean[0] == 0 and clean[1] == 0 and clean[2] == 0
    s2, i2 = sem_s.copy(), sem_i.copy()
    i2[0, 31] = np.iinfo(np.int64).max                    # a padding entry: never read
    i2[1, 4] = 1000                                       # one past the bank
    s2[2, 0] = np.nan
    _, _, flags, count = K.topk_mix_rerank(T(s2, dev), T(i2, dev), T(pq, dev), T(pnn, dev), 0.001, 0.999, 5)
    want = clean.copy()
    want[:3] = 1
    assert np.array_equal(flags.cpu().numpy(), want) and int(count.item()) == int(want.sum())


def test_row_scatter_writes_the_rows_it_is_given(dev):
    from ragraph_amd import kernels as K

    g = torch.Generator().manual_seed(3)
    s = torch.randn(70, 10, generator=g).to(dev)
    i = torch.randint(0, 1 << 40, (70, 10), generator=g).to(dev)
    pos = torch.tensor([69, 0, 17], device=dev)
    rs, ri = torch.randn(3, 10, generator=g).to(dev), torch.randint(0, 1 << 40, (3, 10), generator=g).to(dev)
    want_s, want_i = s.clone(), i.clone()
    want_s[pos], want_i[pos] = rs, ri
    K.scatter_topk_rows_(s, i, pos, rs, ri)
    assert torch.equal(s, want_s) and torch.equal(i, want_i)


# ---- 2: the route end to end ---------------------------------------------------------------------------------------------
def _tgb(dev, kn, codes, n=None):
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    n = kn.shape[0] if n is None else n
    tgb = ToyGraphBase(None, 3, kn.shape[1], 3, device=dev)
    tgb.set_resources(kn[:n], kn[:n], torch.zeros(n, 3, device=dev), codes[:n])
    return tgb


def _open_route(monkeypatch):
    """The measured rule may exclude a test's shape: the tests ask for the route itself (the switches stay as they are)."""
    from ragraph_amd import kernels as K

    monkeypatch.setattr(K, "mix_filter_measured", lambda *shape: True)
    monkeypatch.delenv("RAGRAPH_MIX_FILTER", raising=False)
    monkeypatch.delenv("RAGRAPH_EXACT_FP32", raising=False)


@pytest.fixture(scope="module")
def route0(dev):
    """The reference shape on the device: raw queries, raw bank keys, raw query codes, raw bank codes."""
    q, keys, pq, codes = R.make_raw(R.SEED0, R.B0, R.N0, R.D0, R.A0)
    return T(q, dev), T(keys, dev), T(pq, dev), T(codes, dev)


@pytest.mark.parametrize("ws,wm", R.WEIGHTS)
def test_route_at_k10_equals_the_exact_call_and_the_oracle(dev, monkeypatch, route0, ws, wm):
    from ragraph_amd import kernels as K

    _open_route(monkeypatch)
    q, kn, pq, codes = route0
    _, _, _, _, sem, struct = R.route_inputs()
    tgb = _tgb(dev, kn, codes)
    assert np.array_equal(_bits(tgb.keys_normalized), R.route_inputs()[1].view(np.int32))   # (the oracle's bank)
    assert np.array_equal(_bits(tgb.positions_normalized), R.route_inputs()[3].view(np.int32))
    tgb.structure_weight, tgb.semantic_weight = ws, wm
    got = tgb.topk(q, R.K0, pq)
    st = tgb._index.mix_stats
    assert st["filtered_calls"] == 1 and st["exact_calls"] == 0
    want = K.topk_cosine_mix(q, tgb.keys_normalized, pq, tgb.positions_normalized, ws, wm, R.K0)
    assert _same(got, want)
    os_, oi = R.oracle_mixed_topk(sem[:64], struct[:64], ws, wm, R.K0)
    assert np.array_equal(got[1][:64].cpu().numpy(), oi) and np.array_equal(_bits(got[0][:64]), os_.view(np.int32))
    assert st["rows_unproven"] == R.UNPROVEN0[(ws, wm)]
    assert st["demotions"] == (1 if R.UNPROVEN0[(ws, wm)] > tgb._index.MIX_FILTER_MAX_UNPROVEN * R.B0 else 0)


@pytest.mark.parametrize("B,N,k", [(512, 20000, 20), (256, 65536, 40)])
def test_route_through_the_wide_entries_equals_the_exact_call_and_the_oracle(dev, monkeypatch, B, N, k):
    """k = 20 -> lists of 40 keys at the smallest shape filter_wide_helps accepts; k = 40 -> lists of 80 keys at the smallest
    filter_wide128_helps accepts."""
    from ragraph_amd import kernels as K
    from ragraph_amd.kernels_index import WIDE, WIDE128

    _open_route(monkeypatch)
    D, A = 128, 10
    kl = K.mix_filter_list(k)
    assert (K.filter_wide_helps if kl <= 64 else K.filter_wide128_helps)(B, N, D, kl)
    q, keys, pq, codes = R.make_raw(N + k, B, N, D, A)
    kn, pnn = cref.normalize_rows(keys), cref.normalize_rows(codes)
    qd, pqd = T(q, dev), T(pq, dev)
    tgb = _tgb(dev, T(keys, dev), T(codes, dev))
    knd, pnd = tgb.keys_normalized, tgb.positions_normalized
    assert np.array_equal(_bits(knd), kn.view(np.int32)) and np.array_equal(_bits(pnd), pnn.view(np.int32))   # (the oracle's bank)
    sem64 = cref.linear(cref.normalize_rows(q[:64]), kn)
    struct64 = cref.linear(cref.normalize_rows(pq[:64]), pnn)
    for ws, wm in R.WEIGHTS:
        tgb.structure_weight, tgb.semantic_weight = ws, wm
        before = dict(tgb._index.mix_stats) if tgb._index is not None else {"filtered_calls": 0, "rows_unproven": 0}
        got = tgb.topk(qd, k, pqd)
        st = tgb._index.mix_stats
        assert st["filtered_calls"] == before["filtered_calls"] + 1 and st["exact_calls"] == 0, (ws, wm)
        assert tgb._index._route(B, N, D, kl) == (WIDE if kl <= 64 else WIDE128)
        want = K.topk_cosine_mix(qd, knd, pqd, pnd, ws, wm, k)
        assert _same(got, want), (ws, wm)
        os_, oi = R.oracle_mixed_topk(sem64, struct64, ws, wm, k)
        assert np.array_equal(got[1][:64].cpu().numpy(), oi) and np.array_equal(_bits(got[0][:64]), os_.view(np.int32))
        print(f"{B} x {N} x {D}, k = {k}, weights ({ws}, {wm}): {st['rows_unproven'] - before['rows_unproven']} rows unproven")


def test_demotion_at_a_dominant_structural_weight(dev, monkeypatch, route0):
    from ragraph_amd import kernels as K

    _open_route(monkeypatch)
    q, kn, pq, codes = route0
    tgb = _tgb(dev, kn, codes)
    tgb.structure_weight, tgb.semantic_weight = 0.3, 0.7
    want = K.topk_cosine_mix(q, tgb.keys_normalized, pq, tgb.positions_normalized, 0.3, 0.7, R.K0)
    first = tgb.topk(q, R.K0, pq)
    st = tgb._index.mix_stats
    assert _same(first, want) and st == {"filtered_calls": 1, "exact_calls": 0, "rows_unproven": R.B0, "demotions": 1}
    second = tgb.topk(q, R.K0, pq)
    assert _same(second, want) and st == {"filtered_calls": 1, "exact_calls": 1, "rows_unproven": R.B0, "demotions": 1}
    tgb.set_resources(kn, kn, torch.zeros(R.N0, 3, device=dev), codes)      # the rows are set anew: judged again
    third = tgb.topk(q, R.K0, pq)
    assert _same(third, want) and tgb._index.mix_stats["filtered_calls"] == 1 and tgb._index.mix_stats["demotions"] == 1


def test_bank_with_a_tail_and_retired_rows(dev, monkeypatch):
    """add_resources of 40 rows behind a live index, then remove_resources of 5 -- a semantic winner among them: the bits of a
    fresh bank over the surviving rows, mapped to the physical rows."""
    from ragraph_amd import kernels as K

    _open_route(monkeypatch)
    B, N, D, A, k = 512, 20000, 128, 10, 10
    q, keys, pq, codes = R.make_raw(77, B, N + 40, D, A)
    qd, knd, pqd, pnd = T(q, dev), T(keys, dev), T(pq, dev), T(codes, dev)      # (raw rows: the bank normalises them)
    tgb = _tgb(dev, knd, pnd, n=N)
    tgb.structure_weight, tgb.semantic_weight = 0.02, 0.98
    tgb.topk(qd, k, pqd)                                   # the index and the caches exist: the next rows are a tail
    tgb.add_resources(knd[N:], knd[N:], torch.zeros(40, 3, device=dev), pnd[N:])
    assert tgb._index.tail_rows == 40
    _, sem_i = tgb._index.topk(qd, 1)
    retired = sorted({int(sem_i[0, 0]), int(sem_i[1, 0]), 5, N + 3, N + 39})
    assert len(retired) == 5
    tgb.remove_resources(retired)
    assert tgb.retired_rows == 5 and tgb._index.tail_rows == 40
    calls = tgb._index.mix_stats["filtered_calls"]
    got = tgb.topk(qd, k, pqd)
    assert tgb._index.mix_stats["filtered_calls"] == calls + 1 and tgb.retired_rows == 5 and tgb._index.tail_rows == 40
    live = np.setdiff1d(np.arange(N + 40), retired)
    lived = T(live, dev)
    assert tgb.keys_normalized.shape[0] == N + 40 and tgb.positions_normalized.shape[0] == N + 40
    ws_, wi = K.topk_cosine_mix(qd, K.gather_rows(tgb.keys_normalized, lived), pqd, K.gather_rows(tgb.positions_normalized, lived),
                                0.02, 0.98, k)
    assert torch.equal(got[1], lived[wi]) and torch.equal(got[0].view(torch.int32), ws_.view(torch.int32))
    assert not torch.isin(got[1], T(np.array(retired), dev)).any()


def test_under_a_capture_the_call_is_the_exact_one(dev, monkeypatch, route0):
    from ragraph_amd import kernels as K

    _open_route(monkeypatch)
    q, kn, pq, codes = route0
    tgb = _tgb(dev, kn, codes)
    tgb.structure_weight, tgb.semantic_weight = 0.02, 0.98
    eager = tgb.topk(q, R.K0, pq)                          # (warm-up too: workspace, caches, the index)
    assert tgb._index.mix_stats["filtered_calls"] == 1
    K.topk_cosine_mix(q, tgb.keys_normalized, pq, tgb.positions_normalized, 0.02, 0.98, R.K0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.topk_cosine_mix(q, tgb.keys_normalized, pq, tgb.positions_normalized, 0.02, 0.98, R.K0)
        torch.cuda.synchronize()
        sq, spq = torch.zeros_like(q), torch.zeros_like(pq)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            gs, gi = tgb.topk(sq, R.K0, spq)
        sq.copy_(q)
        spq.copy_(pq)
        graph.replay()
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    st = tgb._index.mix_stats
    assert st["filtered_calls"] == 1 and st["exact_calls"] == 1
    assert _same((gs, gi), eager)


def test_switch_gives_the_exact_path_and_the_same_bits(dev, monkeypatch, route0):
    from ragraph_amd import kernels as K

    _open_route(monkeypatch)
    q, kn, pq, codes = route0
    tgb = _tgb(dev, kn, codes)
    tgb.structure_weight, tgb.semantic_weight = 0.05, 0.95
    routed = tgb.topk(q, R.K0, pq)
    monkeypatch.setenv("RAGRAPH_MIX_FILTER", "0")
    plain = tgb.topk(q, R.K0, pq)
    st = tgb._index.mix_stats
    assert st["filtered_calls"] == 1 and st["exact_calls"] == 1 and _same(routed, plain)
    assert _same(plain, K.topk_cosine_mix(q, tgb.keys_normalized, pq, tgb.positions_normalized, 0.05, 0.95, R.K0))
