"""Bank construction with the draws made on the device (csrc/bank.hip, build_rng = "device"): every kernel against the numpy
restatement of its rule (tests/bank_rng_oracle.py) or against the torch chain it replaces, bit for bit, at the smallest shapes
that reach each edge; the laws of the two samplers with derived bounds; the node, graph and edge flavours end to end with the
host draws made to raise; and "host" mode with the new wrappers made to raise."""
import math

import numpy as np
import pytest
import torch

import bank_rng_oracle as B

pytestmark = pytest.mark.gpu

SEED = 0x0BAD_5EED_1234_567
SEED2 = 0x1357_9BDF_0246_8AC


def _seed(dev, value=SEED):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- edge rewrite ------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 200]   # below, at and above the 64 lanes of a wave; more than one trip of the slot loop


def _graph_batch(dev, sizes, seed=3):
    """Random symmetric 0/1 graphs as one block-diagonal CSR, and their node offsets."""
    from ragraph_amd.graph import CSRGraph

    rng = np.random.default_rng(seed)
    n = sum(sizes)
    a = np.zeros((n, n), np.float32)
    off = 0
    for s in sizes:
        b = (rng.random((s, s)) < 0.1).astype(np.float32)
        b = np.maximum(b, b.T)
        idx = np.arange(s - 1)
        b[idx, idx + 1] = b[idx + 1, idx] = 1          # a path: no isolated node in a graph of two or more
        if s == 1:
            b[0, 0] = 0                                # (the graph of one node has no edge at all)
        a[off:off + s, off:off + s] = b
        off += s
    return CSRGraph.from_dense(T(a, dev)), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _check_rewrite(dev, prob, gp, seed=SEED):
    from ragraph_amd import kernels as K

    rowptr, col, val = K.edge_rewrite_csr(prob, T(gp, dev), _seed(dev, seed))
    want_rowptr, want_col = B.edge_rewrite(seed, prob.cpu().numpy(), gp)
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
    assert np.array_equal(rowptr.cpu().numpy(), want_rowptr)
    assert np.array_equal(col.cpu().numpy(), want_col)
    assert val.numel() == col.numel() and bool((val == 1.0).all())
    return rowptr, col


def test_edge_rewrite_matches_oracle_on_sample_probabilities(dev):
    from ragraph_amd.bank_build import compute_sample_prob

    g, gp = _graph_batch(dev, SIZES)
    prob = compute_sample_prob(g, T(gp, dev))
    rowptr, col = _check_rewrite(dev, prob, gp)
    assert 0 < col.numel() < sum(s * s for s in SIZES)
    other, _ = _check_rewrite(dev, prob, gp, SEED2)    # another seed, another pattern
    assert not torch.equal(other, rowptr)


def test_edge_rewrite_all_ones_keeps_every_slot_and_all_zeros_none(dev):
    gp = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(gp[-1])
    rowptr, col = _check_rewrite(dev, torch.ones(n, device=dev), gp)
    assert col.numel() == sum(s * s for s in SIZES)
    rp, c = rowptr.cpu().numpy(), col.cpu().numpy()
    for lo, hi in zip(gp[:-1], gp[1:]):                # full rows, across the 64-lane boundary
        for i in (lo, hi - 1):
            assert np.array_equal(c[rp[i]:rp[i + 1]], np.arange(lo, hi))
    rowptr, col = _check_rewrite(dev, torch.zeros(n, device=dev), gp)
    assert col.numel() == 0 and bool((rowptr == 0).all())


def test_edge_rewrite_one_graph_of_8192_nodes_needs_no_pair_list(dev):
    from ragraph_amd import kernels as K

    n = 8192
    rng = np.random.default_rng(11)
    p = rng.random(n).astype(np.float32) ** 4
    p = (p / p.sum()).astype(np.float32)               # sums to 1 like a sample probability: about n slots kept
    prob, gp = T(p, dev), np.array([0, n], np.int64)
    gpt, sd = T(gp, dev), _seed(dev)
    K.edge_rewrite_csr(prob, gpt, sd)                  # (the scratch buffer of the stream exists from here on)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    rowptr, col, val = K.edge_rewrite_csr(prob, gpt, sd)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"edge rewrite, one graph of {n}: {col.numel()} slots kept, peak {peak} bytes")
    assert peak < 64 << 20                             # the list of its ordered pairs alone: n^2 * 2 * 8 bytes = 1 GiB
    want_rowptr, want_col = B.edge_rewrite(SEED, p, gp)
    assert np.array_equal(rowptr.cpu().numpy(), want_rowptr) and np.array_equal(col.cpu().numpy(), want_col)
    assert n // 2 < col.numel() < 2 * n and bool((val == 1.0).all())


def test_edge_rewrite_reports_a_kept_total_of_2_to_31_instead_of_wrapping(dev):
    from ragraph_amd import kernels as K

    n = 46341                                          # n^2 = 2 147 488 281 >= 2^31 > 46340^2
    assert n * n >= 2 ** 31 > (n - 1) ** 2
    with pytest.raises(K.RagraphNativeError, match="2\\^31"):
        K.edge_rewrite_csr(torch.ones(n, device=dev), T(np.array([0, n], np.int64), dev), _seed(dev))


# ---- multinomial ---------------------------------------------------------------------------------------------------------------
def _segments(rng, sizes):
    """Random probabilities per segment (normalised), with zeros planted inside: single entries, a run across a tile
    boundary, the first and the last entry of the long segments."""
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
    return np.concatenate(ps), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.mark.parametrize("S", [1, 10, 257])
def test_multinomial_segments_match_oracle(dev, S):
    from ragraph_amd import kernels as K

    p, sp = _segments(np.random.default_rng(5), [1, 2, 64, 65, 1000, 5000])
    got = K.multinomial_segments(T(p, dev), T(sp, dev), S, _seed(dev)).cpu().numpy()
    want = B.multinomial_segments(SEED, p, sp, S)
    assert got.shape == (6, S) and got.dtype == np.int64 and np.array_equal(got, want)
    for g in range(6):                                 # inside its segment, never a zero-weight entry
        assert ((got[g] >= sp[g]) & (got[g] < sp[g + 1])).all() and (p[got[g]] > 0).all()


def test_multinomial_one_long_segment_zero_segment_and_clamp(dev):
    from ragraph_amd import kernels as K

    rng = np.random.default_rng(6)
    n, S = 300_000, 3000
    p = rng.random(n).astype(np.float32) ** 8
    p[rng.integers(0, n, n // 10)] = 0
    p = (p / p.sum()).astype(np.float32)
    whole = np.array([0, n], np.int64)
    got = K.multinomial_segments(T(p, dev), T(whole, dev), S, _seed(dev)).cpu().numpy()
    assert np.array_equal(got, B.multinomial_segments(SEED, p, whole, S)) and (p[got[0]] > 0).all()
    assert len(np.unique(got[0])) > S // 2
    # an all-zero segment (zeros, negatives, NaN) between two live ones gives -1; an empty one as well
    q = np.array([0.5, 0.5, 0, -1, np.nan, -0.0, 0.25, 0.75], np.float32)
    sq = np.array([0, 2, 6, 6, 8], np.int64)
    got = K.multinomial_segments(T(q, dev), T(sq, dev), 7, _seed(dev)).cpu().numpy()
    assert np.array_equal(got, B.multinomial_segments(SEED, q, sq, 7))
    assert (got[1] == -1).all() and (got[2] == -1).all() and (got[0] >= 0).all() and (got[3] >= 6).all()
    # p = 2 counts as 1: the same picks as the clamped row, and not those of a row that really weighs 2
    r2, r1 = np.array([2, 1, 1, 0.5], np.float32), np.array([1, 1, 1, 0.5], np.float32)
    s4 = np.array([0, 4], np.int64)
    g2 = K.multinomial_segments(T(r2, dev), T(s4, dev), 257, _seed(dev)).cpu().numpy()
    g1 = K.multinomial_segments(T(r1, dev), T(s4, dev), 257, _seed(dev)).cpu().numpy()
    assert np.array_equal(g2, g1) and np.array_equal(g2, B.multinomial_segments(SEED, r2, s4, 257))


# ---- induced blocks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 10, 64])
def test_csr_induced_blocks_match_dense_blocks(dev, S):
    from ragraph_amd import kernels as K
    from ragraph_amd.bank_build import _dense_blocks
    from ragraph_amd.graph import CSRGraph

    rng = np.random.default_rng(7 + S)
    n, G = 90, 9
    a = (rng.random((n, n)) < 0.15).astype(np.float32) * rng.random((n, n)).astype(np.float32)
    a[[0, 17, 89]] = 0                                 # rows without an entry, the first and the last among them
    a[5] = rng.random(n).astype(np.float32) + 0.5      # a full row
    g = CSRGraph.from_dense(T(a, dev))
    pick = rng.integers(0, n, (G, S))
    pick[0, :] = 17                                    # an empty row, picked S times
    if S > 1:
        pick[1, 1] = pick[1, 0]                        # a repeat
        pick[2, :2] = [0, 89]
        pick[3, :2] = [5, 5]
    pick = T(pick.astype(np.int64), dev)
    got = K.csr_induced_blocks(g.rowptr, g.col, g.val, pick)
    want = _dense_blocks(g, None, pick)
    assert got.shape == (G, S, S) and torch.equal(bits(got), bits(want))
    assert torch.equal(got.cpu(), T(a, "cpu")[pick.cpu().unsqueeze(2), pick.cpu().unsqueeze(1)])
    assert bool((got[0] == 0).all()) and (S == 1 or bool((got != 0).any()))


# ---- blocks to CSR ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,S", [(3, 1), (60, 64), (70, 64), (409, 10), (411, 10)])
def test_blocks_to_csr_matches_the_torch_chain(dev, G, S):
    from ragraph_amd import kernels as K
    from ragraph_amd.bank_build import _blocks_to_csr

    assert (G * S <= 4096) == ((G, S) in ((3, 1), (60, 64), (409, 10)))   # both sides of the host path's threshold
    rng = np.random.default_rng(G * 100 + S)
    b = (rng.random((G, S, S)) < 0.2).astype(np.float32) * (rng.random((G, S, S)).astype(np.float32) - 0.5)
    b[0] = 0                                           # an all-zero block
    b[1] = rng.random((S, S)).astype(np.float32) + 1   # a full block
    b[2, 0, 0] = -0.0                                  # not an entry
    blocks = T(b, dev)
    rowptr, col, val = K.blocks_to_csr(blocks)
    want = _blocks_to_csr(blocks)
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32
    assert torch.equal(rowptr, want.rowptr) and torch.equal(col, want.col) and torch.equal(bits(val), bits(want.val))
    assert int(rowptr[S]) == 0 and int(rowptr[2 * S] - rowptr[S]) == S * S


# ---- augment features ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("F", [3, 18, 64])
def test_augment_features_match_oracle_and_add_normal_noise(dev, F, with_ids):
    from ragraph_amd import kernels as K

    n = 301
    rng = np.random.default_rng(F)
    x = T(rng.standard_normal((n, F)).astype(np.float32), dev)
    p = rng.random(n).astype(np.float32)
    ids = (rng.integers(0, 50, n) + (np.arange(n) % 3 == 0) * (1 << 33)).astype(np.int64) if with_ids else np.arange(7, 7 + n)
    kw = dict(row_ids=T(ids, dev)) if with_ids else dict(row_base=7)
    prob = T(p, dev)
    got = K.augment_features(x, prob, _seed(dev), _seed(dev, SEED2), rate=0.5, std=0.1, **kw)
    keep = B.rows_kept(SEED, ids, p, 0.5)
    assert 0 < keep.sum() < n
    noisy = K.add_normal_noise(x, 0.1, _seed(dev, SEED2), **kw)
    want = torch.where(T(keep, dev).unsqueeze(1), noisy, torch.zeros((), device=dev))
    assert torch.equal(bits(got), bits(want))
    # rate 1 with p = 1: every row kept -- the bits of add_normal_noise; rate 0: every row +0, the sign bit clear
    ones = torch.ones(n, device=dev)
    assert torch.equal(bits(K.augment_features(x, ones, _seed(dev), _seed(dev, SEED2), rate=1.0, std=0.1, **kw)), bits(noisy))
    zero = K.augment_features(x, ones, _seed(dev), _seed(dev, SEED2), rate=0.0, std=0.1, **kw)
    assert bool((bits(zero) == 0).all())
    if with_ids:                                       # keyed by the id: rows that share one share their fate and their noise
        first = {}
        for r, i in enumerate(ids.tolist()):
            first.setdefault(i, r)
        src = torch.tensor([first[i] for i in ids.tolist()], device=dev)
        z = K.augment_features(torch.zeros_like(x), prob[src], _seed(dev), _seed(dev, SEED2), rate=0.5, std=0.1, **kw)
        assert torch.equal(bits(z), bits(z[src]))


# ---- bad arguments -----------------------------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_and_write_nothing(dev):
    from ragraph_amd import _native as N
    from ragraph_amd import kernels as K

    L = K._ready()
    s = _seed(dev).data_ptr()
    f = torch.full((64,), -7.0, device=dev)
    i64 = torch.full((64,), -7, dtype=torch.int64, device=dev)
    i32 = torch.full((64,), -7, dtype=torch.int32, device=dev)
    prob = torch.full((8,), 0.5, device=dev)
    gp = torch.tensor([0, 8], dtype=torch.int64, device=dev)
    ws = torch.full((1 << 16,), 0x55, dtype=torch.uint8, device=dev)
    pp, gpp, wp, wn = prob.data_ptr(), gp.data_ptr(), ws.data_ptr(), ws.numel()

    er = lambda sd, G, n, col, val, cap: L.ragraph_edge_rewrite_csr(sd, pp, gpp, G, n, i64.data_ptr(), i64.data_ptr() + 256, col, val,
                                                                     cap, wp, wn, None)
    for args in ((None, 1, 8, None, None, 0), (s, 0, 8, None, None, 0), (s, 1, 0, None, None, 0), (s, 1, 2 ** 31, None, None, 0),
                 (s, 1, 8, i32.data_ptr(), None, 8), (s, 1, 8, None, f.data_ptr(), 8), (s, 1, 8, i32.data_ptr(), f.data_ptr(), 0)):
        assert er(*args) == N.EINVAL and N.last_error().startswith("edge_rewrite")
    mn = lambda sd, n, G, S: L.ragraph_multinomial_segments_i64(sd, pp, n, gpp, G, S, i64.data_ptr(), wp, wn, None)
    for args in ((None, 8, 1, 4), (s, 8, 1, 0), (s, 8, 0, 4), (s, 0, 1, 4), (s, 1 << 23, 1, 4)):
        assert mn(*args) == N.EINVAL and N.last_error().startswith("multinomial_segments")
    ib = lambda pick, G, S, n: L.ragraph_csr_induced_blocks_f32(gpp, i32.data_ptr(), f.data_ptr(), n, 8, pick, G, S, f.data_ptr(), None)
    for args in ((None, 1, 4, 1), (i64.data_ptr(), 1, 0, 1), (i64.data_ptr(), 0, 4, 1), (i64.data_ptr(), 1, 4, 0)):
        assert ib(*args) == N.EINVAL and N.last_error().startswith("csr_induced_blocks")
    bc = lambda blocks, G, S: L.ragraph_blocks_to_csr_f32(blocks, G, S, i64.data_ptr(), i32.data_ptr(), f.data_ptr(),
                                                          i64.data_ptr() + 256, wp, wn, None)
    for args in ((None, 1, 4), (prob.data_ptr(), 1, 65), (prob.data_ptr(), 1, 0), (prob.data_ptr(), 0, 4)):
        assert bc(*args) == N.EINVAL and N.last_error().startswith("blocks_to_csr")
    af = lambda sd, sn, n, D, x: L.ragraph_augment_features_f32(x, n, D, pp, 0.5, 0.1, sd, sn, None, 0, f.data_ptr(), None)
    for args in ((None, s, 8, 4, pp), (s, None, 8, 4, pp), (s, s, 8, 0, pp), (s, s, -1, 4, pp), (s, s, 8, 4, None)):
        assert af(*args) == N.EINVAL and N.last_error().startswith("augment_features")
    torch.cuda.synchronize()
    assert bool((f == -7.0).all()) and bool((i64 == -7).all()) and bool((i32 == -7).all()) and bool((ws == 0x55).all())
    with pytest.raises(K.RagraphNativeError):
        K.blocks_to_csr(torch.zeros(2, 65, 65, device=dev))
    with pytest.raises(K.RagraphNativeError):
        K.multinomial_segments(prob, gp, 0, _seed(dev))


# ---- the laws --------------------------------------------------------------------------------------------------------------------
LAW_DRAWS, LAW_NODES = 200_000, 50
LAW_GRAPHS, LAW_GRAPH_NODES = 2000, 30


def law_multinomial_input():
    p = np.random.default_rng(21).random(LAW_NODES).astype(np.float32) ** 2
    return (p / p.sum()).astype(np.float32), np.array([0, LAW_NODES], np.int64)


def law_multinomial_check(picks):
    """Every count within 6 sqrt(N q (1 - q)) + 1 of N q, q the entry's share of the integer weights: a count is binomial
    (N, q); six standard deviations over 50 entries fail a correct sampler with probability below 50 * 2e-9."""
    p, _ = law_multinomial_input()
    w = B.weights(p).astype(np.float64)
    q = w / w.sum()
    counts = np.bincount(picks.reshape(-1), minlength=LAW_NODES)
    assert counts.sum() == LAW_DRAWS and len(counts) == LAW_NODES
    worst = np.max(np.abs(counts - LAW_DRAWS * q) / (6 * np.sqrt(LAW_DRAWS * q * (1 - q)) + 1))
    print(f"multinomial law: worst deviation / bound = {worst:.3f}")
    assert worst <= 1.0


def law_edge_input():
    rng = np.random.default_rng(22)
    p = rng.random((LAW_GRAPHS, LAW_GRAPH_NODES)).astype(np.float32)
    p = (p / p.sum(1, keepdims=True)).astype(np.float32).reshape(-1)
    return p, np.arange(0, LAW_GRAPHS * LAW_GRAPH_NODES + 1, LAW_GRAPH_NODES, dtype=np.int64)


def law_edge_check(kept_total):
    """The kept total is a sum of independent Bernoulli(t) over the 2000 * 30 * 30 slots: within 6 sqrt(sum t (1 - t)) of
    sum t."""
    p, gp = law_edge_input()
    mean, var = B.edge_thresholds_total(p, gp)
    print(f"edge rewrite law: kept {kept_total}, expected {mean:.1f}, 6 sd = {6 * math.sqrt(var):.1f}")
    assert abs(kept_total - mean) <= 6 * math.sqrt(var)


def test_multinomial_law(dev):
    from ragraph_amd import kernels as K

    p, sp = law_multinomial_input()
    law_multinomial_check(K.multinomial_segments(T(p, dev), T(sp, dev), LAW_DRAWS, _seed(dev)).cpu().numpy())


def test_edge_rewrite_law(dev):
    from ragraph_amd import kernels as K

    p, gp = law_edge_input()
    rowptr, col, _ = K.edge_rewrite_csr(T(p, dev), T(gp, dev), _seed(dev))
    assert int(rowptr[-1]) == col.numel()
    law_edge_check(col.numel())


# ---- end to end --------------------------------------------------------------------------------------------------------------------
WRAPPERS = ("edge_rewrite_csr", "multinomial_segments", "csr_induced_blocks", "blocks_to_csr", "augment_features")


@pytest.fixture
def no_host_draws(monkeypatch):
    """torch.multinomial, bernoulli, rand, randn_like and a randint on the host generator raise."""
    def deny(name):
        def f(*a, **k):
            raise AssertionError(f"torch.{name} called although build_rng = 'device'")
        return f
    for name in ("multinomial", "bernoulli", "rand", "randn_like"):
        monkeypatch.setattr(torch, name, deny(name))
    real = torch.randint

    def randint(*a, **k):
        if k.get("device") is None or torch.device(k["device"]).type == "cpu":
            raise AssertionError("torch.randint on the host generator although build_rng = 'device'")
        return real(*a, **k)
    monkeypatch.setattr(torch, "randint", randint)


@pytest.fixture
def no_new_kernels(monkeypatch):
    """The five new wrappers raise."""
    from ragraph_amd import kernels as K

    def deny(name):
        def f(*a, **k):
            raise AssertionError(f"K.{name} called")
        return f
    for name in WRAPPERS:
        monkeypatch.setattr(K, name, deny(name))


@pytest.fixture(scope="module")
def tu(dev):
    from ragraph_amd.data import DataLoader, synthetic_tu_dataset
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.ragraph_utils import process_tu_dataset, seed_everything

    seed_everything(1)
    ds = synthetic_tu_dataset(num_graphs=20, num_node_attributes=18, num_node_labels=3, num_classes=2, seed=5)
    pre = PrePrompt(18, 256, "prelu", 1, 0.3).to(dev)
    batch = next(iter(DataLoader(ds, batch_size=20)))
    feats, adj, labels = process_tu_dataset(batch, 18, device=dev)
    return ds, pre, batch, feats, adj, labels


def _node_bank(tu, dev, seed, build_rng="device"):
    from ragraph_amd.ragraph_utils import ToyGraphBase

    ds, pre = tu[0], tu[1]
    torch.manual_seed(seed)
    tgb = ToyGraphBase(pre, 3, 256, 3, device=dev, flavour="node")
    tgb.build_rng = build_rng
    tgb.build_toy_graph(ds)
    return tgb


def test_node_flavour_builds_on_the_device_draws_alone(dev, tu, no_host_draws):
    from ragraph_amd import kernels as K
    from ragraph_amd.bank_build import DIS_Q, NUM_ANCHORS, compute_sample_prob
    from ragraph_amd.graph import CSRGraph
    from ragraph_amd.ragraph_utils.Propagation import Propagation

    ds, pre, batch, feats, adj, node_labels = tu
    tgb = _node_bank(tu, dev, 3)
    G, S, V = 20, tgb.num_inverse_sample, 1 + tgb.num_augment_scale
    assert tgb.resource_keys.shape == (G * S * V, 256) and tgb.resource_positions.shape == (G * S * V, 10)
    assert tgb.resource_labels.shape == (G * S * V, 3) and bool(torch.isfinite(tgb.resource_values).all())
    seeds = tgb.last_build_seed
    assert seeds.shape == (V, K.BUILD_SEED_COLUMNS) and seeds.dtype == torch.int64 and seeds.is_cuda
    host_seeds = seeds.cpu().numpy()
    assert len(np.unique(host_seeds)) == host_seeds.size
    # the unfused composition, replayed from the seed tensor: the oracle's keep mask over add_normal_noise, then the kernels
    ptr = batch.ptr.to(dev, torch.int64)
    gp = batch.ptr.numpy().astype(np.int64)
    col = lambda v, c: seeds[v, c:c + 1]
    prob0 = compute_sample_prob(adj, ptr)
    keys, values, labels, positions = [], [], [], []
    for v in range(V):
        f, a = feats, adj
        if v > 0:
            keep = B.rows_kept(int(host_seeds[v, K.BUILD_SEED_NODE_DROP]), np.arange(feats.shape[0]), prob0.cpu().numpy(), 0.01)
            noisy = K.add_normal_noise(feats, 0.1, col(v, K.BUILD_SEED_FEATURE_NOISE))
            f = torch.where(T(keep, dev).unsqueeze(1), noisy, torch.zeros((), device=dev))
            rowptr, cols = B.edge_rewrite(int(host_seeds[v, K.BUILD_SEED_EDGE_SLOT]), prob0.cpu().numpy(), gp)
            a = CSRGraph(T(rowptr, dev), T(cols, dev), torch.ones(cols.size, device=dev), feats.shape[0])
        emb = pre.inference(f, a)
        prob = compute_sample_prob(a, ptr)
        pick = T(B.multinomial_segments(int(host_seeds[v, K.BUILD_SEED_PICK]), prob.cpu().numpy(), gp, S), dev)
        blocks = K.csr_induced_blocks(adj.rowptr, adj.col, adj.val, pick)
        k = K.normalize_rows(K.gather_rows(emb, pick.reshape(-1)))
        keys.append(k)
        values.append(Propagation.aggregate_k_hop_features(CSRGraph(*K.blocks_to_csr(blocks), G * S), k, tgb.toy_graph_hop))
        labels.append(K.gather_rows(node_labels, pick.reshape(-1)))
        anchors = K.noise_rows(col(v, K.BUILD_SEED_ANCHOR), G, NUM_ANCHORS, S)
        positions.append(K.position_codes_batch(blocks, anchors, DIS_Q).reshape(G * S, NUM_ANCHORS))
        if v == 0:                                     # each key is the normalised embedding of a node of ITS graph
            full = K.normalize_rows(emb)
            own = (pick >= ptr[:-1].unsqueeze(1)) & (pick < ptr[1:].unsqueeze(1))
            assert bool(own.all()) and torch.equal(k, full[pick.reshape(-1)])
    assert torch.equal(bits(tgb.resource_keys), bits(torch.cat(keys)))
    assert torch.equal(bits(tgb.resource_values), bits(torch.cat(values)))
    assert torch.equal(tgb.resource_labels, torch.cat(labels))
    assert torch.equal(bits(tgb.resource_positions), bits(torch.cat(positions)))
    lab0 = tgb.resource_labels[:G * S]
    assert bool(((lab0 == 0) | (lab0 == 1)).all()) and bool((lab0.sum(1) == 1).all())
    pos = tgb.resource_positions
    assert bool(((pos >= 0) & (pos <= 1)).all()) and bool((pos[:G * S] > 0).any())
    # torch.manual_seed reproduces the bank; another seed gives another
    again, other = _node_bank(tu, dev, 3), _node_bank(tu, dev, 4)
    assert torch.equal(again.last_build_seed, seeds) and torch.equal(bits(again.resource_keys), bits(tgb.resource_keys))
    assert torch.equal(bits(again.resource_values), bits(tgb.resource_values))
    assert torch.equal(bits(again.resource_positions), bits(tgb.resource_positions))
    assert not torch.equal(other.last_build_seed, seeds) and not torch.equal(other.resource_keys, tgb.resource_keys)


def test_graph_flavours_build_without_a_new_kernel(dev, tu, no_host_draws, no_new_kernels):
    from ragraph_amd.ragraph_utils import ToyGraphBase

    ds, pre = tu[0], tu[1]
    for flavour, rows in (("graph", 20), ("graph_fewshot", tu[3].shape[0])):
        banks = []
        for mode in ("device", "host"):
            tgb = ToyGraphBase(pre, 2, 256, 1, device=dev, flavour=flavour)
            tgb.build_rng = mode
            tgb.build_toy_graph(ds)
            assert tgb.resource_keys.shape == (rows, 256) and tgb.resource_labels.shape == (rows, 2)
            assert tgb.last_build_seed is None         # no sampling, no augmentation: no seed is drawn either
            banks.append(tgb)
        assert torch.equal(banks[0].resource_keys, banks[1].resource_keys)
        assert torch.equal(banks[0].resource_values, banks[1].resource_values)


def _edge_dataset(dev, U=600, I=400):
    from ragraph_amd.data import synthetic_bipartite

    edges, norm, times = synthetic_bipartite(U, I, edges_per_user=6, seed=11, device=dev)

    class DS:
        num_users, num_items = U, I
    DS.edges, DS.edge_norm, DS.edge_times = edges, norm, times

    class Pre:
        def generate(self):
            g = torch.Generator(device=dev).manual_seed(3)
            return 0.1 * torch.randn(U, 64, device=dev, generator=g), 0.1 * torch.randn(I, 64, device=dev, generator=g)
    return DS, Pre()


def test_edge_vanilla_phase_samples_first_and_augments_the_picked_rows(dev, no_host_draws, monkeypatch):
    from ragraph_amd import kernels as K
    from ragraph_amd.RAGraph_edge import RAGraph as RAGraphEdge

    U, I, S, D = 600, 400, 10, 64
    n = U + I
    DS, pre = _edge_dataset(dev, U, I)
    torch.manual_seed(0)
    m = RAGraphEdge(DS, pre, phase="vanilla", use_RAG=True, retrieve_num=5, num_augment_scale=1, num_inverse_sample=S,
                    device=dev, build_rng="device").eval()
    assert m.build_rng == "device"
    assert m.resource_keys.shape == (2 * S, D) and m.resource_values.shape == (2 * S, D)
    seeds = m.last_build_seed
    assert seeds.shape == (2, K.BUILD_SEED_COLUMNS)
    full = RAGraphEdge(DS, pre, phase="vanilla", use_RAG=True, retrieve_num=5, device=dev, build_rng="device")
    assert full.last_build_seed is None and full.resource_keys.shape == (n, D)
    # the replay: pick, gather, augment the gathered rows keyed by the node
    prob = m.sample_prob()
    whole = torch.tensor([0, n], dtype=torch.int64, device=dev)
    col = lambda v, c: seeds[v, c:c + 1]
    pick0 = K.multinomial_segments(prob, whole, S, col(0, K.BUILD_SEED_PICK)).reshape(-1)
    assert np.array_equal(pick0.cpu().numpy(), B.multinomial_segments(int(seeds[0, K.BUILD_SEED_PICK]), prob.cpu().numpy(),
                                                                      np.array([0, n]), S)[0])
    assert torch.equal(m.resource_keys[:S], full.resource_keys[pick0])          # rows of the unsampled bank
    assert torch.equal(m.resource_values[:S], full.resource_values[pick0])
    pick1 = K.multinomial_segments(prob, whole, S, col(1, K.BUILD_SEED_PICK)).reshape(-1)
    p1 = prob[pick1]
    want_k = K.augment_features(full.resource_keys[pick1], p1, col(1, K.BUILD_SEED_NODE_DROP), col(1, K.BUILD_SEED_FEATURE_NOISE),
                                row_ids=pick1)
    want_v = K.augment_features(full.resource_values[pick1], p1, col(1, K.BUILD_SEED_VALUE_DROP), col(1, K.BUILD_SEED_VALUE_NOISE),
                                row_ids=pick1)
    assert torch.equal(bits(m.resource_keys[S:]), bits(want_k)) and torch.equal(bits(m.resource_values[S:]), bits(want_v))
    # no noise or mask over a whole table: the peak of _sample_bank stays below ONE [n, D] table plus the outputs
    monkeypatch.setattr(m, "sample_prob", lambda: prob)
    keys, vals = full.resource_keys, full.resource_values
    m._sample_bank(keys, vals)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = m._sample_bank(keys, vals)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"edge _sample_bank, device draws: peak {peak} bytes; one table {n * D * 4}")
    assert out[0].shape == (2 * S, D) and peak < n * D * 4 + 2 * (2 * S * D * 4)
    uo, io = m.generate()
    assert bool(torch.isfinite(uo).all()) and bool(torch.isfinite(io).all()) and uo.shape == (U, D)


def test_host_mode_builds_as_before_without_a_new_kernel(dev, tu, no_new_kernels):
    from ragraph_amd.RAGraph_edge import RAGraph as RAGraphEdge

    a, b = _node_bank(tu, dev, 5, "host"), _node_bank(tu, dev, 5, "host")
    assert a.build_rng == "host" and a.last_build_seed is None
    assert a.resource_keys.shape == (20 * 10 * 4, 256) and a.resource_positions.shape == (800, 10)
    assert torch.equal(a.resource_keys, b.resource_keys) and torch.equal(a.resource_values, b.resource_values)
    DS, pre = _edge_dataset(dev)
    torch.manual_seed(0)
    m = RAGraphEdge(DS, pre, phase="vanilla", use_RAG=True, retrieve_num=5, num_augment_scale=1, num_inverse_sample=10, device=dev)
    assert m.build_rng == "host" and m.last_build_seed is None and m.resource_keys.shape == (20, 64)
