"""Structure-aware retrieval on the GPU: K.topk_cosine_mix (ragraph_topk_cosine_mix_f32) and the flavours that call it.

Every comparison is bit-exact (scores and indices) against the CPU oracle (oracle.pipeline.fewshot_scores / cref) or
against the materialised device composition the library already had (normalize_rows, linear x 2, axpby, topk_rows);
nothing is compared with the new kernels themselves."""
import os

import numpy as np
import pytest
import torch

from oracle import cref, pipeline

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def make_codes(rng, n, A, zero_rows=0.03):
    """Codes of the reference's form (PositionAwareEncoder.py:17-24): 1 / (d + 1) for a hop distance d, 0 for an anchor
    that cannot be reached; some rows reach no anchor at all."""
    d = rng.integers(0, 7, (n, A)).astype(np.float32)
    c = (1.0 / (d + 1.0)).astype(np.float32)
    c[rng.random((n, A)) < 0.3] = 0.0
    c[rng.random(n) < zero_rows] = 0.0
    return c


def oracle_topk(q, kn, pq, pnn, ws, wm, k):
    s = cref.axpby(cref.linear(cref.normalize_rows(pq), pnn), np.float32(ws), cref.linear(cref.normalize_rows(q), kn),
                   np.float32(wm))
    return cref.topk_rows(s, k)


def compose_topk(K, q, knd, pq, pnd, ws, wm, k, rows=None):
    """The materialised composition on the device, in query chunks."""
    B = q.shape[0]
    rows = rows or B
    out_s, out_i = [], []
    for b0 in range(0, B, rows):
        s_sem = K.linear(K.normalize_rows(q[b0:b0 + rows].contiguous()), knd)
        s_str = K.linear(K.normalize_rows(pq[b0:b0 + rows].contiguous()), pnd)
        s, i = K.topk_rows(K.axpby(s_str, ws, s_sem, wm), k)
        del s_sem, s_str
        out_s.append(s)
        out_i.append(i)
    return torch.cat(out_s), torch.cat(out_i)


def both_kernel_families(monkeypatch):
    """Small shapes take materialised slabs by rule; RAGRAPH_TOPK_SLAB=0 (read per call) sends them to the fused kernels."""
    for v in (None, "0"):
        if v is None:
            monkeypatch.delenv("RAGRAPH_TOPK_SLAB", raising=False)
        else:
            monkeypatch.setenv("RAGRAPH_TOPK_SLAB", v)
        yield v


# ---- 1, 2: the golden few-shot retrieve ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ws,wm", [(0.001, 0.999), (0.3, 0.7), (0.5, 0.5)])
def test_g8_mixed_topk_equals_oracle(dev, monkeypatch, ws, wm):
    from ragraph_amd import kernels as K
    from ragraph_amd.RAGraph_fewshot import PositionAwareEncoder, ToyGraphBaseFewShot

    g = dict(np.load(os.path.join(GOLD, "g8_fewshot_retrieve.npz")))
    k = int(g["k"])
    osc, opos = pipeline.fewshot_scores(g["Q"], g["adj"], g["anchors"], g["keys"], g["positions"], ws, wm)
    os_, oi = cref.topk_rows(osc, k)
    if (ws, wm) == (0.001, 0.999):
        assert np.array_equal(oi, g["topk_idx"])
    tgb = ToyGraphBaseFewShot(None, g["labels"].shape[1], 256, 3, k, device=dev)
    tgb.add_resources(T(g["keys"], dev), T(g["values"], dev), T(g["labels"], dev), T(g["positions"], dev))
    tgb.structure_weight, tgb.semantic_weight = ws, wm
    adj, anchors = T(g["adj"], dev), T(g["anchors"], dev)
    pos = PositionAwareEncoder.encode_position_aware_code(adj, 10, 10, anchors=anchors)
    assert np.array_equal(pos.cpu().numpy(), opos)
    for _ in both_kernel_families(monkeypatch):
        s, i = tgb.topk(T(g["Q"], dev), k, pos)
        assert np.array_equal(i.cpu().numpy(), oi) and np.array_equal(s.cpu().numpy(), os_)
        s2, i2 = K.topk_cosine_mix(T(g["Q"], dev), tgb.keys_normalized, pos, tgb.positions_normalized, ws, wm, k, idx_base=1000)
        assert np.array_equal(i2.cpu().numpy(), oi + 1000) and np.array_equal(s2.cpu().numpy(), os_)
        e, l = tgb.retrieve(T(g["Q"], dev), adj, False, anchors=anchors)
        assert np.array_equal(e.cpu().numpy(), cref.gather_rows(g["values"], oi))
        assert np.array_equal(l.cpu().numpy(), cref.gather_rows(g["labels"], oi))


# ---- 3: synthetic sweep against the oracle ------------------------------------------------------------------------------
#          D,   A,  B,   N,     k,   (w_struct, w_sem)
SWEEP = [
    (256, 10, 1, 33333, 5, (0.3, 0.7)),
    (256, 10, 16, 33333, 32, (0.3, 0.7)),
    (256, 16, 100, 33333, 5, (-0.2, 1.0)),
    (256, 4, 129, 33333, 1, (0.3, 0.7)),
    (256, 10, 700, 33333, 5, (0.3, 0.7)),
    (256, 10, 700, 33333, 32, (-0.2, 1.0)),
    (256, 10, 700, 33333, 33, (0.3, 0.7)),      # k beyond the fused kernels' lists: slabs
    (256, 16, 129, 33333, 64, (0.3, 0.7)),
    (256, 10, 100, 33333, 200, (0.3, 0.7)),     # ordered large-k selection
    (256, 10, 700, 1000, 200, (-0.2, 1.0)),
    (256, 10, 16, 1000, 5, (1.0, 0.0)),         # structural term alone
    (256, 4, 129, 33333, 5, (1.0, 0.0)),
    (256, 10, 100, 1000, 5, (0.3, -0.7)),       # a negative semantic weight
    (128, 10, 700, 1000, 32, (0.3, 0.7)),
    (128, 16, 129, 33333, 5, (-0.2, 1.0)),
    (128, 4, 16, 33333, 1, (0.3, 0.7)),
    (128, 10, 1, 1000, 33, (0.3, 0.7)),
    (64, 16, 129, 33333, 5, (0.3, 0.7)),
    (64, 4, 16, 1000, 1, (-0.2, 1.0)),
    (64, 10, 700, 33333, 32, (0.3, 0.7)),
    (64, 10, 100, 33333, 64, (1.0, 0.0)),
    (96, 10, 100, 33333, 5, (0.3, 0.7)),        # a width without a fused kernel: slabs
    (96, 16, 700, 1000, 32, (-0.2, 1.0)),
    (96, 4, 1, 1000, 200, (0.3, 0.7)),
    (96, 10, 129, 33333, 33, (1.0, 0.0)),
] + [(D, 10, B, k, k, w) for D, B, k, w in (                                     # N = k: every key is selected
    (256, 16, 1, (0.3, 0.7)), (256, 1, 5, (-0.2, 1.0)), (128, 129, 32, (0.3, 0.7)), (64, 100, 33, (0.3, 0.7)),
    (256, 700, 64, (1.0, 0.0)), (96, 16, 200, (0.3, 0.7)), (256, 129, 200, (-0.2, 1.0)))]


@pytest.mark.parametrize("D,A,B,N,k,w", SWEEP)
def test_sweep_against_the_oracle(dev, monkeypatch, D, A, B, N, k, w):
    from ragraph_amd import kernels as K

    rng = np.random.default_rng(D * 7 + A * 5 + B * 3 + N + k)
    kn = cref.normalize_rows(rng.standard_normal((N, D), dtype=np.float32))
    q = rng.standard_normal((B, D), dtype=np.float32)
    pnn = cref.normalize_rows(make_codes(rng, N, A))
    pq = make_codes(rng, B, A)
    os_, oi = oracle_topk(q, kn, pq, pnn, w[0], w[1], k)
    knd, pnd, qd, pqd = T(kn, dev), T(pnn, dev), T(q, dev), T(pq, dev)
    assert torch.equal(K.normalize_rows(T(make_codes(np.random.default_rng(1), 50, A), dev)).cpu(),
                       torch.from_numpy(cref.normalize_rows(make_codes(np.random.default_rng(1), 50, A))))
    for fam in both_kernel_families(monkeypatch):
        s, i = K.topk_cosine_mix(qd, knd, pqd, pnd, w[0], w[1], k)
        assert np.array_equal(i.cpu().numpy(), oi), (fam, "indices")
        assert np.array_equal(s.cpu().numpy(), os_), (fam, "scores")
    assert not np.isnan(os_).any()


# ---- 4, 5: at size, against the device composition -----------------------------------------------------------------------
def _big_inputs(dev, B, N, D, A, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    from ragraph_amd import kernels as K

    kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
    q = torch.randn(B, D, device=dev, generator=g)

    def codes(n):
        d = torch.randint(0, 7, (n, A), device=dev, generator=g).float()
        c = 1.0 / (d + 1.0)
        c[torch.rand(n, A, device=dev, generator=g) < 0.3] = 0.0
        return c

    return q, kn, codes(B), K.normalize_rows(codes(N))


def test_at_size_equals_the_materialised_composition(dev):
    from ragraph_amd import kernels as K

    B, N, D, A, k = 4096, 262144, 256, 10, 10
    q, kn, pq, pnn = _big_inputs(dev, B, N, D, A, 11)
    for ws, wm in ((0.001, 0.999), (0.3, 0.7)):
        s, i = K.topk_cosine_mix(q, kn, pq, pnn, ws, wm, k)
        cs, ci = compose_topk(K, q, kn, pq, pnn, ws, wm, k, rows=512)
        assert torch.equal(i, ci) and torch.equal(s, cs), (ws, wm)
    sem_s, sem_i = K.topk_cosine(q, kn, k)
    assert not torch.equal(i, sem_i)          # (0.3, 0.7): the structural term changes the answer


def test_no_score_matrix_at_bank_scale(dev):
    from ragraph_amd import kernels as K

    B, N, D, A, k = 4096, 1 << 20, 256, 10, 10
    q, kn, pq, pnn = _big_inputs(dev, B, N, D, A, 12)
    K._ws_cache.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    s, i = K.topk_cosine_mix(q, kn, pq, pnn, 0.05, 0.95, k)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    assert growth < B * N * 4 // 8, growth
    rows = torch.randperm(B, generator=torch.Generator().manual_seed(3))[:64].to(dev)
    cs, ci = compose_topk(K, q[rows], kn, pq[rows], pnn, 0.05, 0.95, k)
    assert torch.equal(i[rows], ci) and torch.equal(s[rows], cs)


# ---- 6: edge cases -------------------------------------------------------------------------------------------------------
def test_duplicates_zero_rows_and_semantic_only_weights(dev, monkeypatch):
    from ragraph_amd import kernels as K
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    rng = np.random.default_rng(21)
    N, D, A, B, k = 20000, 128, 10, 40, 8
    keys = cref.normalize_rows(rng.standard_normal((N, D), dtype=np.float32))
    codes = make_codes(rng, N, A, zero_rows=0.0)
    q = rng.standard_normal((B, D), dtype=np.float32)
    pq = make_codes(rng, B, A, zero_rows=0.0)
    # every query has 12 exact copies (keys AND codes) of one strong match scattered over the bank
    for b in range(B):
        rows = rng.choice(N, 12, replace=False)
        keys[rows] = cref.normalize_rows(q[b:b + 1] + 0.05 * rng.standard_normal((1, D), dtype=np.float32))
        codes[rows] = 0.0 if b == 11 else pq[b]   # (query 11's matches reach no anchor: selected on the semantic term alone)
    codes[::9] = 0.0                  # more bank rows that reach no anchor
    pq[5] = 0.0                       # a query node that reaches none
    q[7] = 0.0                        # an all-zero query embedding
    keys[3] = 0.0                     # (and an all-zero key row)
    kn, pnn = cref.normalize_rows(keys), cref.normalize_rows(codes)
    os_, oi = oracle_topk(q, kn, pq, pnn, 0.3, 0.7, k)
    knd, pnd, qd, pqd = T(kn, dev), T(pnn, dev), T(q, dev), T(pq, dev)
    for fam in both_kernel_families(monkeypatch):
        s, i = K.topk_cosine_mix(qd, knd, pqd, pnd, 0.3, 0.7, k)
        assert not torch.isnan(s).any()
        assert np.array_equal(i.cpu().numpy(), oi) and np.array_equal(s.cpu().numpy(), os_), fam
        # equal scores come out in ascending index order
        sn, inn = s.cpu().numpy(), i.cpu().numpy()
        tied = sn[:, 1:] == sn[:, :-1]
        assert tied.sum() >= B and (inn[:, 1:][tied] > inn[:, :-1][tied]).all()
        # a zero code row on either side: the structural term is exactly 0, i.e. the score is 0 * w_struct + s_sem * w_sem
        sem = cref.linear(cref.normalize_rows(q), kn)
        zero_term = cref.axpby(np.zeros_like(sem), np.float32(0.3), sem, np.float32(0.7))
        assert np.array_equal(sn[5], np.take_along_axis(zero_term[5:6], inn[5:6], 1)[0])
        zero_keys = (codes[inn] == 0).all(-1)
        assert zero_keys[11].all() and np.array_equal(sn[zero_keys], np.take_along_axis(zero_term, inn, 1)[zero_keys])
        # weights (0, 1): the semantic-only answer (a product of -0 reads +0 after 0 * s_struct is added)
        tgb = ToyGraphBase(None, 3, D, 3, device=dev)
        tgb.add_resources(T(keys, dev), T(keys, dev), torch.zeros(N, 3, device=dev), T(codes, dev))
        s_sem, i_sem = tgb.topk(qd, k)
        s01, i01 = K.topk_cosine_mix(qd, tgb.keys_normalized, pqd, tgb.positions_normalized, 0.0, 1.0, k)
        assert torch.equal(i01, i_sem) and torch.equal(s01 + 0.0, s_sem + 0.0)
        tgb.structure_weight, tgb.semantic_weight = 0.0, 0.999    # the default: KeyIndex, scores NOT scaled
        s_d, i_d = tgb.topk(qd, k, pqd)
        assert torch.equal(i_d, i_sem) and torch.equal(s_d, s_sem)


# ---- 7: the flavours -----------------------------------------------------------------------------------------------------
def _ring_of_cliques(n, dev, seed):
    """A sparse symmetric query graph of n nodes with self loops, as CSR (edge weights in (0, 1])."""
    from ragraph_amd.graph import CSRGraph

    rng = np.random.default_rng(seed)
    src = np.arange(n)
    nbr = np.stack([(src + 1) % n, (src + 7) % n, rng.integers(0, n, n)], 1)
    rows = np.concatenate([src, np.repeat(src, 3), nbr.reshape(-1)])
    cols = np.concatenate([src, nbr.reshape(-1), np.repeat(src, 3)])
    key = np.unique(rows.astype(np.int64) * n + cols)
    rows, cols = key // n, key % n
    val = np.full(rows.shape[0], 0.25, dtype=np.float32)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, rows + 1, 1)
    rowptr = np.cumsum(rowptr)
    return CSRGraph(T(rowptr, dev), T(cols.astype(np.int32), dev), T(val, dev), n), (rowptr, cols.astype(np.int32), val)


def test_fewshot_retrieve_on_a_large_bank_without_the_matrix(dev):
    from ragraph_amd import kernels as K
    from ragraph_amd.RAGraph_fewshot import PositionAwareEncoder, ToyGraphBaseFewShot

    N, n, D, C, k = 200000, 5000, 256, 4, 5
    g = torch.Generator(device=dev).manual_seed(5)
    q, kn, _, _ = _big_inputs(dev, n, N, D, 10, 31)
    d = torch.randint(0, 7, (N, 10), device=dev, generator=g).float()
    bank_codes = 1.0 / (d + 1.0)
    labels = torch.nn.functional.one_hot(torch.randint(0, C, (N,), device=dev, generator=g), C).float()
    tgb = ToyGraphBaseFewShot(None, C, D, 3, k, device=dev)
    tgb.set_resources(kn, kn, labels, bank_codes)
    tgb.structure_weight, tgb.semantic_weight = 0.05, 0.95
    graph, _ = _ring_of_cliques(n, dev, 2)
    anchors = torch.randint(0, n, (10,), generator=torch.Generator().manual_seed(9)).to(dev)
    K._ws_cache.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    e, l = tgb.retrieve(q, graph, False, anchors=anchors)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < n * N * 4 // 8
    assert e.shape == (n, k, D) and l.shape == (n, k, C)
    idx = tgb.retrieve_indices(q, False, graph, anchors=anchors)
    rows = torch.arange(0, n, 79, device=dev)
    pos = PositionAwareEncoder.encode_position_aware_code(graph, 10, 10, anchors=anchors)
    _, ci = compose_topk(K, q[rows], kn, pos[rows], K.normalize_rows(bank_codes), 0.05, 0.95, k)
    assert torch.equal(idx[rows], ci)
    assert torch.equal(e[rows], K.gather_rows(kn, ci)) and torch.equal(l[rows], K.gather_rows(labels, ci))


def _node_model(dev, N=5000):
    from ragraph_amd.data import DataLoader, synthetic_tu_dataset
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph import RAGraph
    from ragraph_amd.ragraph_utils import process_tu_dataset

    torch.manual_seed(0)
    F_in, C, D = 18, 3, 256
    ds = synthetic_tu_dataset(num_graphs=8, num_node_attributes=F_in, num_node_labels=C, seed=3)
    pre = PrePrompt(F_in, D, "prelu", 1, 0.3).to(dev)
    model = RAGraph(pre, None, F_in, C, D, finetune=True, device=dev).eval()
    rng = np.random.default_rng(4)
    keys = cref.normalize_rows(rng.standard_normal((N, D), dtype=np.float32))
    vals = rng.standard_normal((N, D), dtype=np.float32)
    labs = np.eye(C, dtype=np.float32)[rng.integers(0, C, N)]
    codes = make_codes(rng, N, 10)
    model.toy_graph_base.add_resources(T(keys, dev), T(vals, dev), T(labs, dev), T(codes, dev))
    feats, adj, _ = process_tu_dataset(next(iter(DataLoader(ds, batch_size=8))), F_in, device=dev)
    return model, pre, feats, adj, (keys, vals, labs, codes)


def _recompose_forward(model, pre, feats, adj, idx):
    from ragraph_amd import kernels as K
    from ragraph_amd.graph import as_csr
    from ragraph_amd.ragraph_utils.Propagation import Propagation

    tgb = model.toy_graph_base
    g = as_csr(adj)
    h = pre.inference(feats, g)
    sum_v, mean_l = K.gather_reduce(tgb.resource_values, tgb.resource_labels, idx)
    query = Propagation.aggregate_k_hop_features(g, h, model.query_graph_hop)
    return model._fuse_decode(query, sum_v, mean_l)


def test_node_forward_with_and_without_the_structural_weight(dev):
    from ragraph_amd import kernels as K
    from ragraph_amd.graph import as_csr

    model, pre, feats, adj, (keys, vals, labs, codes) = _node_model(dev)
    tgb = model.toy_graph_base
    g = as_csr(adj)
    n = feats.shape[0]
    anchors = torch.randint(0, n, (10,), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        h = pre.inference(feats, g)
        # default weight: the parent's path, bit for bit
        out0 = model(feats, adj)
        _, idx0 = tgb._index.topk(h, tgb.retrieve_num)
        assert torch.equal(out0, _recompose_forward(model, pre, feats, adj, idx0))
        assert torch.equal(model(feats, adj, anchors=anchors.to(dev)), out0)        # anchors are not read at weight 0
        # structural weight 0.3: indices from the oracle, output recomposed from the existing kernels on them
        tgb.structure_weight, tgb.semantic_weight = 0.3, 0.7
        out = model(feats, adj, anchors=anchors.to(dev))
        _, _, idx = tgb.retrieve_reduced(h, search_adj=g, anchors=anchors.to(dev))
    csr = (g.rowptr.cpu().numpy(), g.col.cpu().numpy(), g.val.cpu().numpy())
    opos, _ = cref.position_codes_csr(*csr, anchors.numpy(), 10.0)
    _, oi = oracle_topk(h.cpu().numpy(), cref.normalize_rows(keys), opos, cref.normalize_rows(codes), 0.3, 0.7, tgb.retrieve_num)
    assert np.array_equal(idx.cpu().numpy(), oi)
    assert not torch.equal(idx, idx0)
    with torch.no_grad():
        assert torch.equal(out, _recompose_forward(model, pre, feats, adj, T(oi, dev)))
        # a bank without codes: refused before any retrieval kernel
        tgb.set_resources(tgb.resource_keys, tgb.resource_values, tgb.resource_labels)
        with pytest.raises(ValueError, match="position"):
            model(feats, adj, anchors=anchors.to(dev))


def test_sharded_bank_with_a_structural_weight_raises(dev):
    from ragraph_amd import kernels as K
    from ragraph_amd.sharded import QueryShard, ShardedToyGraphBase

    model, pre, feats, adj, (keys, vals, labs, codes) = _node_model(dev)
    single = model.toy_graph_base
    sharded = ShardedToyGraphBase(T(keys, dev), T(vals, dev), T(labs, dev), 0, single.retrieve_num, values_replicated=True,
                                  emulate_world=2)
    sharded.structure_weight = 0.3
    model.toy_graph_base = sharded
    with torch.no_grad(), pytest.raises(K.RagraphNativeError, match="structure"):
        model(feats, adj)
    model.toy_graph_base = single
    single.structure_weight = 0.3
    model.query_shard = QueryShard()
    with torch.no_grad(), pytest.raises(K.RagraphNativeError, match="structure"):
        model(feats, adj)


# ---- 8: capture ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,D,k", [(16, 70000, 256, 10), (300, 140000, 128, 5), (40, 3000, 256, 40)])
def test_mixed_call_is_captured_and_replayed(dev, B, N, D, k):
    """Recorded under torch.cuda.graph (a synchronisation or a host read inside the call would fail the capture) and
    replayed on new query contents: the replay equals the eager call."""
    from ragraph_amd import kernels as K

    A = 10
    q, kn, pq, pnn = _big_inputs(dev, B, N, D, A, 41)
    q2, _, pq2, _ = _big_inputs(dev, B, 8, D, A, 42)
    K.topk_cosine_mix(q, kn, pq, pnn, 0.3, 0.7, k)                     # (warm-up: workspace, LDS attributes)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.topk_cosine_mix(q, kn, pq, pnn, 0.3, 0.7, k)
        torch.cuda.synchronize()
        sq, spq = q.clone(), pq.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            gs, gi = K.topk_cosine_mix(sq, kn, spq, pnn, 0.3, 0.7, k)
        sq.copy_(q2)
        spq.copy_(pq2)
        graph.replay()
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    es, ei = K.topk_cosine_mix(q2, kn, pq2, pnn, 0.3, 0.7, k)
    assert torch.equal(gi, ei) and torch.equal(gs, es)
    cs, ci = compose_topk(K, q2, kn, pq2, pnn, 0.3, 0.7, k)
    assert torch.equal(ei, ci) and torch.equal(es, cs)


# ---- 9: the clock --------------------------------------------------------------------------------------------------------
def _median_ms(fn, reps=7):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


# Measured on one MI355X (profiles/topk_mix.txt, section 2): semantic fp32 16.66 ms, mixed (0.001, 0.999) 18.07 ms at
# B = 4096, N = 2^20, D = 256, A = 10, k = 10: ratio 1.083 (1.08 in both alternating rounds).  Bound = measured + 15 %
# (boxes of the pool differ by 8 % in clock, README): 1.083 + 0.15 = 1.233, the stricter of the two readings of "+ 15 %".
MIX_RATIO_MEASURED = 1.083
MIX_RATIO_BOUND = 1.233


@pytest.mark.perf
def test_mixed_call_costs_what_the_semantic_fp32_call_costs(dev):
    """B = 4096 queries x 2^20 keys, D = 256, A = 10, k = 10, at the few-shot flavour's weights (0.001, 0.999): the mixed
    call against the semantic-only exact fp32 call (ragraph_topk_cosine_bank_f32, Kp = NULL) in the same process."""
    from ragraph_amd import kernels as K

    B, N, D, A, k = 4096, 1 << 20, 256, 10, 10
    q, kn, pq, pnn = _big_inputs(dev, B, N, D, A, 12)
    t_sem = _median_ms(lambda: K.topk_cosine(q, kn, k))
    t_mix = _median_ms(lambda: K.topk_cosine_mix(q, kn, pq, pnn, 0.001, 0.999, k))
    print(f"semantic fp32 {t_sem:.3f} ms, mixed {t_mix:.3f} ms, ratio {t_mix / t_sem:.3f} (bound {MIX_RATIO_BOUND})")
    assert t_mix / t_sem <= MIX_RATIO_BOUND
