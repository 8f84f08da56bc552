"""Position codes of large query graphs: the chip-wide relaxation with the distance vectors in
global memory (ragraph_position_codes_csr_global_f32) against the CPU oracle, which has no size limit.  Codes and
distances are compared with np.array_equal: the contract is the oracle's bits."""
import numpy as np
import pytest
import torch

from oracle import cref

pytestmark = pytest.mark.gpu
DIS_Q = 10.0


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def csr_from_degrees(rng, deg, n_targets, lo, hi):
    """Rows of the given out-degrees, targets uniform in [0, n_targets), weights U(lo, hi)."""
    rowptr = np.zeros(deg.size + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, n_targets, int(rowptr[-1])).astype(np.int32)
    val = rng.uniform(lo, hi, int(rowptr[-1])).astype(np.float32)
    return rowptr, col, val


def sparse_graph(n, seed, empty=0.05, zeros=0.02):
    """5 % of the rows empty, the others 4 out-edges; weights U(0.5, 2.5), 2 % of the entries explicit zeros; a duplicate anchor."""
    rng = np.random.default_rng(seed)
    deg = np.where(rng.random(n) < empty, 0, 4).astype(np.int64)
    rowptr, col, val = csr_from_degrees(rng, deg, n, 0.5, 2.5)
    val[rng.random(val.size) < zeros] = 0.0
    anchors = rng.integers(0, n, 10)
    anchors[3] = anchors[2]
    return rowptr, col, val, anchors


def chain_graph(n=41000, hops=199, seed=3, scale=1.0):
    """A chain of hops + 1 nodes with ascending ids, base[i] -> base[i + 1] at weight 0.04, anchor 0 at its end; every other
    node has 2 random out-edges of weight U(8, 12), so no shortcut beats the chain (199 * 0.04 < 8)."""
    rng = np.random.default_rng(seed)
    base = np.sort(rng.choice(n, hops + 1, replace=False))
    deg = np.full(n, 2, dtype=np.int64)
    deg[base[:-1]] = 1
    rowptr, col, val = csr_from_degrees(rng, deg, n, 8.0, 12.0)
    col[rowptr[base[:-1]]] = base[1:]
    val[rowptr[base[:-1]]] = 0.04
    anchors = rng.integers(0, n, 10)
    anchors[0] = base[-1]
    return rowptr, col, (val * np.float32(scale)).astype(np.float32), anchors, base


_oracle_cache = {}


def oracle(key, rowptr, col, val, anchors):
    """The oracle's (codes, dist), computed once per graph and shared (read only)."""
    if key not in _oracle_cache:
        oc, od = cref.position_codes_csr(rowptr, col, val, anchors, DIS_Q)
        oc.setflags(write=False)
        od.setflags(write=False)
        _oracle_cache[key] = (oc, od)
    return _oracle_cache[key]


def run(K, dev, rowptr, col, val, anchors, **kw):
    out = K.position_codes_csr(T(rowptr, dev), T(col, dev), T(val, dev), T(anchors, dev), DIS_Q, return_dist=True, **kw)
    return tuple(t.cpu().numpy() for t in out)


# ---- 1: small shapes, forced global path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 10, 16, 17])
@pytest.mark.parametrize("n,deg", [(97, 0.05), (528, 0.01), (3000, 0.002)])
def test_small_graphs_forced_global_equal_oracle_and_lds_kernel(dev, n, deg, A):
    """The graphs of test_position_codes_csr_bit_exact_vs_oracle: an unreachable half, explicit zero entries, self-loops,
    duplicate anchors; one column chunk, a full one, and two."""
    from ragraph_amd import kernels as K

    rng = np.random.default_rng(n)
    a = (rng.random((n, n)) < deg).astype(np.float32) * rng.random((n, n)).astype(np.float32)
    a = np.maximum(a, a.T)
    np.fill_diagonal(a, 0.3)
    a[n // 2:, : n // 2] = 0
    rowptr, col, val = cref.dense_to_csr(a)
    val = val.copy()
    val[::17] = 0.0
    anchors = rng.integers(0, n, A)
    if A > 3:
        anchors[3] = anchors[2]
    oc, od = cref.position_codes_csr(rowptr, col, val, anchors, DIS_Q)
    codes, dist = run(K, dev, rowptr, col, val, anchors, method="global")
    assert np.array_equal(dist, od) and np.array_equal(codes, oc)
    lc, ld = run(K, dev, rowptr, col, val, anchors)
    assert np.array_equal(dist, ld) and np.array_equal(codes, lc)
    if A >= 10:
        assert np.isinf(od).any() and np.isfinite(od).any()


# ---- 2: just past the LDS kernel's limit, default dispatch ----------------------------------------------------------------
@pytest.mark.parametrize("n", [40001, 70001])
def test_past_the_lds_limit_default_dispatch_equals_oracle(dev, n):
    """Raised RagraphNativeError before the global path existed."""
    from ragraph_amd import kernels as K

    rowptr, col, val, anchors = sparse_graph(n, 1)
    oc, od = oracle(("sparse", n), rowptr, col, val, anchors)
    share = float((oc != 0).mean())
    print(f"n={n}: non-zero codes {share:.3f}, infinite {np.isinf(od).mean():.3f}, "
          f"finite >= dis_q {(np.isfinite(od) & (od >= DIS_Q)).mean():.3f}")
    assert 0.1 < share < 0.9                       # both branches of the code expression; a degenerate generator cannot pass
    assert np.isinf(od).any() and (np.isfinite(od) & (od >= DIS_Q)).any()
    codes, dist = run(K, dev, rowptr, col, val, anchors)
    assert np.array_equal(dist, od) and np.array_equal(codes, oc)


def test_node_flavour_headline_size_equals_oracle(dev):
    """100 000 nodes, the node flavour's headline graph size: both branches of the code expression and unreachable nodes."""
    from ragraph_amd import kernels as K

    rowptr, col, val, anchors = sparse_graph(100000, 2)
    oc, od = cref.position_codes_csr(rowptr, col, val, anchors, DIS_Q)
    assert (oc != 0).any() and (oc == 0).any() and np.isinf(od).any()
    codes, dist = run(K, dev, rowptr, col, val, anchors)
    assert np.array_equal(dist, od) and np.array_equal(codes, oc)


# ---- 3: a deep path across several read-back batches ----------------------------------------------------------------------
def test_deep_chain_across_read_back_batches(dev):
    from ragraph_amd import kernels as K

    rowptr, col, val, anchors, base = chain_graph()
    oc, od = oracle("chain", rowptr, col, val, anchors)
    assert abs(float(od[base[0], 0]) - 7.959994) < 1e-6          # 199 hops of 0.04, summed from the anchor's end in fp32
    assert 199 > 3 * K.POSITION_CODES_ROUNDS_PER_READBACK         # (several batches of the eager driver)
    codes, dist = run(K, dev, rowptr, col, val, anchors)
    assert np.array_equal(dist, od) and np.array_equal(codes, oc)
    assert dist[base[0], 0] == od[base[0], 0]


# ---- 4: long rows ---------------------------------------------------------------------------------------------------------
def test_long_rows_and_an_anchor_behind_the_hub(dev):
    """One row of degree 40000, rows of exactly the long-row threshold and threshold +- 1, and an anchor (node n - 1) that
    only the hub points to; 17 anchors, so long rows run in both column chunks."""
    from ragraph_amd import _native as N
    from ragraph_amd import kernels as K

    n, hub, far = 45000, 1234, 44999
    thr = N.POSITION_CODES_LONG_ROW
    rng = np.random.default_rng(11)
    deg = np.full(n, 3, dtype=np.int64)
    deg[hub] = 40000
    deg[[7, 20000, 44000]] = [thr - 1, thr, thr + 1]
    rowptr, col, val = csr_from_degrees(rng, deg, n - 1, 0.1, 0.5)     # nobody points to node n - 1 ...
    val[rng.random(val.size) < 0.02] = 0.0
    h0 = rowptr[hub]
    col[h0:h0 + 40000] = rng.permutation(n - 1)[:40000]
    col[h0 + 39999] = far                                             # ... but the hub, with its last edge
    val[h0 + 39999] = 0.25
    anchors = rng.integers(0, n - 1, 17)
    anchors[0] = far
    anchors[16] = 20000                                               # second chunk: a row of exactly the threshold
    oc, od = cref.position_codes_csr(rowptr, col, val, anchors, DIS_Q)
    reach = np.isfinite(od[:, 0])
    assert reach[hub] and reach.sum() > 1000 and (oc[:, 0] != 0).sum() > 1000    # reached through the hub only
    codes, dist = run(K, dev, rowptr, col, val, anchors)
    assert np.array_equal(dist, od) and np.array_equal(codes, oc)


# ---- 5: fixed rounds, capture ---------------------------------------------------------------------------------------------
def test_fixed_rounds_converged_word_and_upper_bounds(dev):
    from ragraph_amd import kernels as K

    rowptr, col, val, anchors, _ = chain_graph()
    oc, od = oracle("chain", rowptr, col, val, anchors)
    codes, dist, word = run(K, dev, rowptr, col, val, anchors, rounds=400, return_converged=True)
    assert word.tolist() == [1]
    assert np.array_equal(dist, od) and np.array_equal(codes, oc)
    codes2, dist2, word2 = run(K, dev, rowptr, col, val, anchors, rounds=2, return_converged=True)
    assert word2.tolist() == [0]
    assert (dist2 >= od).all() and (codes2 <= oc).all() and not np.array_equal(dist2, od)


def test_fixed_rounds_call_is_captured_and_replayed_on_new_weights(dev):
    from ragraph_amd import kernels as K

    rowptr, col, val, anchors, _ = chain_graph()
    _, _, val2, _, _ = chain_graph(scale=2.0)
    rp, cl, an = T(rowptr, dev), T(col, dev), T(anchors, dev)
    vd = T(val, dev)
    K.position_codes_csr(rp, cl, vd, an, DIS_Q, rounds=2)                          # (warm-up: workspace)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.position_codes_csr(rp, cl, vd, an, DIS_Q, rounds=2)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            gc, gd, gw = K.position_codes_csr(rp, cl, vd, an, DIS_Q, return_dist=True, rounds=400, return_converged=True)
            with pytest.raises(K.RagraphNativeError, match="rounds"):
                K.position_codes_csr(rp, cl, vd, an, DIS_Q)                        # eager mode reads back: not capturable
        vd.copy_(T(val2, dev))
        graph.replay()
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    ec, ed = K.position_codes_csr(rp, cl, vd, an, DIS_Q, return_dist=True)
    assert gw.tolist() == [1]
    assert torch.equal(gd, ed) and torch.equal(gc, ec)
    oc, od = cref.position_codes_csr(rowptr, col, val2, anchors, DIS_Q)
    assert np.array_equal(gd.cpu().numpy(), od) and np.array_equal(gc.cpu().numpy(), oc)


# ---- 6: at the limit, both kernels ----------------------------------------------------------------------------------------
def test_global_path_equals_lds_kernel_at_40000_nodes(dev):
    from ragraph_amd import kernels as K

    n = 40000
    rng = np.random.default_rng(6)
    rowptr, col, val = csr_from_degrees(rng, np.full(n, 10, dtype=np.int64), n, 0.5, 2.5)
    anchors = rng.integers(0, n, 10)
    gc, gd = run(K, dev, rowptr, col, val, anchors, method="global")
    lc, ld = run(K, dev, rowptr, col, val, anchors)
    assert np.array_equal(gd, ld) and np.array_equal(gc, lc)
    assert np.isfinite(ld).all() and np.unique(ld).size > 1000     # (a connected graph: every distance real, none trivial)


# ---- 7: end to end --------------------------------------------------------------------------------------------------------
def test_node_forward_on_a_graph_past_the_lds_limit(dev):
    from ragraph_amd import kernels as K
    from ragraph_amd.graph import CSRGraph
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph import RAGraph
    from ragraph_amd.ragraph_utils.Propagation import Propagation

    torch.manual_seed(0)
    n, F_in, C, D, Nb = 40961, 18, 3, 256, 3000
    rowptr, col, val, anchors = sparse_graph(n, 5, empty=0.0, zeros=0.0)
    g = CSRGraph(T(rowptr, dev), T(col, dev), T(val, dev), n)
    rng = np.random.default_rng(4)
    feats = T(rng.standard_normal((n, F_in), dtype=np.float32), dev)
    pre = PrePrompt(F_in, D, "prelu", 1, 0.3).to(dev)
    model = RAGraph(pre, None, F_in, C, D, finetune=True, device=dev).eval()
    tgb = model.toy_graph_base
    d = rng.integers(0, 7, (Nb, 10)).astype(np.float32)
    bank_codes = (1.0 / (d + 1.0)).astype(np.float32)
    bank_codes[rng.random((Nb, 10)) < 0.3] = 0.0
    tgb.add_resources(T(cref.normalize_rows(rng.standard_normal((Nb, D), dtype=np.float32)), dev),
                      T(rng.standard_normal((Nb, D), dtype=np.float32), dev),
                      T(np.eye(C, dtype=np.float32)[rng.integers(0, C, Nb)], dev), T(bank_codes, dev))
    a = T(anchors, dev)

    def recompose(idx):
        h = pre.inference(feats, g)
        sum_v, mean_l = K.gather_reduce(tgb.resource_values, tgb.resource_labels, idx)
        return model._fuse_decode(Propagation.aggregate_k_hop_features(g, h, model.query_graph_hop), sum_v, mean_l)

    with torch.no_grad():
        out0 = model(feats, g)
        assert torch.equal(model(feats, g, anchors=a), out0)                   # weight 0: anchors are not read
        assert torch.isfinite(out0).all()
        tgb.structure_weight, tgb.semantic_weight = 0.3, 0.7
        out = model(feats, g, anchors=a)
        opos, _ = cref.position_codes_csr(rowptr, col, val, anchors, DIS_Q)
        assert 0.1 < float((opos != 0).mean()) < 0.9
        h = pre.inference(feats, g)
        _, idx = tgb.topk(h, tgb.retrieve_num, search_positions=T(opos, dev))
        _, idx0 = tgb._index.topk(h, tgb.retrieve_num)
        assert not torch.equal(idx, idx0)                                      # the codes move the retrieval
        assert torch.equal(out, recompose(idx))
        # the fixed-round form the captured forward uses: same output, the converged word stays on the device
        tgb.position_rounds = 64
        assert torch.equal(model(feats, g, anchors=a), out)
        assert tgb.last_position_converged.dtype == torch.int32 and tgb.last_position_converged.tolist() == [1]
