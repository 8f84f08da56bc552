"""Ordered top-k beyond k = 64 (csrc/topk_large.hip): kernels.topk_rows / topk_cosine, KeyIndex, the node models at
retrieve_num = num_class + 1 > 64 and with noise, the few-shot retrieve, and the error paths.  Every comparison is
bit-exact against the CPU oracle (oracle/cref.py), which takes any k."""

import numpy as np
import pytest
import torch

from oracle import cref, pipeline

pytestmark = pytest.mark.gpu

INT64_MAX = np.iinfo(np.int64).max


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(got, want):
    """(scores, idx) pairs equal bit for bit."""
    gs, gi = (x.cpu().numpy() if torch.is_tensor(x) else x for x in got)
    ws, wi = want
    assert gs.shape == ws.shape and gi.shape == wi.shape
    assert np.array_equal(gi, wi)
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32))


# ---- 1. kernels.topk_rows vs cref.topk_rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,k", [(3, 65, 65), (7, 1000, 65), (5, 5000, 256), (4, 4096, 4096), (9, 70001, 1000),
                                   (2, 300001, 4096), (3, 1048576, 128)])
def test_topk_rows_random(dev, B, N, k):
    from ragraph_amd import kernels as K

    S = np.random.default_rng(B * 7 + k).standard_normal((B, N)).astype(np.float32)
    _same(K.topk_rows(T(S, dev), k), cref.topk_rows(S, k))


def test_topk_rows_strided_slice(dev):
    """ld > N through the C entry (short rows, and chunked rows with an odd ld: unaligned rows, scalar loads)."""
    from ragraph_amd import _native as N_

    L = N_.lib()
    for B, Nn, ld, k in ((6, 3000, 3077, 300), (3, 70000, 70003, 700)):
        full = np.random.default_rng(Nn).standard_normal((B, ld)).astype(np.float32)
        S = T(full, dev)
        out_s = torch.empty((B, k), dtype=torch.float32, device=dev)
        out_i = torch.empty((B, k), dtype=torch.int64, device=dev)
        nbytes = L.ragraph_topk_rows_large_workspace_bytes(B, Nn, k)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        rc = L.ragraph_topk_rows_large_f32(S.data_ptr(), B, Nn, ld, k, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(),
                                           ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == N_.OK, N_.last_error()
        _same((out_s, out_i), cref.topk_rows(full[:, :Nn], k))


@pytest.mark.parametrize("N,k", [(3000, 1000), (5000, 100), (200000, 4096), (200000, 65)])
def test_topk_rows_heavy_ties(dev, N, k):
    """Scores quantised to 8 levels and constant rows: the digit refinement and the ordered tie ranks."""
    from ragraph_amd import kernels as K

    rng = np.random.default_rng(N + k)
    S = np.floor(rng.random((4, N)) * 8).astype(np.float32) - 4.0
    S[2] = 0.5     # constant row
    S[3, ::2] = 1.0  # half the row ties at the top
    _same(K.topk_rows(T(S, dev), k), cref.topk_rows(S, k))


@pytest.mark.parametrize("N,k", [(6000, 100), (100000, 300)])
def test_topk_rows_special_values(dev, N, k):
    """+-0 are one score (a tie), -inf is an ordinary score, NaN is never selected: rows short of k other scores pad with
    (-inf, INT64_MAX) as the oracle does."""
    from ragraph_amd import kernels as K

    rng = np.random.default_rng(N)
    pool = np.array([0.0, -0.0, -np.inf, np.nan, 1.0, -1.0, np.inf], dtype=np.float32)
    S = pool[rng.integers(0, len(pool), (5, N))]
    S[1] = np.nan
    S[1, rng.choice(N, k // 2, replace=False)] = rng.standard_normal(k // 2).astype(np.float32)   # fewer than k
    S[2] = np.nan                                                                                  # nothing at all
    S[3] = np.where(rng.random(N) < 0.5, np.float32(0.0), np.float32(-0.0))                       # only +-0
    S[4, : N // 2] = -np.inf
    S[4, N // 2:] = np.nan                                                                         # -inf and NaN
    want = cref.topk_rows(S, k)
    assert (want[1][2] == INT64_MAX).all() and (want[1][1][k // 2:] == INT64_MAX).all()
    _same(K.topk_rows(T(S, dev), k), want)


# ---- 2. kernels.topk_cosine vs cref.topk_cosine -----------------------------------------------------------------------
def _bank(n, D, seed, dev):
    from ragraph_amd import kernels as K

    g = torch.Generator(device=dev).manual_seed(seed)
    kn = K.normalize_rows(torch.randn(n, D, device=dev, generator=g))
    q = torch.randn(8, D, device=dev, generator=g)
    return q, kn


@pytest.mark.parametrize("n,D,k", [(5000, D, k) for D in (64, 100, 256) for k in (65, 100, 512, 4096)]
                         + [(200000, 64, 65), (200000, 100, 512), (200000, 256, 4096)])
def test_topk_cosine_large_k(dev, n, D, k):
    from ragraph_amd import kernels as K

    q, kn = _bank(n, D, n + D + k, dev)
    _same(K.topk_cosine(q, kn, k), cref.topk_cosine(q.cpu().numpy(), kn.cpu().numpy(), k))


def test_topk_cosine_idx_base_and_1m_bank(dev):
    from ragraph_amd import kernels as K

    q, kn = _bank(5000, 256, 3, dev)
    _same(K.topk_cosine(q, kn, 300, idx_base=1000), cref.topk_cosine(q.cpu().numpy(), kn.cpu().numpy(), 300, 1000))
    g = torch.Generator(device=dev).manual_seed(11)
    kn = K.normalize_rows(torch.randn(1 << 20, 256, device=dev, generator=g))
    q = torch.randn(64, 256, device=dev, generator=g)
    _same(K.topk_cosine(q, kn, 128), cref.topk_cosine(q.cpu().numpy(), kn.cpu().numpy(), 128))


def test_topk_cosine_large_k_above_key_chunk(dev):
    """8 M keys (two key chunks of the slab path, G * k > 4096): the per-chunk lists are merged by the large-k kernel."""
    from ragraph_amd import kernels as K

    g = torch.Generator(device=dev).manual_seed(5)
    kn = K.normalize_rows(torch.randn(8 << 20, 64, device=dev, generator=g))
    q = torch.randn(2, 64, device=dev, generator=g)
    got = K.topk_cosine(q, kn, 256)
    want = cref.topk_cosine(q.cpu().numpy(), kn.cpu().numpy(), 256)
    del kn
    _same(got, want)


# ---- 3. ToyGraphBase / KeyIndex on a bank of duplicate rows -----------------------------------------------------------
def _dup_bank(dev, C=5):
    rng = np.random.default_rng(21)
    base = rng.standard_normal((1500, 256)).astype(np.float32)
    keys = base[rng.integers(0, 1500, 6000)]                  # ~4x duplicates, shuffled
    values = rng.standard_normal((6000, 256)).astype(np.float32)
    labels = np.eye(C, dtype=np.float32)[rng.integers(0, C, 6000)]
    return keys, values, labels


def test_toy_graph_base_large_k_on_duplicate_bank(dev):
    from ragraph_amd.ragraph_utils import ToyGraphBase

    keys, values, labels = _dup_bank(dev)
    Q = np.random.default_rng(2).standard_normal((40, 256)).astype(np.float32)

    def fresh():
        tgb = ToyGraphBase(None, labels.shape[1], 256, 3, device=dev)
        tgb.add_resources(T(keys, dev), T(values, dev), T(labels, dev))
        return tgb

    tgb = fresh()
    _same(tgb.topk(T(Q, dev), 100), cref.topk_cosine(Q, cref.normalize_rows(keys), 100))
    # a large-k call leaves the index as it was: k = 10, 100, 10 behaves as a fresh index's k = 10, 10
    a, b = fresh(), fresh()
    a1 = a.topk(T(Q, dev), 10)
    a.topk(T(Q, dev), 100)
    a2 = a.topk(T(Q, dev), 10)
    b1 = b.topk(T(Q, dev), 10)
    b2 = b.topk(T(Q, dev), 10)
    for x, y in ((a1, b1), (a2, b2)):
        _same(x, (y[0].cpu().numpy(), y[1].cpu().numpy()))
    pa, pb = a._index.last_prior, b._index.last_prior
    assert (pa is None and pb is None) or (torch.is_tensor(pa) and torch.equal(pa, pb)) or pa == pb
    assert a._index._queries == b._index._queries


def test_toy_graph_base_large_k_on_padded_width(dev):
    """A bank of D = 100 is kept zero-padded to 128 columns by KeyIndex: the large-k route pads the queries too and
    scores the padded bank -- the same bits as the oracle on the unpadded rows."""
    from ragraph_amd.ragraph_utils import ToyGraphBase

    rng = np.random.default_rng(8)
    keys = rng.standard_normal((7000, 100)).astype(np.float32)
    Q = rng.standard_normal((33, 100)).astype(np.float32)
    tgb = ToyGraphBase(None, 4, 100, 3, device=dev)
    tgb.add_resources(T(keys, dev), T(rng.standard_normal((7000, 100)).astype(np.float32), dev),
                      T(np.eye(4, dtype=np.float32)[rng.integers(0, 4, 7000)], dev))
    for k in (65, 700):
        _same(tgb.topk(T(Q, dev), k), cref.topk_cosine(Q, cref.normalize_rows(keys), k))
    assert tgb._index.keys_normalized.shape[1] == 128


# ---- 4/5. node models at retrieve_num > 64 and with noise ---------------------------------------------------------------
def _node_setup(dev, C, n=2500, F=30, M=6000, seed=0, noise=False):
    # (F = 30: the encoder keeps the reference's association, pipeline.aggregate_first_applies)
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph import RAGraph

    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    pre = PrePrompt(F, 256, "prelu", 1, 0.3).to(dev)
    model = RAGraph(pre, None, F, C, 256, finetune=True, noise_finetune=noise, device=dev)
    keys = rng.standard_normal((M, 256)).astype(np.float32)
    values = rng.standard_normal((M, 256)).astype(np.float32)
    labels = np.eye(C, dtype=np.float32)[rng.integers(0, C, M)]
    model.toy_graph_base.add_resources(T(keys, dev), T(values, dev), T(labels, dev))
    X = rng.random((n, F)).astype(np.float32)
    a = rng.random((n, n)) < 3.0 / n
    adj = ((a | a.T) | np.eye(n, dtype=bool)).astype(np.float32)
    return model, pre, keys, values, labels, X, adj


def _params(model, pre):
    conv, dec = pre.gcn.convs[0], model.decoder
    c = lambda t: t.detach().cpu().numpy()
    return {"W": c(conv.fc.weight), "bias": c(conv.bias), "alpha": c(conv.act.weight)[0], "fc1_w": c(dec.fc1.weight),
            "fc1_b": c(dec.fc1.bias), "fc2_w": c(dec.fc2.weight), "fc2_b": c(dec.fc2.bias)}


def test_node_forward_70_classes_and_capture(dev):
    from ragraph_amd.capture import CapturedForward

    model, pre, keys, values, labels, X, adj = _node_setup(dev, 70)
    tgb = model.toy_graph_base
    assert tgb.retrieve_num == 71
    model.eval()
    Xd, adjd = T(X, dev), T(adj, dev)
    with torch.no_grad():
        logits = model(Xd, adjd)
        h = pre.inference(Xd, adjd)
        _, idx = tgb.topk(h, 71)
    # vs the oracle's restatement of RAGraph.forward (as test_node_forward_g6): encoder output and indices exact,
    # logits to expf rounding
    ol, oi, oh = pipeline.node_forward(X, cref.dense_to_csr(adj), _params(model, pre), keys, values, labels, 71,
                                       model.query_graph_hop, 0.5, 0.5)
    assert np.array_equal(h.cpu().numpy(), oh) and np.array_equal(idx.cpu().numpy(), oi)
    assert np.allclose(logits.cpu().numpy(), ol, atol=1e-6)
    from ragraph_amd.graph import as_csr

    g = as_csr(adjd)   # (the dense -> CSR conversion is not capturable: built once, as callers of CapturedForward do)
    _ = g.row_normalized_values()
    with torch.no_grad():
        want = model(Xd, g)
    assert torch.equal(want, logits)
    fwd = CapturedForward(lambda x: model(x, g), Xd)
    assert torch.equal(fwd(Xd), logits)


def test_noise_finetune_40_classes(dev):
    import torch.nn.functional as F_

    model, pre, keys, values, labels, X, adj = _node_setup(dev, 40, noise=True, seed=1)
    tgb = model.toy_graph_base
    assert tgb.retrieve_num == 41
    Xd, adjd = T(X, dev), T(adj, dev)
    with torch.no_grad():
        h = pre.inference(Xd, adjd)
        idx = tgb.retrieve_indices(h, add_noise=True)
    _, oi = cref.topk_cosine(h.cpu().numpy(), cref.normalize_rows(keys), 82)
    assert np.array_equal(idx[:, :82].cpu().numpy(), oi)
    model.train()
    out = model(Xd, adjd)
    loss = F_.cross_entropy(out, torch.from_numpy(labels[: X.shape[0]].argmax(1)).to(dev))
    loss.backward()
    assert torch.isfinite(loss)
    grads = [p.grad for p in model.decoder.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and any(g.abs().sum() > 0 for g in grads)


# ---- 6. few-shot node flavour: retrieve_num = 40 with noise -> topk_rows at k = 80 ------------------------------------------
def test_fewshot_retrieve_large_k(dev):
    from ragraph_amd import kernels as K
    from ragraph_amd.RAGraph_fewshot import ToyGraphBaseFewShot

    rng = np.random.default_rng(6)
    n, M, C = 300, 5000, 7
    tgb = ToyGraphBaseFewShot(None, C, 256, 3, retrieve_num=40, device=dev)
    values = rng.standard_normal((M, 256)).astype(np.float32)
    tgb.add_resources(T(rng.standard_normal((M, 256)).astype(np.float32), dev), T(values, dev),
                      T(np.eye(C, dtype=np.float32)[rng.integers(0, C, M)], dev),
                      T(rng.random((M, 10)).astype(np.float32), dev))
    a = rng.random((n, n)) < 4.0 / n
    adj = T(((a | a.T) | np.eye(n, dtype=bool)).astype(np.float32), dev)
    q = T(rng.standard_normal((n, 256)).astype(np.float32), dev)
    anchors = torch.randint(0, n, (10,))
    scores = tgb.similarity_scores(q, adj, anchors)
    want = cref.topk_rows(scores.cpu().numpy(), 80)
    _same(K.topk_rows(scores, 80), want)
    emb, _ = tgb.retrieve(q, adj, True, anchors)
    assert emb.shape[1] == 80 + tgb.noise_retrieve_num
    assert np.array_equal(emb[:, :80].cpu().numpy(), values[want[1]])


# ---- 7. errors --------------------------------------------------------------------------------------------------------
def test_large_k_errors(dev):
    from ragraph_amd import _native as N_
    from ragraph_amd import kernels as K
    from ragraph_amd._native import RagraphNativeError

    S = torch.randn(3, 5000, device=dev)
    with pytest.raises(RagraphNativeError):
        K.topk_rows(S, 4097)
    with pytest.raises(RagraphNativeError):
        K.topk_rows(S[:, :100].contiguous(), 101)
    with pytest.raises(RagraphNativeError):
        K.topk_cosine(torch.randn(2, 64, device=dev), K.normalize_rows(torch.randn(5000, 64, device=dev)), 4097)
    L = N_.lib()
    out_s = torch.full((3, 4097), 7.0, device=dev)
    out_i = torch.full((3, 4097), -5, dtype=torch.int64, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    rc = L.ragraph_topk_rows_large_f32(S.data_ptr(), 3, 5000, 5000, 4097, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(),
                                       ws.numel(), st)
    assert rc == N_.EUNSUPPORTED
    rc = L.ragraph_topk_rows_large_f32(S.data_ptr(), 3, 100, 5000, 101, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(),
                                       ws.numel(), st)
    assert rc == N_.EINVAL
    torch.cuda.synchronize()
    assert (out_s == 7.0).all() and (out_i == -5).all()
