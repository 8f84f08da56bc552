"""Noisy fine-tuning with the noise drawn on the device (csrc/noise.hip, noise_rng = "device"): the noise rows against the
Python restatement of the hash (tests/noise_oracle.py) bit for bit, the fused noisy gather-reduce against gather_reduce over
cat(idx, noise rows) bit for bit, the Gaussian source's contracts and moments, every flavour's noisy training forward against
the unfused composition from `last_noise_seed`, the edge flavour's forward_rows / cal_loss without a host draw, the captured
noisy step, and the error paths."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import noise_oracle as O

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF


def _seed(dev, value=SEED):
    return torch.tensor([value], dtype=torch.int64, device=dev)


# ---- noise rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("B", [0, 1, 5, 257])
def test_noise_rows_match_the_python_oracle(dev, B, m):
    from ragraph_amd import kernels as K

    pat = [(1 << 33) + 5, 10, 31, 10, 2]             # unsorted, with a repeat, an id above 2^32
    ids = [pat[b % 5] + b // 5 for b in range(B)]
    assert B < 5 or (len(set(ids)) < B and max(ids) > 1 << 32 and ids != sorted(ids))
    row_ids = torch.tensor(ids, dtype=torch.int64, device=dev)
    for n in (1, 7, 2 ** 40):
        got = K.noise_rows(_seed(dev), B, m, n, row_ids=row_ids)
        assert got.shape == (B, m) and got.dtype == torch.int64
        assert got.cpu().tolist() == O.noise_rows(SEED, ids, m, n)
        got = K.noise_rows(_seed(dev), B, m, n, row_base=1000)
        assert got.cpu().tolist() == O.noise_rows(SEED, range(1000, 1000 + B), m, n)
        # the tail columns of a prefilled [B, k + m] matrix, in place
        k = 4
        full = torch.full((B, k + m), -7, dtype=torch.int64, device=dev)
        K.noise_rows(_seed(dev), B, m, n, row_ids=row_ids, out=full[:, k:])
        assert bool((full[:, :k] == -7).all()) and full[:, k:].cpu().tolist() == O.noise_rows(SEED, ids, m, n)


def test_noise_entries_reject_bad_arguments_and_write_nothing(dev):
    from ragraph_amd import _native as N
    from ragraph_amd import kernels as K

    L = K._ready()
    seed = _seed(dev)
    out = torch.full((4, 3), -7, dtype=torch.int64, device=dev)
    p, s = out.data_ptr(), seed.data_ptr()
    for args in ((s, None, 0, 4, 3, 0, p, 3),      # N = 0
                 (s, None, 0, 4, 0, 10, p, 3),     # m = 0
                 (s, None, 0, 4, 3, 10, p, 2),     # out_stride < m
                 (None, None, 0, 4, 3, 10, p, 3)):  # null seed
        assert L.ragraph_noise_rows_i64(*args, None) == N.EINVAL
        assert N.last_error().startswith("noise_rows")
    v = torch.ones(10, 8, device=dev)
    idx = torch.zeros(4, 2, dtype=torch.int64, device=dev)
    o = torch.full((4, 8), -7.0, device=dev)
    gr = lambda sd, m, nn: L.ragraph_gather_reduce_noisy_f32(v.data_ptr(), 8, None, 0, 10, idx.data_ptr(), 4, 2, 0, 1.0, sd, None,
                                                             0, m, nn, None, 0.0, 0.0, o.data_ptr(), None, None)
    assert gr(None, 1, 10) == N.EINVAL and gr(s, 0, 10) == N.EINVAL and gr(s, 1, 0) == N.EINVAL
    an = lambda sd, J, D: L.ragraph_add_normal_noise_f32(None, 4, J, D, 0.01, sd, None, 0, o.data_ptr(), None)
    assert an(None, 1, 8) == N.EINVAL and an(s, 0, 8) == N.EINVAL and an(s, 1, 0) == N.EINVAL
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((o == -7.0).all())
    with pytest.raises(K.RagraphNativeError):
        K.noise_rows(seed, 4, 3, 0)


# ---- fused noisy gather-reduce -------------------------------------------------------------------------------------------
BANK = 300


def _bank(dev, D, C):
    g = torch.Generator(device=dev).manual_seed(100 + D)
    v = torch.randn(BANK, D, device=dev, generator=g)
    lab = F.one_hot(torch.randint(0, C, (BANK,), device=dev, generator=g), C).float() if C else None
    return v, lab, g


@pytest.mark.parametrize("D", [256, 64, 10])   # one float4 chunk per lane, a partly used wave, the scalar path
def test_gather_reduce_noisy_equals_gather_reduce_over_cat(dev, D):
    from ragraph_amd import kernels as K

    seed = _seed(dev)
    for C in (0, 7):
        v, lab, g = _bank(dev, D, C)
        for B in (1, 5):
            a = torch.randn(B, D, device=dev, generator=g)
            row_ids = torch.randint(0, 1 << 40, (B,), device=dev, generator=g)
            for k in (1, 8, 9, 65):
                idx = torch.randint(0, BANK, (B, k), device=dev, generator=g)
                for m in (1, 3):
                    for keys in (dict(row_ids=row_ids), dict(row_base=17)):
                        cat = torch.cat([idx, K.noise_rows(seed, B, m, BANK, **keys)], dim=1)
                        for v_scale in (1.0, 1.0 / (k + m)):
                            ref = K.gather_reduce(v, lab, cat, v_scale=v_scale)
                            got = K.gather_reduce_noisy(v, lab, idx, seed, m, v_scale=v_scale, **keys)
                            assert torch.equal(got[0], ref[0]), (C, B, k, m, v_scale)
                            assert (C == 0 and got[1] is None) or torch.equal(got[1], ref[1]), (C, B, k, m)
                        ref = K.gather_reduce_mix(v, lab, cat, a, 0.7, 0.3, v_scale=1.0 / (k + m))
                        got = K.gather_reduce_noisy(v, lab, idx, seed, m, v_scale=1.0 / (k + m), mix=(a, 0.7, 0.3), **keys)
                        assert torch.equal(got[0], ref[0]) and (C == 0 or torch.equal(got[1], ref[1])), (C, B, k, m, "mix")


@pytest.mark.parametrize("D", [256, 10])
def test_gather_reduce_noisy_shards_add_up(dev, D):
    """The bank cut in two at row 130: a shard adds +0 for the other's rows, listed or noise.  Values on a 2^-10 grid below 4
    and a power-of-two scale make every partial sum exact in fp32 (68 terms: 19 bits), so the shards' sums add up to the
    whole bit for bit; a label mean is three roundings of numbers <= 1 away: 4 * 2^-24."""
    from ragraph_amd import kernels as K

    C, cut, seed = 7, 130, _seed(dev)
    g = torch.Generator(device=dev).manual_seed(7)
    v = torch.randint(-4095, 4096, (BANK, D), device=dev, generator=g).float() / 1024
    lab = F.one_hot(torch.randint(0, C, (BANK,), device=dev, generator=g), C).float()
    for k, m in ((9, 3), (65, 3)):
        idx = torch.randint(0, BANK, (5, k), device=dev, generator=g)
        whole = K.gather_reduce_noisy(v, lab, idx, seed, m, v_scale=0.25, row_base=3)
        lo = K.gather_reduce_noisy(v[:cut].contiguous(), lab[:cut].contiguous(), idx, seed, m, noise_n=BANK, v_scale=0.25,
                                   row_base=3)
        hi = K.gather_reduce_noisy(v[cut:].contiguous(), lab[cut:].contiguous(), idx, seed, m, noise_n=BANK, v_scale=0.25,
                                   row_base=3, idx_base=cut)
        assert torch.equal(lo[0] + hi[0], whole[0])
        assert float((lo[1] + hi[1] - whole[1]).abs().max()) <= 4 * 2.0 ** -24
        noise = K.noise_rows(seed, 5, m, BANK, row_base=3)
        assert bool((noise < cut).any()) and bool((noise >= cut).any()), "the noise rows must fall on both shards"


# ---- Gaussian noise --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 6, 256), (3, 2, 10)])
def test_add_normal_noise(dev, shape):
    from ragraph_amd import kernels as K

    std, seed = 0.01, _seed(dev)
    x = torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    z = K.add_normal_noise(None, std, seed, shape=shape)
    out = K.add_normal_noise(x, std, seed)
    assert out.shape == shape and torch.equal(out, x + z)
    assert torch.equal(out, K.axpby(x, 1.0, z, 1.0))                       # the host mode's arithmetic on a materialised noise
    assert torch.equal(K.add_normal_noise(None, std, seed, shape=shape), z)
    assert not torch.equal(K.add_normal_noise(None, std, _seed(dev, SEED + 1), shape=shape), z)
    b = min(7, shape[0] - 1)
    one = K.add_normal_noise(x[b:b + 1].contiguous(), std, seed, row_ids=torch.tensor([b], device=dev))
    assert torch.equal(one[0], out[b])
    assert torch.equal(K.add_normal_noise(x[b:b + 1].contiguous(), std, seed, row_base=b)[0], out[b])
    # in place: out may alias X
    y = x.clone()
    L = K._ready()
    assert L.ragraph_add_normal_noise_f32(y.data_ptr(), shape[0], shape[1], shape[2], std, seed.data_ptr(), None, 0,
                                          y.data_ptr(), None) == 0
    assert torch.equal(y, out)
    zs = (z.double() / std).flatten()
    n = zs.numel()
    assert bool(torch.isfinite(zs).all())
    assert float(zs.abs().max()) <= 5.78
    if n >= 50_000:   # (the moments need the large shape: 56 832 values)
        mean, var = float(zs.mean()), float(zs.var(unbiased=False))
        print(f"n {n}: mean {mean:.5f} var {var:.5f} max |z| {float(zs.abs().max()):.3f}")
        assert abs(mean) < 5 / math.sqrt(n)
        assert abs(var - 1) < 5 * math.sqrt(2 / n)


# ---- node flavour ----------------------------------------------------------------------------------------------------------
def _node_setup(dev, C=70, n=300, F_in=30, M=600, seed=0):
    """tests/test_gpu_topk_large.py's _node_setup (k' = 2 * 71 = 142 listed rows: three index blocks) at 300 nodes and a
    600-row bank, noisy fine-tuning with the noise on the device."""
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph import RAGraph

    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    pre = PrePrompt(F_in, 256, "prelu", 1, 0.3).to(dev)
    model = RAGraph(pre, None, F_in, C, 256, finetune=True, noise_finetune=True, device=dev)
    T = lambda a: torch.from_numpy(a).to(dev)
    model.toy_graph_base.add_resources(T(rng.standard_normal((M, 256)).astype(np.float32)),
                                       T(rng.standard_normal((M, 256)).astype(np.float32)),
                                       T(np.eye(C, dtype=np.float32)[rng.integers(0, C, M)]))
    X = rng.random((n, F_in)).astype(np.float32)
    a = rng.random((n, n)) < 3.0 / n
    adj = ((a | a.T) | np.eye(n, dtype=bool)).astype(np.float32)
    model.toy_graph_base.noise_rng = "device"
    return model.train(), T(X), T(adj)


def test_node_noisy_forward_equals_unfused_composition(dev, monkeypatch):
    from ragraph_amd import kernels as K

    model, X, adj = _node_setup(dev)
    tgb = model.toy_graph_base
    assert tgb.noise_rng == "device" and tgb.retrieve_num == 71
    torch.manual_seed(21)
    out = model(X, adj).detach().clone()
    seed = tgb.last_noise_seed.clone()
    assert seed.is_cuda and seed.dtype == torch.int64 and 0 <= int(seed) < 2 ** 62
    torch.manual_seed(21)
    assert torch.equal(model(X, adj).detach(), out) and torch.equal(tgb.last_noise_seed, seed)
    torch.manual_seed(22)
    other = model(X, adj).detach()
    assert not torch.equal(tgb.last_noise_seed, seed) and not torch.equal(other, out)
    # retrieve_indices in device mode: the top-k' columns, then the oracle's rows of its own fresh seed
    q = model.pretrain_model.inference(X, adj)
    idx = tgb.retrieve_indices(q, True)
    assert idx.shape == (X.shape[0], 2 * 71 + 1) and torch.equal(idx[:, :142], tgb.topk(q, 142)[1])
    assert idx[:, 142:].cpu().tolist() == O.noise_rows(int(tgb.last_noise_seed), range(X.shape[0]), 1, 600)
    # a caller that holds a slice of the batch keys it by the rows' places in the batch
    part = tgb.retrieve_indices(q[100:110].contiguous(), True, row_base=100)
    assert part[:, 142:].cpu().tolist() == O.noise_rows(int(tgb.last_noise_seed), range(100, 110), 1, 600)

    def unfused(queries, **kw):   # top-k, noise_rows of the first forward's seed, the plain gather_reduce
        _, top = tgb.topk(queries, 2 * tgb.retrieve_num)
        noise = K.noise_rows(seed, top.shape[0], tgb.noise_retrieve_num, tgb.resource_values.shape[0])
        return K.gather_reduce(tgb.resource_values, tgb.resource_labels, torch.cat([top, noise], dim=1))

    monkeypatch.setattr(tgb, "retrieve_reduced_noisy", unfused)
    assert torch.equal(model(X, adj).detach(), out)


# ---- few-shot flavours -----------------------------------------------------------------------------------------------------
def _tu_batch(dev, F_in, num_graphs, seed):
    from ragraph_amd.data import DataLoader, synthetic_tu_dataset
    from ragraph_amd.ragraph_utils import process_tu_dataset

    ds = synthetic_tu_dataset(num_graphs=num_graphs, num_node_attributes=F_in, num_node_labels=3, seed=seed)
    feats, adj, _ = process_tu_dataset(next(iter(DataLoader(ds, batch_size=num_graphs))), F_in, device=dev)
    return feats, adj


def test_node_fewshot_noisy_forward_equals_unfused_composition(dev, monkeypatch):
    from ragraph_amd import kernels as K
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph_fewshot import RAGraph as RAGraphFewShot

    F_in, C, D = 18, 3, 256
    feats, adj = _tu_batch(dev, F_in, 4, 8)
    gen = torch.Generator(device=dev).manual_seed(4)
    bank = (F.normalize(torch.randn(600, D, device=dev, generator=gen), dim=-1), torch.randn(600, D, device=dev, generator=gen),
            F.one_hot(torch.randint(0, C, (600,), device=dev, generator=gen), C).float(),
            torch.rand(600, 10, device=dev, generator=gen))
    anchors = torch.randint(0, feats.shape[0], (10,), device=dev, generator=gen)
    mean = torch.randn(C, D, device=dev, generator=gen)
    torch.manual_seed(12)
    model = RAGraphFewShot(PrePrompt(F_in, D, "prelu", 2, 0.3).to(dev), None, torch.zeros(C, D, device=dev), D,
                           noise_finetune=True, device=dev, dataset_name="ENZYMES").train()
    tgb = model.toy_graph_base
    tgb.add_resources(*bank)
    tgb.noise_rng = "device"
    torch.manual_seed(5)
    out = model(feats, adj, mean, anchors=anchors).detach().clone()
    seed = int(tgb.last_noise_seed)

    def unfused(search_keys, search_adj, add_noise, anchors=None):   # the oracle's rows behind the top-2k, gathered and joined
        assert add_noise
        _, idx = tgb.topk(search_keys, 2 * tgb.retrieve_num, tgb.search_positions(search_adj, None, anchors))
        noise = torch.tensor(O.noise_rows(seed, range(idx.shape[0]), tgb.noise_retrieve_num, 600), device=dev)
        idx = torch.cat([idx, noise], dim=1)
        return K.gather_rows(tgb.resource_values, idx), K.gather_rows(tgb.resource_labels, idx)

    monkeypatch.setattr(tgb, "retrieve", unfused)
    assert torch.equal(model(feats, adj, mean, anchors=anchors).detach(), out)


def test_graph_fewshot_noisy_forward_equals_unfused_composition(dev, monkeypatch):
    from ragraph_amd import kernels as K
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph_fewshot import RAGraphGraphFewShot

    F_in, C, D = 18, 2, 256
    feats, adj = _tu_batch(dev, F_in, 1, 30)
    gen = torch.Generator(device=dev).manual_seed(31)
    bank = (F.normalize(torch.randn(800, D, device=dev, generator=gen), dim=-1), torch.randn(800, D, device=dev, generator=gen),
            F.one_hot(torch.randint(0, C, (800,), device=dev, generator=gen), C).float())
    mean = torch.randn(C, D, device=dev, generator=gen)
    torch.manual_seed(13)
    model = RAGraphGraphFewShot(PrePrompt(F_in, D, "prelu", 2, 0.3).to(dev), None, F_in, C, D, noise_finetune=True, device=dev,
                                dataset_name="PROTEINS").train()
    tgb = model.toy_graph_base
    tgb.add_resources(*bank)
    tgb.noise_rng = "device"
    torch.manual_seed(6)
    out = model(feats, adj, mean).detach().clone()
    seed = tgb.last_noise_seed.clone()
    torch.manual_seed(6)
    assert torch.equal(model(feats, adj, mean).detach(), out)

    def unfused(search_keys, search_adj, add_noise, idx=None, **kw):   # the noise materialised, then today's axpby
        assert add_noise and idx is not None
        emb = K.gather_rows(tgb.resource_values, idx)
        z = K.add_normal_noise(None, tgb.noise_std, seed, shape=emb.shape)
        assert float(z.abs().max()) > 0 and float(z.abs().max()) <= 6 * tgb.noise_std
        return K.axpby(emb, 1.0, z, 1.0), K.gather_rows(tgb.resource_labels, idx)

    monkeypatch.setattr(tgb, "retrieve", unfused)
    assert torch.equal(model(feats, adj, mean).detach(), out)


# ---- edge flavour ----------------------------------------------------------------------------------------------------------
U, I, DE = 300, 200, 64
USER_ROWS = [7, 299, 7, 0, 150, 151, 150, 42, 7]          # repeated, unsorted
ITEM_ROWS = [199, 3, 3, 0, 77, 199, 120]


def _edge_model(dev, **kw):
    """tests/test_gpu_edge_rows.py's model."""
    from ragraph_amd.data import synthetic_bipartite
    from ragraph_amd.RAGraph_edge import RAGraph

    edges, norm, times = synthetic_bipartite(U, I, edges_per_user=6, seed=12, device=dev)

    class DS:
        num_users, num_items = U, I
    DS.edges, DS.edge_norm, DS.edge_times = edges, norm, times

    class Pre:
        def generate(self):
            g = torch.Generator(device=dev).manual_seed(5)
            return 0.1 * torch.randn(U, DE, device=dev, generator=g), 0.1 * torch.randn(I, DE, device=dev, generator=g)

    torch.manual_seed(3)
    m = RAGraph(DS, Pre(), device=dev, **kw).train()
    m.noise_rng = "device"
    return m


@pytest.fixture
def no_host_randint(monkeypatch):
    real = torch.randint

    def guarded(*a, **kw):
        if torch.device(kw.get("device") or "cpu").type == "cpu":
            raise AssertionError("torch.randint on the CPU during a noise_rng = 'device' step")
        return real(*a, **kw)

    monkeypatch.setattr(torch, "randint", guarded)


def test_edge_forward_rows_equals_forward_finetune_noise(dev, no_host_randint, monkeypatch):
    from ragraph_amd import kernels as K

    m = _edge_model(dev, phase="finetune", use_RAG=True, use_noise=True, retrieve_num=5)
    ur, ir = torch.tensor(USER_ROWS, device=dev), torch.tensor(ITEM_ROWS, device=dev)
    args = (m.edges, m.edge_norm, m.edge_times)
    for grad in (False, True):
        with torch.set_grad_enabled(grad):
            torch.manual_seed(11)
            uo, io = m.forward(*args)
            seed = m.last_noise_seed.clone()
            torch.manual_seed(11)
            us, is_ = m.forward_rows(*args, ur, ir)
            assert torch.equal(m.last_noise_seed, seed)
        assert us.shape == (len(USER_ROWS), DE) and is_.shape == (len(ITEM_ROWS), DE)
        assert torch.equal(us.detach(), uo.detach()[ur]) and torch.equal(is_.detach(), io.detach()[ir])
    # the forward against the unfused composition: the noise rows of the global node ids behind the top-k, one plain mean
    real = K.gather_reduce_noisy

    def unfused(v, labels, idx, sd, n_noise, **kw):
        cat = torch.cat([idx, K.noise_rows(sd, idx.shape[0], n_noise, v.shape[0], kw.get("row_ids"), kw.get("row_base", 0))], 1)
        assert cat.shape[1] == 5 + 1 + 1 and kw["v_scale"] == 1.0 / cat.shape[1]
        return K.gather_reduce(v, labels, cat, v_scale=kw["v_scale"])

    monkeypatch.setattr(K, "gather_reduce_noisy", unfused)
    with torch.no_grad():
        torch.manual_seed(11)
        u2, i2 = m.forward(*args)
    monkeypatch.setattr(K, "gather_reduce_noisy", real)
    assert torch.equal(u2, uo.detach()) and torch.equal(i2, io.detach())
    with torch.no_grad():                            # the noise really is drawn per call: another seed, other rows
        torch.manual_seed(12)
        assert not torch.equal(m.forward_rows(*args, ur, ir)[0], us.detach())


def test_edge_cal_loss_noise_device_batch_rows_equals_all_rows(dev, no_host_randint):
    m = _edge_model(dev, phase="finetune", use_RAG=True, use_noise=True, retrieve_num=5)
    users = (torch.arange(64) * 37) % U              # (made from ranges: no randint on the host in this test at all)
    pos, neg = (torch.arange(64) * 11) % I, (torch.arange(64) * 29 + 5) % I
    users[5] = users[9] = users[0]                   # repeated users
    neg[3] = pos[17]                                 # an item that is a positive and a negative
    out = {}
    for mode in ("all", "batch"):
        m.loss_rows = mode
        m.zero_grad(set_to_none=True)
        torch.manual_seed(8)
        loss, parts = m.cal_loss((users, pos, neg))
        loss.backward()
        out[mode] = (loss.detach().clone(), parts, m.last_noise_seed.clone())
    assert torch.equal(out["all"][0], out["batch"][0]) and out["all"][1] == out["batch"][1]
    assert torch.equal(out["all"][2], out["batch"][2])
    assert all(p.grad is not None for p in (m.user_embedding, m.item_embedding, m.gating_weight))


# ---- capture ---------------------------------------------------------------------------------------------------------------
def _node528(dev):
    """tests/test_gpu_capture_train.py's make(noise=True) model (the node_528 shape)."""
    from ragraph_amd.data import DataLoader, synthetic_tu_dataset
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph import RAGraph
    from ragraph_amd.ragraph_utils import process_tu_dataset

    F_in, C, D, N = 18, 3, 256, 20_000
    ds = synthetic_tu_dataset(num_graphs=16, num_node_attributes=F_in, num_node_labels=C, seed=21)
    feats, adj, _ = process_tu_dataset(next(iter(DataLoader(ds, batch_size=16))), F_in, device=dev)
    _ = adj.row_normalized_values()
    n = feats.shape[0]
    gen = torch.Generator(device=dev).manual_seed(74)
    keys = F.normalize(torch.randn(N, D, device=dev, generator=gen), dim=-1)
    vals = torch.randn(N, D, device=dev, generator=gen)
    labs = F.one_hot(torch.randint(0, C, (N,), device=dev, generator=gen), C).float()
    labels = torch.randint(0, C, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(75))

    def make(noise_rng):
        torch.manual_seed(5)
        model = RAGraph(PrePrompt(F_in, D, "prelu", 1, 0.3).to(dev), None, F_in, C, D, finetune=True, noise_finetune=True,
                        device=dev)
        model.toy_graph_base.add_resources(keys, vals, labs)
        model.toy_graph_base.noise_rng = noise_rng
        model.train()
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3, capturable=True)

        def step(x, y):   # RAGraph_node/finetune-rag.py:77-84
            return F.cross_entropy(model(x, adj), y)
        return model, step, opt

    return make, feats, labels


def test_noisy_node_step_captures_with_device_noise(dev, monkeypatch):
    from ragraph_amd.capture import CapturedTrainStep
    from ragraph_amd.kernels import RagraphNativeError

    make, feats, labels = _node528(dev)
    model, step, opt = make("device")
    cap = CapturedTrainStep(step, opt, feats, labels)
    tgb = model.toy_graph_base
    cap(feats, labels)
    seed1 = tgb.last_noise_seed.clone()
    before = [p.detach().clone() for p in model.parameters()]
    loss2 = cap(feats, labels).clone()
    seed2 = tgb.last_noise_seed.clone()
    print(f"seeds of two replays: {int(seed1)} {int(seed2)}")
    assert not torch.equal(seed1, seed2), "a replay must draw a new seed"
    # the replayed step, recomputed eagerly from the parameters before it and its seed
    twin, step_t, _ = make("device")
    with torch.no_grad():
        for p, b in zip(twin.parameters(), before):
            p.copy_(b)
    monkeypatch.setattr(twin.toy_graph_base, "_draw_noise_seed", lambda: seed2)
    assert torch.equal(step_t(feats, labels).detach(), loss2)
    # the reference's host draws still cannot be captured
    model_h, step_h, opt_h = make("host")
    with pytest.raises(RagraphNativeError, match="noise"):
        CapturedTrainStep(step_h, opt_h, feats, labels)
