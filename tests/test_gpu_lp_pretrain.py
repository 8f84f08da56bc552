"""Link-prediction pre-training on the device: PrePrompt.forward / backward against the reference's own step (g18, both
flavours), the compare loss against the reference's torch op chain (duplicates, self partners, an isolated node, a hub
target, a zero row, two layers with dropout), determinism, the sampler's rules, memory and a short pre-training run."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g18_lp_pretrain.npz")
T = 1.5


def _ref_compareloss(feature, tuples, temperature=T):
    """preprompt.py:72-103 as torch ops (mygather + F.cosine_similarity + the exp / log chain)."""
    n, S = tuples.shape
    D = feature.shape[1]
    h_t = torch.gather(feature, 0, tuples.reshape(-1, 1).expand(-1, D)).reshape(n, S, D)
    own = torch.arange(n, device=feature.device).reshape(-1, 1).expand(n, S)
    h_i = torch.gather(feature, 0, own.reshape(-1, 1).expand(-1, D)).reshape(n, S, D)
    sim = F.cosine_similarity(h_i, h_t, dim=2)
    e = (torch.exp(sim) / temperature).permute(1, 0)
    num = e[0].reshape(-1, 1)
    den = e[1:].permute(1, 0).sum(dim=1, keepdim=True)
    return (-1 * torch.log(num / den)).mean()


def _random_graph(dev, n, deg, seed, isolated=(), self_loops=False):
    from ragraph_amd.graph import CSRGraph
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, n, (n * deg // 2,), generator=g)
    c = torch.randint(0, n, (n * deg // 2,), generator=g)
    a = torch.zeros(n, n)
    a[r, c] = 1.0
    a[c, r] = 1.0
    a.fill_diagonal_(1.0 if self_loops else 0.0)
    for i in isolated:
        a[i, :] = 0.0
        a[:, i] = 0.0
    return CSRGraph.from_dense(a.to(dev)), a


def _ref_model(F_in, D, layers, p, dev, seed):
    from ragraph_amd.preprompt import PrePrompt
    torch.manual_seed(seed)
    m = PrePrompt(F_in, D, "prelu", layers, p).to(dev)
    with torch.no_grad():
        for conv, bn in zip(m.gcn.convs, m.gcn.bns):
            conv.bias.normal_(0.0, 0.1)
            conv.act.weight.fill_(0.2)
            bn.weight.normal_(1.0, 0.1)
            bn.bias.normal_(0.0, 0.1)
    return m


def _torch_encoder(model, X, adj_dense):
    """models/gcnlayers.py:40-67 (LP=True) + LP.py + layers/gcn.py as torch ops, with the model's own modules."""
    out = X
    for conv, bn in zip(model.gcn.convs, model.gcn.bns):
        z = torch.mm(adj_dense, out @ conv.fc.weight.t()) + conv.bias
        out = model.gcn.dropout(bn(conv.act(z)))
    return F.elu(out)


# ---- golden: the reference's own step ----------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["node", "graph"])
def test_forward_backward_matches_g18(dev, flavour):
    from ragraph_amd.graph import CSRGraph
    from ragraph_amd.preprompt import PrePrompt
    z = np.load(GOLDEN)
    g = lambda k: z[f"{flavour}_{k}"]  # noqa: E731
    n = g("X").shape[0]
    adj = CSRGraph(torch.from_numpy(g("adj_rowptr")).to(dev), torch.from_numpy(g("adj_col")).to(dev),
                   torch.from_numpy(g("adj_val")).to(dev), n)
    model = PrePrompt(18, 256, "prelu", 1, 0.0).to(dev)
    conv, bn = model.gcn.convs[0], model.gcn.bns[0]
    with torch.no_grad():
        conv.fc.weight.copy_(torch.from_numpy(g("W")))
        conv.bias.copy_(torch.from_numpy(g("bias")))
        conv.act.weight.copy_(torch.from_numpy(g("alpha")))
        bn.weight.copy_(torch.from_numpy(g("bn_weight")))
        bn.bias.copy_(torch.from_numpy(g("bn_bias")))
    X = torch.from_numpy(g("X")).to(dev)
    model.train()
    probe = copy.deepcopy(model)
    elu = F.elu(probe.gcn(X, adj, False, True).squeeze(0))
    # (A_hat X W^T is summed in another order than the reference's dense mm; BatchNorm's 1 / std scales that fp32 rounding
    # up to ~2e-6 on entries near 0, so the absolute slack here is 5e-6)
    np.testing.assert_allclose(elu.detach().cpu().numpy(), g("elu"), rtol=1e-4, atol=5e-6)
    loss = model(X[None], None, None, None, adj, None, None, False, None, None, None, lbl=None, sample=g("sample"))
    loss.backward()
    assert float(loss) == pytest.approx(float(g("loss")), rel=1e-5)
    for name, p in (("g_W", conv.fc.weight), ("g_bias", conv.bias), ("g_alpha", conv.act.weight),
                    ("g_bn_weight", bn.weight), ("g_bn_bias", bn.bias)):
        np.testing.assert_allclose(p.grad.cpu().numpy(), g(name), rtol=1e-4, atol=1e-6, err_msg=name)
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), g("bn_running_mean"), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), g("bn_running_var"), rtol=1e-4, atol=1e-6)


# ---- against the torch composition --------------------------------------------------------------------------------------
def _hard_case(dev, n=5000, n_neg=100, D=256):
    from ragraph_amd.preprompt import prompt_pretrain_sample
    adj, _ = _random_graph(dev, n, 6, seed=21, isolated=(11,))
    gen = torch.Generator(device=dev).manual_seed(3)
    t = prompt_pretrain_sample(adj, n_neg, generator=gen)
    t[:, 5] = t[:, 6]                                  # duplicate partners in every row
    t[::7, 9] = torch.arange(0, n, 7, device=dev)      # t[i, s] = i
    t[:, 2] = 7                                        # a hub target: 5000 transposed slots (+ its own)
    t[::3, 0] = 7
    assert int((t == 7).sum()) >= 5000
    torch.manual_seed(4)
    h = torch.randn(n, D, device=dev)
    h[3] = 0.0                                         # a zero row (also a partner of others)
    t[::5, 3] = 3
    return h, t


def test_compare_loss_matches_torch_chain(dev):
    from ragraph_amd.preprompt import compareloss
    h, t = _hard_case(dev)
    assert int(t[11, 0]) == 11                         # the isolated node's positive is itself
    h1 = h.clone().requires_grad_(True)
    h2 = h.clone().requires_grad_(True)
    l1 = compareloss(h1, t, T)
    l1.backward()
    l2 = _ref_compareloss(h2, t)
    l2.backward()
    assert float(l1) == pytest.approx(float(l2), rel=1e-5)
    assert torch.isfinite(h1.grad).all()
    rest = torch.ones(h.shape[0], dtype=torch.bool, device=dev)
    rest[3] = False
    scale = float(h2.grad[rest].abs().max())
    torch.testing.assert_close(h1.grad[rest], h2.grad[rest], rtol=1e-4, atol=1e-5 * scale)
    # the zero row: what autograd gives (the clamped norm's direct term only), and finite
    torch.testing.assert_close(h1.grad[3], h2.grad[3], rtol=1e-4, atol=1e-5 * float(h2.grad[3].abs().max()))


def test_two_layers_with_dropout_match_torch_composition(dev):
    n, F_in, D = 5000, 18, 256
    adj, a = _random_graph(dev, n, 6, seed=31, isolated=(5,), self_loops=True)
    deg = a.sum(1)
    dinv = deg.pow(-0.5)
    dinv[torch.isinf(dinv)] = 0
    a_hat = (dinv[:, None] * a * dinv[None, :]).to(dev)
    from ragraph_amd.graph import CSRGraph
    adj = CSRGraph.from_dense(a_hat)
    from ragraph_amd.preprompt import prompt_pretrain_sample
    t = prompt_pretrain_sample(adj, 100, generator=torch.Generator(device=dev).manual_seed(8))
    model = _ref_model(F_in, D, 2, 0.3, dev, seed=9)
    ref = copy.deepcopy(model)
    X = torch.rand(n, F_in, generator=torch.Generator().manual_seed(10)).to(dev)
    model.train()
    ref.train()
    torch.manual_seed(123)
    loss = model(X[None], None, None, None, adj, None, None, False, None, None, None, lbl=None, sample=t)
    loss.backward()
    torch.manual_seed(123)
    rloss = _ref_compareloss(_torch_encoder(ref, X, a_hat), t)
    rloss.backward()
    assert float(loss) == pytest.approx(float(rloss), rel=1e-5)
    for (name, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-3, atol=1e-5 * float(q.grad.abs().max()) + 1e-7, msg=name)
    for b1, b2 in zip(model.gcn.bns, ref.gcn.bns):
        torch.testing.assert_close(b1.running_mean, b2.running_mean, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(b1.running_var, b2.running_var, rtol=1e-4, atol=1e-6)


def test_compare_loss_is_deterministic(dev):
    from ragraph_amd.preprompt import compareloss
    h, t = _hard_case(dev)
    out = []
    for _ in range(2):
        x = h.clone().requires_grad_(True)
        loss = compareloss(x, t, T)
        loss.backward()
        out.append((loss.detach().clone(), x.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_compare_loss_rejects_bad_ids(dev):
    from ragraph_amd import kernels as K
    from ragraph_amd.preprompt import compareloss
    h = torch.randn(10, 8, device=dev)
    t = torch.zeros(10, 3, dtype=torch.int64, device=dev)
    t[4, 1] = 10
    with pytest.raises(K.RagraphNativeError, match="outside"):
        compareloss(h, t, T)


# ---- sampler -------------------------------------------------------------------------------------------------------------
def test_sampler_rules(dev):
    from ragraph_amd.preprompt import prompt_pretrain_sample
    n, n_neg = 3000, 100
    adj, a = _random_graph(dev, n, 8, seed=41, isolated=(0, 17))
    t = prompt_pretrain_sample(adj, n_neg, generator=torch.Generator(device=dev).manual_seed(1)).cpu()
    assert t.shape == (n, 1 + n_neg) and t.dtype == torch.int64
    assert ((t >= 0) & (t < n)).all()
    a = a.bool()
    rows = torch.arange(n)
    has_nb = a.any(1)
    assert a[rows[has_nb], t[has_nb, 0]].all()
    assert torch.equal(t[~has_nb, 0], rows[~has_nb])
    neg = t[:, 1:]
    assert not a[rows[:, None].expand_as(neg), neg].any()
    srt = neg.sort(1).values
    assert (srt[:, 1:] != srt[:, :-1]).all()
    # the same seed gives the same sample; self loops are ignored
    again = prompt_pretrain_sample(adj, n_neg, generator=torch.Generator(device=dev).manual_seed(1)).cpu()
    assert torch.equal(t, again)
    looped, _ = _random_graph(dev, n, 8, seed=41, isolated=(0, 17), self_loops=True)
    assert looped.nnz == adj.nnz + n - 2
    with_loops = prompt_pretrain_sample(looped, n_neg, generator=torch.Generator(device=dev).manual_seed(1)).cpu()
    assert torch.equal(t, with_loops)
    # torch.manual_seed reproduces a default-generator sample
    torch.manual_seed(5)
    s1 = prompt_pretrain_sample(adj, n_neg)
    torch.manual_seed(5)
    assert torch.equal(s1, prompt_pretrain_sample(adj, n_neg))


def test_sampler_inputs_scipy_and_dense(dev):
    import scipy.sparse as sp
    from ragraph_amd.preprompt import prompt_pretrain_sample
    adj, a = _random_graph(dev, 400, 6, seed=43)
    gen = lambda: torch.Generator(device=dev).manual_seed(2)  # noqa: E731
    t = prompt_pretrain_sample(adj, 50, generator=gen())
    assert torch.equal(t, prompt_pretrain_sample(a.to(dev), 50, generator=gen()))
    assert torch.equal(t, prompt_pretrain_sample(sp.csr_matrix(a.numpy()), 50, generator=gen()))
    empty = prompt_pretrain_sample(torch.zeros(30, 30, device=dev), 100, generator=gen())   # n' = min(n, nodenum)
    assert empty.shape == (30, 31) and torch.equal(empty[:, 0], torch.arange(30, device=dev))
    assert torch.equal(empty[:, 1:].sort(1).values, torch.arange(30, device=dev).expand(30, 30))


def test_sampler_exact_complement_and_too_dense(dev):
    from ragraph_amd.graph import CSRGraph
    from ragraph_amd.preprompt import prompt_pretrain_sample
    n, n_neg = 300, 100
    a = torch.zeros(n, n)
    a[0, 100:] = 1.0                                    # row 0: exactly n_neg non-neighbours (0..99)
    a[100:, 0] = 1.0
    g = CSRGraph.from_dense(a.to(dev))
    t = prompt_pretrain_sample(g, n_neg, generator=torch.Generator(device=dev).manual_seed(3)).cpu()
    assert sorted(t[0, 1:].tolist()) == list(range(100))
    a[0, 99] = 1.0                                      # now 99 non-neighbours
    a[99, 0] = 1.0
    with pytest.raises(ValueError, match="non-neighbours"):
        prompt_pretrain_sample(CSRGraph.from_dense(a.to(dev)), n_neg)


def test_sampler_uniform_chi_square(dev):
    from scipy.stats import chi2
    from ragraph_amd.graph import CSRGraph
    from ragraph_amd.preprompt import prompt_pretrain_sample
    n, n_neg, draws = 120, 10, 2000
    a = torch.zeros(n, n)
    nb = torch.tensor([3, 4, 50, 51, 90, 119])
    a[0, nb] = 1.0
    a[nb, 0] = 1.0
    g = CSRGraph.from_dense(a.to(dev))
    counts = torch.zeros(n, dtype=torch.int64)
    pos = torch.zeros(n, dtype=torch.int64)
    for s in range(draws):
        t = prompt_pretrain_sample(g, n_neg, generator=torch.Generator(device=dev).manual_seed(1000 + s))[0].cpu()
        counts += torch.bincount(t[1:], minlength=n)
        pos[t[0]] += 1
    assert counts[nb].sum() == 0 and pos.sum() == draws and pos[nb].sum() == draws
    comp = torch.ones(n, dtype=torch.bool)
    comp[nb] = False
    obs = counts[comp].double()
    exp = draws * n_neg / comp.sum().item()
    stat = float(((obs - exp) ** 2 / exp).sum())
    assert stat < chi2.ppf(0.999, int(comp.sum()) - 1), stat
    pstat = float(((pos[nb].double() - draws / 6) ** 2 / (draws / 6)).sum())
    assert pstat < chi2.ppf(0.999, 5), pstat


# ---- memory ----------------------------------------------------------------------------------------------------------------
def test_memory_has_no_gathered_tuples(dev):
    from ragraph_amd.preprompt import compareloss, prompt_pretrain_sample
    n, n_neg, D = 20000, 100, 256
    adj, _ = _random_graph(dev, n, 6, seed=51)
    t = prompt_pretrain_sample(adj, n_neg, generator=torch.Generator(device=dev).manual_seed(1))
    h = torch.randn(n, D, device=dev, requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    loss = compareloss(h, t, T)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    gathered = n * (1 + n_neg) * D * 4                   # one [n, 1 + n_neg, D] fp32 buffer: 2.07 GB
    assert peak < gathered // 4, (peak, gathered)


# ---- a short pre-training run -----------------------------------------------------------------------------------------------
def test_pretraining_lowers_loss_and_loads_into_ragraph(dev, tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    try:
        import pretrain as P
    finally:
        sys.path.pop(0)
    from ragraph_amd.data import synthetic_tu_dataset
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph import RAGraph
    from ragraph_amd.ragraph_utils import process_tu_dataset
    from ragraph_amd.data import DataLoader
    F_in, C, D = 18, 3, 256
    ds = synthetic_tu_dataset(num_graphs=48, num_node_attributes=F_in, num_node_labels=C, seed=9)
    torch.manual_seed(0)
    model = PrePrompt(F_in, D, "prelu", 1, 0.3).to(dev)
    path = str(tmp_path / "model.pkl")
    history, best = P.pretrain(model, ds, F_in, 30, patience=30, save_path=path, device=dev, log=lambda *a: None)
    assert len(history) == 30 and min(history[1:]) < history[0] and history[-1] < history[0], history
    pre = PrePrompt(F_in, D, "prelu", 1, 0.3).to(dev)
    pre.load_state_dict(torch.load(path, map_location=dev))
    rag = RAGraph(pre, None, F_in, C, D, finetune=True, device=dev).eval()
    g = torch.Generator().manual_seed(1)
    keys = F.normalize(torch.randn(500, D, generator=g), dim=-1)
    rag.toy_graph_base.add_resources(keys.to(dev), torch.randn(500, D, generator=g).to(dev),
                                     F.one_hot(torch.randint(0, C, (500,), generator=g), C).float().to(dev))
    feats, adj, _ = process_tu_dataset(next(iter(DataLoader(ds, batch_size=8))), F_in, device=dev)
    with torch.no_grad():
        logits = rag(feats, adj)
    assert logits.shape == (feats.shape[0], C) and torch.isfinite(logits).all()
