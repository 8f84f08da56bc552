"""Captured fine-tuning steps (ragraph_amd.capture.CapturedTrainStep): the device-slope SpMM / act_grad entries against the
host-scalar ones bit for bit, replayed training against eager training bit for bit (node few-shot, node at the node_528
shape, graph few-shot), the few-shot prototype helpers against the reference's torch formulas, and the error paths."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _hub_graph(dev, n, seed, hubs=()):
    """Random sparse graph; rows in `hubs` get more than ROW_BLOCK edges (the hub-row block sums)."""
    from ragraph_amd.graph import CSRGraph

    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(0, n, (8 * n,), generator=g)
    cols = torch.randint(0, n, (8 * n,), generator=g)
    for h in hubs:
        rows = torch.cat([rows, torch.full((5000,), h)])
        cols = torch.cat([cols, torch.randint(0, n, (5000,), generator=g)])
    vals = torch.rand(rows.numel(), generator=g)
    csr, _ = CSRGraph.from_coo(rows.to(dev), cols.to(dev), vals.to(dev), n)
    return csr


@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("hubs", [False, True])
def test_device_slope_kernels_match_host_scalar(dev, D, hubs):
    from ragraph_amd import kernels as K

    n = 3000
    g = _hub_graph(dev, n, 3 + D, hubs=(7, 1500) if hubs else ())
    assert g.has_long_rows == hubs
    torch.manual_seed(D)
    x = torch.randn(n, D, device=dev)
    bias = torch.randn(D, device=dev) * 0.1
    gy = torch.randn(n, D, device=dev)
    for slope in (0.25, 1.7, 0.0, -0.3):
        a = torch.full((1,), slope, device=dev)
        y_dev, z_dev = K.spmm_csr_prelu_dev(g.rowptr, g.col, g.val, x, bias, a, want_z=True, long_rows=hubs)
        y_host = K.spmm_csr(g.rowptr, g.col, g.val, x, bias=bias, act=K.ACT_PRELU, alpha=slope, long_rows=hubs)
        z_host = K.spmm_csr(g.rowptr, g.col, g.val, x, bias=bias, act=K.ACT_NONE, long_rows=hubs)
        assert torch.equal(y_dev, y_host) and torch.equal(z_dev, z_host)
        assert torch.equal(K.spmm_csr_prelu_dev(g.rowptr, g.col, g.val, x, bias, a, long_rows=hubs), y_host)
        gz, t = K.act_grad_prelu_dev(z_dev, gy, a, want_alpha_terms=True)
        assert torch.equal(K.act_grad_prelu_dev(z_dev, gy, a), gz)
        if slope > 0:   # the host-scalar path: through the output y
            gz_h, t_h = K.act_grad(y_host, gy, K.ACT_PRELU, slope, want_alpha_terms=True)
        else:           # the host-scalar path for a slope <= 0: on z, terms gy * (z - relu(z))
            gz_h = K.act_grad(z_host, gy, K.ACT_PRELU, slope)
            ones = torch.ones(D, device=dev)
            t_h = K.mul(gy, K.axpby(z_host, 1.0, K.mul_cols(z_host, ones, K.ACT_RELU), -1.0))
        assert torch.equal(gz, gz_h) and torch.equal(t, t_h)
        assert torch.equal(K.column_sums(t), K.column_sums(t_h))


@pytest.mark.parametrize("slope", [0.25, 1.7, 0.0, -0.3])
def test_device_slope_layer_grads_match_host_scalar_path(dev, slope):
    """autograd.spmm_csr in device-slope mode: output and every gradient (x, bias, slope) equal the host-scalar mode's."""
    from ragraph_amd import autograd as A
    from ragraph_amd import kernels as K

    n, D = 3000, 256
    g = _hub_graph(dev, n, 11, hubs=(3,))
    torch.manual_seed(5)
    x0, b0, w = torch.randn(n, D, device=dev), torch.randn(D, device=dev), torch.randn(n, D, device=dev)
    outs = []
    for mode in ("host", "dev"):
        x, b = x0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        a = torch.full((1,), slope, device=dev, requires_grad=True)
        y = A.spmm_csr(g, x, b, K.ACT_PRELU, a, slope if mode == "host" else None)
        (y * w).sum().backward()
        outs.append((y.detach(), x.grad, b.grad, a.grad))
    for h, d in zip(*outs):
        assert torch.equal(h, d)


# ---- few-shot helpers ----------------------------------------------------------------------------------------------------
def test_fewshot_helpers_match_reference_formulas(dev):
    from ragraph_amd.ragraph_utils import fewshot_mean_logits, fewshot_predict_labels_by_mean, fewshot_predict_logits

    torch.manual_seed(3)
    C, D = 5, 256
    labels = torch.tensor([3, 0, 1, 4, 2, 2, 0, 3, 1, 4, 4, 0, 2], device=dev)
    fl = torch.randn(labels.numel(), D, device=dev)
    mean = fewshot_mean_logits(fl, labels)
    ref = torch.stack([fl[labels == c].mean(dim=0) for c in range(C)])   # utility.py:72-92 + :114-127
    assert mean.shape == (C, D)
    assert float((mean - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    assert torch.equal(fewshot_mean_logits(fl, labels, num_class=C), mean)
    logits = torch.randn(40, D, device=dev, requires_grad=True)
    cos = fewshot_predict_logits(mean, logits)
    cref = F.cosine_similarity(logits.detach().unsqueeze(1), mean.unsqueeze(0), dim=-1)   # :129-134
    assert float((cos.detach() - cref).abs().max()) <= 1e-6 * float(cref.abs().max())
    assert torch.equal(fewshot_predict_labels_by_mean(mean, logits.detach()), cref.max(dim=1)[1])   # :154-162
    wts = torch.randn(40, C, device=dev)
    (cos * wts).sum().backward()
    l2 = logits.detach().clone().requires_grad_(True)
    (F.cosine_similarity(l2.unsqueeze(1), mean.unsqueeze(0), dim=-1) * wts).sum().backward()
    assert float((logits.grad - l2.grad).abs().max()) <= 1e-5 * float(l2.grad.abs().max())
    with pytest.raises(KeyError):   # label 1 missing from range(3): the reference's dict lookup fails
        fewshot_mean_logits(fl[:4], torch.tensor([0, 2, 3, 0], device=dev))


# ---- replayed training against eager training ------------------------------------------------------------------------
def _snapshot(model):
    return [p.detach().clone() for p in model.parameters()]


def _run_pair(make, steps, batches, between=None):
    """make() -> (model, step_fn, opt); the same model trained eagerly and through a captured step from the same state.
    between(): run after the capture, before the first replay."""
    m_e, step_e, opt_e = make()
    m_c, step_c, opt_c = make()
    for a, b in zip(_snapshot(m_e), _snapshot(m_c)):
        assert torch.equal(a, b)
    from ragraph_amd.capture import CapturedTrainStep

    cap = CapturedTrainStep(step_c, opt_c, *batches[0])
    for a, b in zip(_snapshot(m_e), _snapshot(m_c)):
        assert torch.equal(a, b), "warm-up must leave the parameters as they were"
    if between is not None:
        between()
    for i in range(steps):
        ins = batches[i % len(batches)]
        opt_e.zero_grad()
        le = step_e(*ins)
        le.backward()
        opt_e.step()
        lc = cap(*ins)
        assert torch.equal(le.detach(), lc), f"loss differs at step {i + 1}"
        for (name, p), q in zip(m_e.named_parameters(), m_c.parameters()):
            assert torch.equal(p.detach(), q.detach()), f"{name} differs at step {i + 1}"
    return m_e, m_c


def _fewshot_setup(dev):
    from ragraph_amd.data import DataLoader, synthetic_tu_dataset
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph_fewshot import RAGraph as RAGraphFewShot
    from ragraph_amd.ragraph_utils import fewshot_mean_logits, fewshot_predict_logits, process_tu_dataset

    F_in, C, D = 18, 3, 256
    ds = synthetic_tu_dataset(num_graphs=8, num_node_attributes=F_in, num_node_labels=C, seed=8)
    feats, adj, node_oh = process_tu_dataset(next(iter(DataLoader(ds, batch_size=8))), F_in, device=dev)
    node_labels = node_oh.argmax(dim=1)
    sup = synthetic_tu_dataset(num_graphs=2, num_node_attributes=F_in, num_node_labels=C, seed=9)
    sfeat, sadj, soh = process_tu_dataset(next(iter(DataLoader(sup, batch_size=2))), F_in, device=dev)
    slabels = torch.arange(sfeat.shape[0], device=dev) % C
    _ = adj.row_normalized_values(), sadj.row_normalized_values()
    gen = torch.Generator(device=dev).manual_seed(4)
    bank = (F.normalize(torch.randn(600, D, device=dev, generator=gen), dim=-1), torch.randn(600, D, device=dev, generator=gen),
            F.one_hot(torch.randint(0, C, (600,), device=dev, generator=gen), C).float(),
            torch.rand(600, 10, device=dev, generator=gen))
    anchors = torch.randint(0, feats.shape[0], (10,), device=dev, generator=gen)

    def make():
        torch.manual_seed(12)
        pre = PrePrompt(F_in, D, "prelu", 2, 0.3).to(dev)
        with torch.no_grad():
            pre.gcn.convs[1].bias.normal_(0, 0.1)
        model = RAGraphFewShot(pre, None, torch.zeros(C, D, device=dev), D, device=dev, dataset_name="ENZYMES")
        model.toy_graph_base.add_resources(*bank)
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)

        def step(x, y):   # RAGraph_node_fewshot/finetune-rag.py:94-103
            fewshot_logits = pre.inference(sfeat, sadj)
            mean = fewshot_mean_logits(fewshot_logits, slabels, num_class=C)
            logits = model(x, adj, mean, anchors=anchors)
            return F.cross_entropy(fewshot_predict_logits(mean, logits), y)
        return model, step, opt

    feats2 = feats + 0.1 * torch.rand(feats.shape, device=dev, generator=gen)
    return make, [(feats, node_labels), (feats2, node_labels)], adj, anchors


def test_node_fewshot_step_replays_bit_exact(dev):
    make, batches, _, _ = _fewshot_setup(dev)
    m_e, m_c = _run_pair(make, 20, batches)
    slope = m_c.pretrain_model.gcn.convs[1].act.weight
    assert abs(float(slope) - 0.25) > 1e-3, "the PReLU slope must have moved: the case a frozen slope gets wrong"


def _node528(dev):
    from ragraph_amd.data import DataLoader, synthetic_tu_dataset
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph import RAGraph
    from ragraph_amd.ragraph_utils import process_tu_dataset

    F_in, C, D, N = 18, 3, 256, 20_000   # tools/bench_blocks.py finetune_node("528")
    ds = synthetic_tu_dataset(num_graphs=16, num_node_attributes=F_in, num_node_labels=C, seed=21)
    feats, adj, _ = process_tu_dataset(next(iter(DataLoader(ds, batch_size=16))), F_in, device=dev)
    _ = adj.row_normalized_values()
    n = feats.shape[0]
    gen = torch.Generator(device=dev).manual_seed(74)
    keys = F.normalize(torch.randn(N, D, device=dev, generator=gen), dim=-1)
    vals = torch.randn(N, D, device=dev, generator=gen)
    labs = F.one_hot(torch.randint(0, C, (N,), device=dev, generator=gen), C).float()
    labels = torch.randint(0, C, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(75))

    def make(noise=False, capturable=True):
        torch.manual_seed(5)
        model = RAGraph(PrePrompt(F_in, D, "prelu", 1, 0.3).to(dev), None, F_in, C, D, finetune=True,
                        noise_finetune=noise, device=dev)
        model.toy_graph_base.add_resources(keys, vals, labs)
        model.train()
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-3, capturable=capturable)

        def step(x, y):   # RAGraph_node/finetune-rag.py:77-84
            return F.cross_entropy(model(x, adj), y)
        return model, step, opt

    return make, feats, adj, labels


def test_node528_step_replays_bit_exact(dev):
    make, feats, _, labels = _node528(dev)
    feats2 = torch.rand_like(feats)

    def churn():   # eager work on many row counts after the capture (varying TU batches): the graph's bias-gradient
        from ragraph_amd import kernels as K   # segment pointers must stay alive and untouched

        for n in range(1, 301):
            K.column_sums(torch.ones(n, 8, device=dev))
        junk = [torch.zeros(64, dtype=torch.int64, device=dev) for _ in range(2000)]   # (in-bounds if ever read)
        del junk
    _run_pair(make, 20, [(feats, labels), (feats2, labels)], between=churn)


def test_graph_fewshot_step_replays_bit_exact(dev):
    from ragraph_amd.data import DataLoader, synthetic_tu_dataset
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph_fewshot import RAGraphGraphFewShot
    from ragraph_amd.ragraph_utils import process_tu_dataset

    F_in, C, D = 18, 2, 256
    ds = synthetic_tu_dataset(num_graphs=1, num_node_attributes=F_in, num_node_labels=3, seed=30)
    feats, adj, _ = process_tu_dataset(next(iter(DataLoader(ds, batch_size=1))), F_in, device=dev)
    _ = adj.row_normalized_values()
    gen = torch.Generator(device=dev).manual_seed(31)
    bank = (F.normalize(torch.randn(800, D, device=dev, generator=gen), dim=-1), torch.randn(800, D, device=dev, generator=gen),
            F.one_hot(torch.randint(0, C, (800,), device=dev, generator=gen), C).float())
    mean = torch.randn(C, D, device=dev, generator=gen)
    y = torch.tensor([1], device=dev)

    def make():
        torch.manual_seed(13)
        model = RAGraphGraphFewShot(PrePrompt(F_in, D, "prelu", 2, 0.3).to(dev), None, F_in, C, D, device=dev,
                                    dataset_name="PROTEINS")
        model.toy_graph_base.add_resources(*bank)
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)

        def step(x, m):
            return F.cross_entropy(model(x, adj, m), y)
        return model, step, opt

    _, m_c = _run_pair(make, 20, [(feats, mean), (feats * 0.5, mean)])
    slope = float(m_c.pretrain_model.gcn.convs[1].act.weight.detach())
    assert abs(slope - 0.25) > 1e-3, "the decode layer's PReLU slope must have moved"


# ---- errors ------------------------------------------------------------------------------------------------------------
def _state(model, opt):
    return ([p.detach().clone() for p in model.parameters()],
            {id(p): {k: v.clone() for k, v in s.items()} for p, s in opt.state.items()})


def _same(model, opt, st):
    ps, ss = st
    assert all(torch.equal(a, b.detach()) for a, b in zip(ps, model.parameters()))
    assert sorted(id(p) for p in opt.state) == sorted(ss), "states made by the warm-up must be dropped"
    for p, s in opt.state.items():
        assert sorted(s) == sorted(ss[id(p)])
        for k, v in s.items():
            assert torch.equal(v, ss[id(p)][k]), k
    assert all(p.grad is None for p in model.parameters())


def test_capture_errors(dev):
    from ragraph_amd.capture import CapturedTrainStep
    from ragraph_amd.kernels import RagraphNativeError

    make, feats, adj, labels = _node528(dev)
    # a non-capturable optimizer: rejected before any device work
    model, step, opt = make(capturable=False)
    st = _state(model, opt)
    with pytest.raises(ValueError, match="capturable"):
        CapturedTrainStep(step, opt, feats, labels)
    _same(model, opt, st)
    # noisy fine-tuning: host-generator noise, rejected with the model and optimizer as they were
    model, step, opt = make(noise=True)
    st = _state(model, opt)
    with pytest.raises(RagraphNativeError, match="noise"):
        CapturedTrainStep(step, opt, feats, labels)
    _same(model, opt, st)
    # a dense adjacency: its CSR conversion (torch.nonzero) synchronises inside the capture
    model, _, opt = make()
    dense = torch.zeros(adj.n, adj.n, device=dev)
    rows = torch.repeat_interleave(torch.arange(adj.n, device=dev), adj.rowptr[1:] - adj.rowptr[:-1])
    dense[rows, adj.col.long()] = adj.val
    st = _state(model, opt)
    with pytest.raises(RagraphNativeError, match="could not be captured"):
        CapturedTrainStep(lambda x, y: F.cross_entropy(model(x, dense), y), opt, feats, labels)
    _same(model, opt, st)
    # a step that fails during the warm-up, after an optimizer step: everything put back, the exception passes through
    model, step, opt = make()
    st = _state(model, opt)
    calls = []

    def failing(x, y):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("second warm-up step fails")
        return step(x, y)
    with pytest.raises(RuntimeError, match="second warm-up step"):
        CapturedTrainStep(failing, opt, feats, labels)
    _same(model, opt, st)
    # a bank grown after the capture: the next call asks for a re-capture instead of replaying stale addresses
    model, step, opt = make()
    cap = CapturedTrainStep(step, opt, feats, labels)
    cap(feats, labels)
    torch.cuda.synchronize()
    tgb = model.toy_graph_base
    tgb.add_resources(tgb.resource_keys[:5].clone(), tgb.resource_values[:5].clone(), tgb.resource_labels[:5].clone())
    with pytest.raises(RagraphNativeError, match="re-capture"):
        cap(feats, labels)
