"""Edge flavour, the rows the loss reads (RAGraph.forward_rows, cal_loss with loss_rows = "batch"): bit for bit the rows of
forward() in every phase and on both retrieval branches, the same loss and gradients within the step's tolerance, and the
work for every other node really is skipped."""
import pytest
import torch

pytestmark = pytest.mark.gpu

U, I, D = 300, 200, 64


def close(a, b, tol=1e-4):   # (tests/test_gpu_backward.py's measure)
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _model(dev, **kw):
    from ragraph_amd.data import synthetic_bipartite
    from ragraph_amd.RAGraph_edge import RAGraph

    edges, norm, times = synthetic_bipartite(U, I, edges_per_user=6, seed=12, device=dev)

    class DS:
        num_users, num_items = U, I
    DS.edges, DS.edge_norm, DS.edge_times = edges, norm, times

    class Pre:
        def generate(self):
            g = torch.Generator(device=dev).manual_seed(5)
            return 0.1 * torch.randn(U, D, device=dev, generator=g), 0.1 * torch.randn(I, D, device=dev, generator=g)

    torch.manual_seed(3)
    return RAGraph(DS, Pre(), device=dev, **kw)


USER_ROWS = [7, 299, 7, 0, 150, 151, 150, 42, 7]          # repeated, unsorted
ITEM_ROWS = [199, 3, 3, 0, 77, 199, 120]


@pytest.mark.parametrize("case", ["finetune_rag", "finetune_lora", "finetune_noise", "vanilla_large_k", "pretrain", "for_tune"])
def test_forward_rows_equals_forward_at_those_rows(dev, case):
    from ragraph_amd import kernels as K

    kw = {"finetune_rag": dict(phase="finetune", use_RAG=True, retrieve_num=5),
          "finetune_lora": dict(phase="finetune", use_RAG=True, use_LoRA=True, LoRA_rank=8, retrieve_num=5),
          "finetune_noise": dict(phase="finetune", use_RAG=True, use_noise=True, retrieve_num=5),
          "vanilla_large_k": dict(phase="vanilla", use_RAG=True, retrieve_num=70),
          "pretrain": dict(phase="pretrain", use_RAG=False),
          "for_tune": dict(phase="for_tune", use_RAG=False)}[case]
    m = _model(dev, **kw)
    m = m.train() if case == "finetune_noise" else m.eval()
    if case == "vanilla_large_k":
        assert m.resource_keys.shape[0] == U + I and m.retrieve_num > K.N.TOPK_MAX
    ur, ir = torch.tensor(USER_ROWS, device=dev), torch.tensor(ITEM_ROWS, device=dev)
    args = (m.edges, m.edge_norm, m.edge_times)
    for grad in (False, True):                       # the inference kernels and the autograd wrappers
        with torch.set_grad_enabled(grad):
            torch.manual_seed(11)                    # (noise indices / the for_tune gate are drawn per call)
            uo, io = m.forward(*args)
            torch.manual_seed(11)
            us, is_ = m.forward_rows(*args, ur, ir)
        assert us.shape == (len(USER_ROWS), D) and is_.shape == (len(ITEM_ROWS), D)
        assert torch.equal(us.detach(), uo.detach()[ur]) and torch.equal(is_.detach(), io.detach()[ir])
    if case == "for_tune":                           # the gate really is drawn per call: another seed, other rows
        with torch.no_grad():
            torch.manual_seed(12)
            assert not torch.equal(m.forward_rows(*args, ur, ir)[0], us.detach())


def _batch():
    g = torch.Generator().manual_seed(21)
    users = torch.randint(0, U, (64,), generator=g)
    pos = torch.randint(0, I, (64,), generator=g)
    neg = torch.randint(0, I, (64,), generator=g)
    users[5] = users[9] = users[0]                   # repeated users
    neg[3] = pos[17]                                 # an item that is a positive and a negative
    return users, pos, neg


@pytest.mark.parametrize("dropout", [0.0, 0.5])
def test_cal_loss_batch_rows_equals_all_rows(dev, dropout):
    m = _model(dev, phase="finetune", use_RAG=True, use_LoRA=True, LoRA_rank=8, retrieve_num=5).train()
    assert m.loss_rows == "batch"                    # the default
    m.edge_dropout, m.dropout_rng = dropout, "host"
    batch = _batch()
    out = {}
    for mode in ("all", "batch"):
        m.loss_rows = mode
        m.zero_grad(set_to_none=True)
        torch.manual_seed(8)                         # the same dropout mask
        loss, parts = m.cal_loss(batch)
        loss.backward()
        out[mode] = (float(loss), parts, {k: p.grad.clone() for k, p in m.named_parameters()})
    la, pa, ga = out["all"]
    lb, pb, gb = out["batch"]
    assert lb == la and pb == pa and set(pb) == {"rec_loss", "reg_loss"}
    assert set(ga) == set(gb) and len(ga) == 8
    for k in ga:
        err = float((gb[k] - ga[k]).abs().max())
        print(f"dropout {dropout} {k}: max abs err {err:.3e} of {float(ga[k].abs().max()):.3e}")
        assert float(ga[k].abs().max()) > 0 and close(gb[k], ga[k], 2e-4), k


def test_batch_rows_skip_the_other_nodes_retrieval(dev, monkeypatch):
    from ragraph_amd import kernels as K

    m = _model(dev, phase="finetune", use_RAG=True, retrieve_num=5).train()
    m.edge_dropout = 0.0
    seen = []
    m._index = K.KeyIndex(m.keys_normalized)         # (what forward makes on first use)
    real = m._index.topk

    def spy(queries, k, *a, **kw):
        seen.append(int(queries.shape[0]))
        return real(queries, k, *a, **kw)

    monkeypatch.setattr(m._index, "topk", spy)
    users, pos, neg = _batch()
    distinct = len(set(users.tolist())) + len(set(pos.tolist()) | set(neg.tolist()))
    assert distinct < U + I
    m.loss_rows = "batch"
    m.cal_loss((users, pos, neg))
    m.loss_rows = "all"
    m.cal_loss((users, pos, neg))
    assert seen == [distinct, U + I]
