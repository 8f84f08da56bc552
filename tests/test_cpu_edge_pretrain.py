"""Edge-flavour pre-training, host side: the g19 fixture (the reference's own EdgeListData / RAGraph(phase="pretrain") on
CPU), the pretrain constructor's tables on the CPU, the host flattening of train_user_dict into the sampler's history CSR,
a torch-CPU restatement of the fixture's loss, and the sampler's refusal to run without a device."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g19_edge_pretrain.npz")


@pytest.fixture(scope="module")
def g19():
    return np.load(GOLDEN)


def _data(g19, tmp_path, device="cpu"):
    from ragraph_amd.edge_data import EdgeListData

    tr, te = tmp_path / "train.txt", tmp_path / "test.txt"
    tr.write_text(str(g19["train_txt"]))
    te.write_text(str(g19["test_txt"]))
    return EdgeListData(str(tr), str(te), device=device)


def test_g19_loads(g19):
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert sorted(str(k) for k in g19["state_keys"]) == ["item_embedding", "user_embedding"]
    for k in ("init_user", "init_item", "g_user", "g_item", "user_after", "item_after", "ft_user", "ft_item"):
        assert np.isfinite(g19[k]).all(), k
    assert g19["users"].shape == g19["pos"].shape == g19["neg"].shape


def test_pretrain_constructor_on_cpu_reproduces_g19_tables(g19, tmp_path):
    """modules/RAGraph.py:93-95: the user table, then the item table, xavier-uniform on the CPU generator -- bit for bit."""
    from ragraph_amd.RAGraph_edge import RAGraph

    ds = _data(g19, tmp_path)
    torch.manual_seed(int(g19["seeds"][0]))
    m = RAGraph(ds, None, phase="pretrain", use_RAG=False, device="cpu")
    assert torch.equal(m.user_embedding.detach(), torch.from_numpy(g19["init_user"]))
    assert torch.equal(m.item_embedding.detach(), torch.from_numpy(g19["init_item"]))
    assert set(m.state_dict().keys()) == {str(k) for k in g19["state_keys"]}
    assert m.resource_keys is None and m.gating_weight is None


def test_flatten_history_last_line_wins_and_removes_repeats(g19):
    from ragraph_amd.edge_data import flatten_history

    # user 1 on two lines (the dict keeps the second), user 2 with a repeat, user 3 without interactions
    d = {0: [4, 1], 2: [3, 0, 3, 3], 1: [2, 5]}
    rowptr, items = flatten_history(d, 4, 6)
    assert rowptr.tolist() == [0, 2, 4, 6, 6]
    assert items.tolist() == [1, 4, 2, 5, 0, 3]
    assert rowptr.dtype == items.dtype == np.int64
    # the fixture's train_user_dict (the reference's): every row the sorted set of the recorded list
    U, I = int(g19["num_users"]), int(g19["num_items"])
    hu, hi = g19["hist_users"], g19["hist_items"]
    ref = {}
    for u, i in zip(hu.tolist(), hi.tolist()):
        ref.setdefault(u, []).append(i)
    rowptr, items = flatten_history(ref, U, I)
    for u in range(U):
        assert items[rowptr[u]:rowptr[u + 1]].tolist() == sorted(set(ref.get(u, []))), u
    assert ref[4] == [5, 12, 20]                     # the second line of user 4
    with pytest.raises(ValueError):
        flatten_history({0: [6]}, 1, 6)


def test_edge_data_cpu_keeps_file_order_and_history(g19, tmp_path):
    ds = _data(g19, tmp_path)
    lines = [ln.split("\t") for ln in str(g19["train_txt"]).strip().split("\n")]
    pairs = [(int(u), int(i)) for u, items, _ in lines for i in items.split(" ")]
    assert ds.edgelist.tolist() == [list(p) for p in pairs]                      # file order, repeats included
    assert ds.edgelist.dtype == ds.edge_time.dtype == torch.int64 and ds.edge_time.shape == (len(pairs),)
    assert ds.train_user_dict[4] == [5, 12, 20]
    rp, it = ds.hist_rowptr.numpy(), ds.hist_items.numpy()
    assert it[rp[6]:rp[7]].tolist() == [3, 9, 17]


def _loss_restated(g19):
    """modules/RAGraph.py:250-355 in torch on the CPU from the fixture's tables, graph, mask and batch (pretrain: no gate,
    no retrieval)."""
    U = int(g19["num_users"])
    n = U + int(g19["num_items"])
    mask = torch.from_numpy(g19["mask"])
    e = torch.from_numpy(g19["edges"])[mask]
    norm = torch.from_numpy(g19["edge_norm"])[mask]
    t = torch.from_numpy(g19["edge_times"])[mask].double()
    t = (t - t.min()) / (t.max() - t.min())
    dst = e[:, 1]
    mx = torch.full((n,), float("-inf"), dtype=torch.float64).scatter_reduce(0, dst, t, reduce="amax")
    ex = torch.exp(t - mx[dst])
    tn = ex / torch.zeros(n, dtype=torch.float64).index_add_(0, dst, ex)[dst]
    w = norm.double() * 0.5 + tn * 0.5
    x = torch.cat([torch.from_numpy(g19["init_user"]), torch.from_numpy(g19["init_item"])]).double()
    res = [x]
    for _ in range(3):
        res.append(torch.zeros_like(x).index_add_(0, dst, res[-1][e[:, 0]] * w[:, None]))
    tot = sum(res)
    ue, ie = tot[:U], tot[U:]
    us, ps, ns = (torch.from_numpy(g19[k]) for k in ("users", "pos", "neg"))
    pos, neg = (ue[us] * ie[ps]).sum(1), (ue[us] * ie[ns]).sum(1)
    rec = (-torch.log(1e-10 + torch.sigmoid(pos - neg))).mean()
    x0u, x0i = x[:U], x[U:]
    reg = 0.5 * (x0u[us].norm(2) ** 2 + x0i[ps].norm(2) ** 2 + x0i[ns].norm(2) ** 2) / len(us)
    return float(rec), float(1e-4 * reg)


def test_loss_restated_matches_g19(g19):
    rec, reg = _loss_restated(g19)
    assert rec == pytest.approx(float(g19["rec"]), rel=1e-5)
    assert reg == pytest.approx(float(g19["reg"]), rel=1e-5)
    assert rec + reg == pytest.approx(float(g19["loss"]), rel=1e-5)


def test_get_train_batch_without_device_raises(g19, tmp_path):
    from ragraph_amd._native import RagraphNativeError

    ds = _data(g19, tmp_path)
    with pytest.raises(RagraphNativeError):
        ds.get_train_batch(0, 8)
