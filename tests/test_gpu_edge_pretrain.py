"""Edge-flavour pre-training on the device: RAGraph(phase="pretrain") against the reference's own step (g19), the history
CSR, the negative sampler's law, reproducibility and errors, a short pre-training run that learns, and the chain
pretrain -> for_tune -> finetune -> evaluation."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g19_edge_pretrain.npz")


@pytest.fixture(scope="module")
def g19():
    return np.load(GOLDEN)


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def _data(g19, tmp_path, dev):
    from ragraph_amd.edge_data import EdgeListData

    return EdgeListData(_write(tmp_path, "train.txt", str(g19["train_txt"])),
                        _write(tmp_path, "test.txt", str(g19["test_txt"])), device=dev)


def _close(a, b, rtol, atol):
    return np.allclose(a.detach().cpu().numpy(), b, rtol=rtol, atol=atol)


# ---- g19: the reference's own pre-training step ---------------------------------------------------------------------------
def test_g19_pretrain_step_matches_reference(g19, tmp_path, dev):
    from ragraph_amd.RAGraph_edge import RAGraph

    s_init, _, s_step, s_gate = (int(x) for x in g19["seeds"])
    ds = _data(g19, tmp_path, dev)
    assert (ds.num_users, ds.num_items) == (int(g19["num_users"]), int(g19["num_items"]))
    assert torch.equal(ds.edges.cpu(), torch.from_numpy(g19["edges"]))     # (the mask below indexes this order)
    torch.manual_seed(s_init)
    m = RAGraph(ds, None, phase="pretrain", use_RAG=False, device=dev).train()
    assert torch.equal(m.user_embedding.detach().cpu(), torch.from_numpy(g19["init_user"]))
    assert torch.equal(m.item_embedding.detach().cpu(), torch.from_numpy(g19["init_item"]))
    assert m.resource_keys is None
    # the host-drawn dropout mask (modules/utils.py:46 on the CPU generator)
    torch.manual_seed(s_step)
    assert np.array_equal(m.draw_edge_mask().cpu().numpy(), g19["mask"])
    batch = tuple(torch.from_numpy(g19[k]).to(dev) for k in ("users", "pos", "neg"))
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    torch.manual_seed(s_step)
    opt.zero_grad()
    loss, parts = m.cal_loss(batch)
    loss.backward()
    assert float(loss) == pytest.approx(float(g19["loss"]), rel=1e-5)
    assert parts["rec_loss"] == pytest.approx(float(g19["rec"]), rel=1e-5)
    assert parts["reg_loss"] == pytest.approx(float(g19["reg"]), rel=1e-5)
    assert _close(m.user_embedding.grad, g19["g_user"], 1e-4, 1e-6)
    assert _close(m.item_embedding.grad, g19["g_item"], 1e-4, 1e-6)
    opt.step()
    assert _close(m.user_embedding, g19["user_after"], 1e-4, 1e-6)
    assert _close(m.item_embedding, g19["item_after"], 1e-4, 1e-6)
    # state dict: the reference's keys; a strict load both ways
    keys = {str(k) for k in g19["state_keys"]}
    assert set(m.state_dict().keys()) == keys
    ref_state = {"user_embedding": torch.from_numpy(g19["user_after"]), "item_embedding": torch.from_numpy(g19["item_after"])}
    ft = RAGraph(ds, None, phase="for_tune", use_RAG=False, device=dev).eval()
    ft.load_state_dict(ref_state, strict=True)
    back = {k: v.cpu() for k, v in m.state_dict().items()}
    assert set(back) == keys and all(back[k].shape == ref_state[k].shape for k in keys)
    RAGraph(ds, None, phase="pretrain", use_RAG=False, device="cpu").load_state_dict(back, strict=True)
    # for_tune: a random gate drawn afresh at every generate() (modules/RAGraph.py:177-183)
    torch.manual_seed(s_gate)
    fu, fi = ft.generate()
    assert _close(fu, g19["ft_user"], 1e-5, 1e-5) and _close(fi, g19["ft_item"], 1e-5, 1e-5)
    fu2, _ = ft.generate()
    assert not torch.equal(fu, fu2)


# ---- the history CSR ------------------------------------------------------------------------------------------------------
def _check_history(ds):
    rp, it = ds.hist_rowptr.cpu().numpy(), ds.hist_items.cpu().numpy()
    assert ds.hist_rowptr.is_cuda and rp.shape == (ds.num_users + 1,) and rp[-1] == it.size
    for u in range(ds.num_users):
        assert it[rp[u]:rp[u + 1]].tolist() == sorted(set(ds.train_user_dict.get(u, []))), u


def test_history_csr_on_device_matches_train_user_dict(g19, tmp_path, dev):
    from ragraph_amd.edge_data import EdgeListData

    ds = _data(g19, tmp_path, dev)
    hu, hi = g19["hist_users"], g19["hist_items"]
    ref = {}
    for u, i in zip(hu.tolist(), hi.tolist()):
        ref.setdefault(u, []).append(i)
    assert ds.train_user_dict == ref                   # the reference's dict: last line wins, repeats as written
    _check_history(ds)
    rng = np.random.default_rng(5)
    lines = []
    for _ in range(400):                                # users on several lines, repeats inside lines
        u = int(rng.integers(0, 150))
        items = rng.integers(0, 90, int(rng.integers(1, 12)))
        lines.append(f"{u}\t{' '.join(map(str, items))}\t{' '.join(['1700000000'] * len(items))}")
    ds2 = EdgeListData(_write(tmp_path, "r.txt", "\n".join(lines) + "\n"), device=dev)
    last = {}
    for ln in lines:
        u, items, _ = ln.split("\t")
        last[int(u)] = [int(x) for x in items.split(" ")]
    assert ds2.train_user_dict == last
    _check_history(ds2)
    assert ds2.edgelist.shape == (sum(len(ln.split("\t")[1].split(" ")) for ln in lines), 2)


# ---- the sampler's law ----------------------------------------------------------------------------------------------------
def _law_history(dev, I=60):
    """User 0: every item but 7; user 1: one item; user 2: none."""
    rng = np.random.default_rng(11)
    free = np.sort(rng.choice(I, 7, replace=False))
    h0 = np.setdiff1d(np.arange(I), free)
    rows = [h0, np.array([23]), np.zeros(0, np.int64)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    items = np.concatenate(rows).astype(np.int64)
    return torch.from_numpy(rowptr).to(dev), torch.from_numpy(items).to(dev), rows, I


def test_sampler_law_excludes_history_and_is_uniform(dev):
    from scipy.stats import chisquare

    from ragraph_amd import kernels as K

    rowptr, items, rows, I = _law_history(dev)
    K.edge_hist_check(rowptr, items, I)
    n = 120_000
    users = torch.tensor([0, 1], device=dev).repeat(n // 2)
    seed = torch.tensor([12345], dtype=torch.int64, device=dev)
    out = K.edge_neg_sample(rowptr, items, I, users, 1, seed).cpu().numpy()
    assert out.shape == (n,) and out.dtype == np.int64
    for u in (0, 1):
        got = out[u::2]
        comp = np.setdiff1d(np.arange(I), rows[u])
        assert not np.isin(got, rows[u]).any()                       # never a history item
        counts = np.array([(got == c).sum() for c in comp])
        assert counts.sum() == got.size and (counts > 0).all()       # every complement item appears
        assert chisquare(counts).pvalue > 1e-3, (u, counts)
    # n_negs = 16: [B * 16], slot b * 16 + j belongs to users[b]
    users16 = torch.tensor([0, 1, 2, 0, 1] * 400, device=dev)
    o16 = K.edge_neg_sample(rowptr, items, I, users16, 16, seed).cpu().numpy()
    assert o16.shape == (users16.numel() * 16,)
    blocks = o16.reshape(-1, 16)
    for b, u in enumerate(users16.cpu().tolist()):
        assert not np.isin(blocks[b], rows[u]).any()
    assert set(np.unique(blocks[0::5])) == set(np.setdiff1d(np.arange(I), rows[0]))
    assert ((blocks[2::5] >= 0) & (blocks[2::5] < I)).all() and len(np.unique(blocks[2::5])) == I


def test_get_train_batch_n_negs_16_and_slicing(g19, tmp_path, dev):
    ds = _data(g19, tmp_path, dev)
    hist = {u: set(v) for u, v in ds.train_user_dict.items()}
    torch.manual_seed(0)
    users, pos, neg = ds.get_train_batch(3, 40, n_negs=16)
    assert users.shape == pos.shape == (37,) and neg.shape == (37 * 16,)
    assert all(t.is_cuda and t.dtype == torch.int64 for t in (users, pos, neg))
    assert torch.equal(torch.stack([users, pos], 1), ds.edgelist[3:40])
    nb = neg.cpu().numpy().reshape(37, 16)
    for b, u in enumerate(users.cpu().tolist()):
        assert not (set(nb[b].tolist()) & hist[u])
    u2, _, n2 = ds.get_train_batch(ds.num_edges - 5, ds.num_edges + 100)    # numpy slicing: clamped at the end
    assert u2.shape == (5,) and n2.shape == (5,)


# ---- reproducibility ------------------------------------------------------------------------------------------------------
def test_batches_are_reproducible_and_need_no_sync(g19, tmp_path, dev):
    from ragraph_amd import kernels as K

    ds = _data(g19, tmp_path, dev)

    def run(seed):
        torch.manual_seed(seed)
        ds.shuffle()
        return ds.edgelist.clone(), ds.edge_time.clone(), ds.get_train_batch(0, 64)

    base_list, base_time = ds.edgelist.clone(), ds.edge_time.clone()
    e1, t1, b1 = run(7)
    # the shuffle permutes pairs and times together
    pair_time = {(tuple(p), int(t)) for p, t in zip(base_list.cpu().tolist(), base_time.cpu().tolist())}
    assert sorted(zip(map(tuple, e1.cpu().tolist()), t1.cpu().tolist())) == sorted(
        (p, t) for p, t in zip(map(tuple, base_list.cpu().tolist()), base_time.cpu().tolist()))
    assert all((tuple(p), int(t)) in pair_time for p, t in zip(e1.cpu().tolist(), t1.cpu().tolist()))
    ds.edgelist, ds.edge_time = base_list.clone(), base_time.clone()
    e2, t2, b2 = run(7)
    assert torch.equal(e1, e2) and torch.equal(t1, t2) and all(torch.equal(x, y) for x, y in zip(b1, b2))
    ds.edgelist, ds.edge_time = base_list.clone(), base_time.clone()
    e3, _, b3 = run(8)
    assert not torch.equal(e1, e3) and not torch.equal(b1[2], b3[2])
    # one seed tensor, two calls: bit-identical
    seed = torch.tensor([99], dtype=torch.int64, device=dev)
    u = ds.edgelist[:, 0].contiguous()
    a = K.edge_neg_sample(ds.hist_rowptr, ds.hist_items, ds.num_items, u, 4, seed)
    b = K.edge_neg_sample(ds.hist_rowptr, ds.hist_items, ds.num_items, u, 4, seed)
    assert torch.equal(a, b)
    # no synchronising torch call in a batch
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ds.get_train_batch(0, 64)
        ds.get_train_batch(10, 100, n_negs=3)
    finally:
        torch.cuda.set_sync_debug_mode("default")


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_full_history_raises_value_error(tmp_path, dev):
    from ragraph_amd.edge_data import EdgeListData

    text = "0\t0 1 2 3 4 1\t" + " ".join(["1700000000"] * 6) + "\n1\t2 3\t1700000000 1700003600\n"
    with pytest.raises(ValueError, match="covers every item"):
        EdgeListData(_write(tmp_path, "full.txt", text), device=dev)


def test_out_of_range_users_refused_before_writing(dev):
    from ragraph_amd import _native as N
    from ragraph_amd import kernels as K

    rowptr, items, _, I = _law_history(dev)
    seed = torch.tensor([1], dtype=torch.int64, device=dev)
    for bad in (3, -1, 1 << 40):
        users = torch.tensor([0, 1, bad, 2], device=dev)
        with pytest.raises(N.RagraphNativeError, match="outside"):
            K.edge_neg_sample(rowptr, items, I, users, 2, seed)
        out = torch.full((8,), -7, dtype=torch.int64, device=dev)
        ws = torch.zeros(1 << 12, dtype=torch.uint8, device=dev)
        rc = N.lib().ragraph_edge_neg_sample_i64(rowptr.data_ptr(), items.data_ptr(), 3, I, users.data_ptr(), 4, 2, 1,
                                                 seed.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == N.EINVAL and (out == -7).all()
    # a bad history CSR (unsorted row) is refused at the check
    with pytest.raises(N.RagraphNativeError, match="ascending"):
        K.edge_hist_check(torch.tensor([0, 2], device=dev), torch.tensor([5, 1], device=dev), 10)


# ---- learning and the chain -----------------------------------------------------------------------------------------------
def _planted(tmp_path, U=2000, I=1500, C=10, per_user=24, n_test=5, noise=0.1, seed=0):
    """Users of community c interact with items of c (and a few random ones); the test file holds n_test unseen items of
    their community each."""
    rng = np.random.default_rng(seed)
    uc, ic = rng.integers(0, C, U), np.arange(I) % C
    pools = [np.flatnonzero(ic == c) for c in range(C)]
    train, test = [], []
    for u in range(U):
        its = rng.choice(pools[uc[u]], size=per_user + n_test, replace=False)
        tr = its[:per_user].copy()
        nz = rng.random(per_user) < noise
        tr[nz] = rng.integers(0, I, int(nz.sum()))
        times = 1_700_000_000 + rng.integers(0, 48 * 3600, per_user)
        train.append(f"{u}\t{' '.join(map(str, tr))}\t{' '.join(map(str, times))}")
        test.append(f"{u}\t{' '.join(map(str, its[per_user:]))}")
    return _write(tmp_path, "p.txt", "\n".join(train) + "\n"), _write(tmp_path, "p_val.txt", "\n".join(test) + "\n")


def test_pretraining_learns(tmp_path, dev):
    from ragraph_amd.edge_data import EdgeListData
    from ragraph_amd.edge_eval import Metric
    from ragraph_amd.RAGraph_edge import RAGraph

    ds = EdgeListData(*_planted(tmp_path), device=dev)
    torch.manual_seed(2023)
    m = RAGraph(ds, None, phase="pretrain", device=dev)
    metric = Metric("recall;ndcg", "20")
    m.eval()
    r0 = float(metric.eval(m, ds)["recall"][0])
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(3):
        ds.shuffle()
        m.train()
        s, ep = 0, []
        while s + 2048 <= ds.num_edges:
            opt.zero_grad()
            loss, _ = m.cal_loss(ds.get_train_batch(s, s + 2048))
            loss.backward()
            opt.step()
            ep.append(float(loss))
            s += 2048
        losses.append(np.mean(ep))
    m.eval()
    r1 = float(metric.eval(m, ds)["recall"][0])
    assert losses[-1] < losses[0] and r1 >= 3 * r0 and r1 > 0, (losses, r0, r1)


def test_chain_pretrain_for_tune_finetune_eval(tmp_path, dev):
    from ragraph_amd.edge_data import EdgeListData
    from ragraph_amd.edge_eval import Metric
    from ragraph_amd.RAGraph_edge import RAGraph

    ds = EdgeListData(*_planted(tmp_path, U=400, I=300, per_user=12), device=dev)
    torch.manual_seed(1)
    pre = RAGraph(ds, None, phase="pretrain", device=dev).train()
    opt = torch.optim.Adam(pre.parameters(), lr=1e-3)
    ds.shuffle()
    for s in range(0, 2048, 1024):
        opt.zero_grad()
        loss, _ = pre.cal_loss(ds.get_train_batch(s, s + 1024))
        loss.backward()
        opt.step()
    path = str(tmp_path / "pre.pt")
    torch.save(pre.state_dict(), path)
    ft = RAGraph(ds, None, phase="for_tune", device=dev)
    ft.load_state_dict(torch.load(path), strict=True)
    m = RAGraph(ds, ft, phase="finetune", use_RAG=True, retrieve_num=5, device=dev).train()
    assert m.resource_keys is not None and m.resource_keys.shape[0] == ds.num_users + ds.num_items
    loss, parts = m.cal_loss(ds.get_train_batch(0, 1024))
    loss.backward()
    assert np.isfinite(float(loss)) and np.isfinite(parts["rec_loss"])
    grads = [p.grad for p in m.parameters() if p.requires_grad]
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads)
    m.eval()
    res = Metric("recall;ndcg", "20").eval(m, ds)
    assert 0.0 <= float(res["recall"][0]) <= 1.0 and np.isfinite(res["ndcg"]).all()
