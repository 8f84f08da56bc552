"""Edge evaluation on the device (RAGraph_edge/utils/metrics.py:83-214): the masked inner-product top-k
(ragraph_topk_dot_masked_f32) bit-exact against the oracle's linear + history fill + topk_rows on both dispatch families,
the amazon-width batch without a score slab, Metric.eval / eval_grouped against golden g17 from the reference, an
end-to-end run on an EdgeListData, and the argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import cref, pipeline

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MASK = np.float32(-1e8)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def csr(lists):
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    items = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if rowptr[-1] else np.zeros(0, np.int64)
    return rowptr, items


def oracle(ue, ie, users, hist, k, rows):
    """cref.linear with -1e8 written in, then cref.topk_rows -- for the listed rows."""
    S = cref.linear(ue[users[rows]], ie)
    for r, b in enumerate(rows):
        S[r, np.asarray(hist[b], dtype=np.int64)] = MASK
    return cref.topk_rows(S, k)


def make_case(B, N, D, k, seed):
    rng = np.random.default_rng(seed)
    nU = B + 7
    ue = rng.standard_normal((nU, D)).astype(np.float32)
    ie = rng.standard_normal((N, D)).astype(np.float32)
    if N > 8:
        ie[5] = ie[3]                                   # exactly duplicated item rows: ties broken by index
        ie[N - 1] = ie[3]
    users = rng.integers(0, nU, B)
    if B > 2:
        users[2] = users[1]                             # repeated user ids
    hist = []
    for b in range(B):
        h = rng.integers(0, N, int(rng.integers(0, min(N, 30)))).tolist()   # unsorted, duplicates possible
        if h and b % 4 == 1:
            h += h[: len(h) // 2 + 1]                   # explicit duplicates
        hist.append(h)
    top1 = np.argmax(ue[users] @ ie.T, axis=1)
    for b in range(0, B, 3):
        hist[b] = hist[b] + [int(top1[b])]              # the user's (near-)best item is history: masked, not ranked
    hist[0] = []                                        # an empty history
    special = []
    if B > 1:
        b = B - 1                                       # all but 3 items masked: the tail is -1e8 ties in index order
        keep = rng.choice(N, 3, replace=False)
        hist[b] = np.setdiff1d(np.arange(N), keep)[::-1].tolist()
        special.append(b)
    if B > 3 and N > 1000:
        b = B // 2                                      # one 20 000-item history (duplicates when N is smaller)
        hist[b] = rng.integers(0, N, 20000).tolist()
        special.append(b)
    return ue, ie, users, hist, special


SHAPES = [(1, 1000, 64, 20), (7, 4099, 64, 64), (513, 3001, 128, 20), (600, 107028, 64, 20), (2000, 50000, 256, 10),
          (33, 2000, 48, 20), (300, 10, 64, 10)]


@pytest.mark.parametrize("slab_env", [None, "0"])
@pytest.mark.parametrize("B,N,D,k", SHAPES)
def test_topk_dot_masked_matches_oracle(dev, monkeypatch, B, N, D, k, slab_env):
    from ragraph_amd import kernels as K

    if slab_env is not None:
        monkeypatch.setenv("RAGRAPH_TOPK_SLAB", slab_env)
    else:
        monkeypatch.delenv("RAGRAPH_TOPK_SLAB", raising=False)
    ue, ie, users, hist, special = make_case(B, N, D, k, B + N + D + k)
    rp, items = csr(hist)
    s, i = K.topk_dot_masked(T(ue, dev), T(ie, dev), k, T(rp, dev), T(items, dev), users=T(users, dev))
    s, i = s.cpu().numpy(), i.cpu().numpy()
    rng = np.random.default_rng(0)
    rows = np.arange(B) if B <= 600 else np.unique(np.concatenate([rng.choice(B, 250, replace=False), special, [0, 1, 2]]))
    rs, ri = oracle(ue, ie, users, hist, k, rows)
    assert np.array_equal(i[rows], ri), (B, N, D, k, slab_env)
    assert np.array_equal(s[rows], rs), (B, N, D, k, slab_env)
    for b in special:
        if len(set(hist[b])) >= N - 3 and k > 3:        # the masked tail, in ascending index order
            assert np.all(s[b, 3:] == MASK)
            assert np.all(np.diff(i[b, 3:]) > 0)


def test_topk_dot_masked_amazon_width_no_slab(dev):
    from ragraph_amd import kernels as K

    B, N, D, k = 20000, 107028, 64, 20
    rng = np.random.default_rng(5)
    ue = rng.standard_normal((B, D)).astype(np.float32)
    ie = rng.standard_normal((N, D)).astype(np.float32)
    hist = [rng.integers(0, N, int(rng.integers(0, 20))).tolist() for _ in range(B)]
    rp, items = csr(hist)
    assert K.topk_dot_masked_workspace_bytes(B, N, D, k, items.size) < 64 << 20
    ued, ied, rpd, itd = T(ue, dev), T(ie, dev), T(rp, dev), T(items, dev)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    s, i = K.topk_dot_masked(ued, ied, k, rpd, itd)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 64 << 20     # a [B, N] slab would be 8.6 GB
    rows = np.sort(rng.choice(B, 64, replace=False))
    rs, ri = oracle(ue, ie, np.arange(B), hist, k, rows)
    assert np.array_equal(i.cpu().numpy()[rows], ri) and np.array_equal(s.cpu().numpy()[rows], rs)


class _Loader:
    def __init__(self, g):
        rows = lambda rp, it: [it[rp[u]:rp[u + 1]].tolist() for u in range(len(rp) - 1)]   # noqa: E731
        users = g["eval_users"].tolist()
        hist = rows(g["eval_hist_rowptr"], g["eval_hist_items"])
        gt = rows(g["eval_gt_rowptr"], g["eval_gt_items"])
        self.test_user_dict = {u: gt[i] for i, u in enumerate(users)}
        self.user_hist_dict = {u: hist[i] for i, u in enumerate(users)}
        self.train_user_dict = {int(u): self.user_hist_dict.get(int(u), []) for u in g["train_users"]}


def test_metric_eval_matches_reference_g17(dev):
    from ragraph_amd.edge_eval import Metric

    g = dict(np.load(os.path.join(GOLD, "g17_metric_eval.npz")))

    class Model:
        def generate(self):
            return T(g["user_emb"], dev), T(g["item_emb"], dev)

    dl = _Loader(g)
    m = Metric("recall;ndcg;precision", ";".join(str(k) for k in g["ks"]), int(g["eval_batch_size"]))
    for name in ("eval", "tuned", "untuned"):
        res = m.eval(Model(), dl) if name == "eval" else m.eval_grouped(Model(), dl, group=name)
        assert np.array_equal(m.last_ranked.cpu().numpy(), g[f"{name}_ranked"]), name
        assert list(res) == ["recall", "ndcg", "precision", "eval_time"]
        for mm in ("recall", "ndcg", "precision"):
            assert np.array_equal(res[mm], g[f"{name}_{mm}"]), (name, mm)
            assert np.allclose(m.last_values[mm], g[f"{name}_{mm}_raw"], rtol=0, atol=1e-9), (name, mm)


def _np_metrics(ranked, gt, ks, batch):
    n = len(gt)
    out = {mm: np.zeros(len(ks)) for mm in ("recall", "ndcg", "precision")}
    for s in range(0, n, batch):
        rk, g = ranked[s:s + batch], gt[s:s + batch]
        r = np.array([[float(x in gg) for x in row] for row, gg in zip(rk, g)])
        rn = np.array([len(gg) for gg in g])
        for t, k in enumerate(ks):
            right = r[:, :k].sum(1)
            disc = 1. / np.log2(np.arange(2, k + 2))
            idcg = np.array([disc[:min(k, len(gg))].sum() for gg in g])
            idcg[idcg == 0.] = 1.
            out["recall"][t] += np.sum(right / rn) / n
            out["ndcg"][t] += np.sum((r[:, :k] * disc).sum(1) / idcg) / n
            out["precision"][t] += np.sum(right) / k / n
    return out


def test_metric_eval_end_to_end_edge_list(dev, tmp_path):
    from ragraph_amd.edge_data import EdgeListData
    from ragraph_amd.edge_eval import Metric
    from ragraph_amd.RAGraph_edge import RAGraph as RAGraphEdge

    rng = np.random.default_rng(3)
    U, I, D = 150, 400, 64
    tr, te = [], []
    for u in range(U):
        if u < 120:
            its = rng.choice(I, int(rng.integers(1, 15)), replace=False)
            tms = np.sort(rng.integers(1_600_000_000, 1_600_500_000, its.size))
            tr.append(f"{u}\t{' '.join(map(str, its))}\t{' '.join(map(str, tms))}")
        if u % 3 != 2:
            te.append(f"{u}\t{' '.join(map(str, rng.choice(I, int(rng.integers(1, 6)), replace=False)))}")
    (tmp_path / "train.txt").write_text("\n".join(tr) + "\n")
    (tmp_path / "test.txt").write_text("\n".join(te) + "\n")
    ds = EdgeListData(str(tmp_path / "train.txt"), str(tmp_path / "test.txt"), num_users=U, num_items=I, device=dev)
    g = torch.Generator().manual_seed(4)
    ue0, ie0 = torch.randn(U, D, generator=g).to(dev), torch.randn(I, D, generator=g).to(dev)

    class Pre:
        def generate(self):
            return ue0.clone(), ie0.clone()

    model = RAGraphEdge(ds, Pre(), phase="finetune", use_RAG=True, retrieve_num=10, device=dev).eval()
    m = Metric("recall;ndcg;precision", "5;20", 64)
    res = m.eval(model, ds)
    with torch.no_grad():
        uo, io = model.generate()
    users = list(ds.test_user_dict.keys())
    hist = [ds.user_hist_dict[u] for u in users]
    ranked = pipeline.edge_topk_items(uo.cpu().numpy(), io.cpu().numpy(), np.array(users), hist, 20)
    assert np.array_equal(m.last_ranked.cpu().numpy(), ranked)
    ref = _np_metrics(ranked, [ds.test_user_dict[u] for u in users], [5, 20], 64)
    for mm, v in ref.items():
        assert np.allclose(m.last_values[mm], v, rtol=0, atol=1e-12), mm
        assert np.array_equal(res[mm], np.round(v, 6)), mm


def test_topk_dot_masked_rejects_bad_ids_without_writing(dev):
    from ragraph_amd import _native as N
    from ragraph_amd import kernels as K

    B, Nn, D, k = 40, 3000, 64, 10
    rng = np.random.default_rng(9)
    ue, ie = T(rng.standard_normal((B, D)).astype(np.float32), dev), T(rng.standard_normal((Nn, D)).astype(np.float32), dev)
    rp = T(np.arange(0, 2 * B + 1, 2, dtype=np.int64), dev)
    L = K._ready()
    for bad in (Nn, -1, Nn + 1000):
        items = rng.integers(0, Nn, 2 * B).astype(np.int64)
        items[17] = bad
        with pytest.raises(N.RagraphNativeError, match="history item id"):
            K.topk_dot_masked(ue, ie, k, rp, T(items, dev))
        # the raw entry point with a guard band behind both outputs: nothing is written on the error
        sc = torch.full((B * k + 4096,), 7.0, dtype=torch.float32, device=dev)
        ix = torch.full((B * k + 4096,), 7, dtype=torch.int64, device=dev)
        it = T(items, dev)
        ws = torch.empty(L.ragraph_topk_dot_masked_workspace_bytes(B, Nn, D, k, it.numel()), dtype=torch.uint8, device=dev)
        rc = L.ragraph_topk_dot_masked_f32(ue.data_ptr(), B, None, B, ie.data_ptr(), Nn, D, k, rp.data_ptr(), it.data_ptr(),
                                           it.numel(), ctypes.c_float(-1e8), sc.data_ptr(), ix.data_ptr(), ws.data_ptr(),
                                           ws.numel(), K._stream())
        torch.cuda.synchronize()
        assert rc == N.EINVAL
        assert bool((sc == 7.0).all()) and bool((ix == 7).all())
    with pytest.raises(N.RagraphNativeError, match="user id"):
        K.topk_dot_masked(ue, ie, k, rp, T(rng.integers(0, Nn, 2 * B), dev), users=T(np.full(B, B, np.int64), dev))
    with pytest.raises(N.RagraphNativeError, match="limit of 64"):
        K.topk_dot_masked(ue, ie, 65, rp, T(rng.integers(0, Nn, 2 * B), dev))
