"""Staged fine-tuning of the edge flavour on the device: kernels.interp_normalize against the composition of the entries
whose bits it promises (axpby chain + normalize_rows) with a guarded output buffer, against the reference's own result
(g20), interpolative_update's choice of keys, and two real stages of run_stages on g20's files."""
import os

import numpy as np
import pytest
import torch

from guarded_workspace import GuardedWorkspace

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g20_edge_stages.npz")
WEIGHTS = {1: [-0.75], 2: [0.5, -0.5], 3: [0.5, -0.5, 0.0], 8: [0.5, -0.5, 0.0, 0.25, -1.5, 1e-3, 2.0, 0.125]}


@pytest.fixture(scope="module")
def g20():
    return np.load(GOLDEN)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _tables(S, n, D, dev, seed):
    """S random tables; row 1 of table 0 is zero; row 2 mixes to exactly zero under WEIGHTS[S] (table 1 repeats table 0
    there under the opposite weight, every other table holds zeros); row 3 is zero in every table."""
    g = torch.Generator().manual_seed(seed)
    ts = [torch.randn(n, D, generator=g) for _ in range(S)]
    if n > 1:
        ts[0][1] = 0.0
    if n > 2:
        for s in range(S):
            ts[s][2] = ts[0][2] if s == 1 else (ts[s][2] if s == 0 else 0.0)
        if S == 1:
            ts[0][2] = 0.0
    if n > 3:
        for s in range(S):
            ts[s][3] = 0.0
    return [t.to(dev) for t in ts]


def _chain(tables, w):
    """The unnormalised mix through the entries the header names: T_0 * w_0 (mul), then axpby(acc, 1, T_s, w_s) -- for
    S >= 2 the first step is axpby(T_0, w_0, T_1, w_1)."""
    from ragraph_amd import kernels as K

    if len(tables) == 1:
        return K.mul(tables[0], torch.full_like(tables[0], w[0]))
    acc = K.axpby(tables[0], w[0], tables[1], w[1])
    for t, ws in zip(tables[2:], w[2:]):
        acc = K.axpby(acc, 1.0, t, ws)
    return acc


def _guarded_out(gw, n, D, dev):
    return gw(n * D * 4, dev).view(torch.float32).reshape(n, D)


@pytest.mark.parametrize("D", [1, 3, 64, 65, 256, 260])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_interp_normalize_has_the_bits_of_the_composition(S, D, dev):
    from ragraph_amd import kernels as K

    gw = GuardedWorkspace(fill=0xFF)
    for n in (1, 5, 1027):
        tables, w = _tables(S, n, D, dev, 100 * S + D + n), WEIGHTS[S]
        ref = K.normalize_rows(_chain(tables, w))
        out = K.interp_normalize(tables, w, out=_guarded_out(gw, n, D, dev))
        assert torch.equal(_bits(out), _bits(ref)), (S, D, n)
        assert not torch.isnan(out).any()
        if n > 3:
            assert not out[2].any() and not out[3].any()                    # a mix of exactly zero stays zero
            assert (out[1] == 0).all() == (S == 1)
        fresh = K.interp_normalize(tables, torch.tensor(w))                 # weights as a host tensor, out allocated
        assert torch.equal(_bits(fresh), _bits(ref))
    assert gw.check() == 3                                                  # no write outside n * D floats


@pytest.mark.parametrize("D", [1028, 1030])
def test_interp_normalize_long_rows_mix_twice(D, dev):
    """Rows of more than 256 chunks are not kept in registers: the second pass recomputes the mix."""
    from ragraph_amd import kernels as K

    gw = GuardedWorkspace(fill=0xA5)
    for S in (2, 8):
        tables, w = _tables(S, 5, D, dev, D + S), WEIGHTS[S]
        out = K.interp_normalize(tables, w, out=_guarded_out(gw, 5, D, dev))
        assert torch.equal(_bits(out), _bits(K.normalize_rows(_chain(tables, w)))), (S, D)
    assert gw.check() == 2


def test_interp_normalize_unaligned_tables_take_the_scalar_path(dev):
    from ragraph_amd import kernels as K

    n, D, S = 9, 64, 3
    g = torch.Generator().manual_seed(5)
    bufs = [torch.randn(n * D + 1, generator=g).to(dev) for _ in range(S)]
    tables = [b[1:].reshape(n, D) for b in bufs]                            # 4 bytes off a 16-byte boundary
    assert all(t.data_ptr() % 16 == 4 and t.is_contiguous() for t in tables)
    gw = GuardedWorkspace(fill=0xFF)
    out = K.interp_normalize(tables, WEIGHTS[S], out=_guarded_out(gw, n, D, dev))
    assert torch.equal(_bits(out), _bits(K.normalize_rows(_chain(tables, WEIGHTS[S]))))
    assert gw.check() == 1


def test_interp_normalize_wrapper_errors(dev):
    from ragraph_amd import kernels as K

    a, b = torch.ones(4, 8, device=dev), torch.ones(4, 8, device=dev)
    for bad in (lambda: K.interp_normalize([], []), lambda: K.interp_normalize([a] * 9, [1.0] * 9),
                lambda: K.interp_normalize([a, b], [1.0]), lambda: K.interp_normalize([a, torch.ones(4, 4, device=dev)], [1.0, 1.0]),
                lambda: K.interp_normalize([a, b.double()], [1.0, 1.0]), lambda: K.interp_normalize([a, b.cpu()], [1.0, 1.0]),
                lambda: K.interp_normalize([a, b], [1.0, 1.0], out=a),      # out aliases a table: refused by the entry
                lambda: K.interp_normalize([a, b], [1.0, 1.0], out=torch.empty(4, 4, device=dev))):
        with pytest.raises(K.RagraphNativeError):
            bad()
    assert K.interp_normalize([torch.empty(0, 8, device=dev)], [1.0]).shape == (0, 8)


@pytest.mark.parametrize("S", [2, 3])
def test_interp_normalize_against_the_reference(g20, S, dev):
    """g20: finetune_rag.py:70-86 executed by the reference on the CPU.  The unnormalised mix has its bits; the normalised
    result differs only by the norm's summation order."""
    from ragraph_amd import kernels as K
    from ragraph_amd.edge_train import interpolation_weights

    tables = [torch.from_numpy(g20["tables"][s]).to(dev) for s in range(S)]
    w = interpolation_weights(S - 1)
    mix = _chain(tables, w.tolist())
    assert np.array_equal(mix.cpu().numpy().view(np.uint32), g20[f"mix_{S}"].view(np.uint32))
    out = K.interp_normalize(tables, w)
    assert torch.equal(_bits(out), _bits(K.normalize_rows(mix)))
    assert np.allclose(out.cpu().numpy(), g20[f"out_{S}"], rtol=1e-6, atol=1e-7)
    assert not out[0].any()


def test_interpolative_update_takes_only_the_pretrained_tables(dev):
    from ragraph_amd import kernels as K
    from ragraph_amd.edge_train import interpolation_weights, interpolative_update

    g = torch.Generator().manual_seed(3)
    r = lambda *shape: torch.randn(*shape, generator=g)   # noqa: E731
    pre = {"user_embedding": r(5, 64), "item_embedding": r(7, 64).to(dev), "not_a_table": r(2, 2)}
    saved = [{"user_embedding": r(5, 64).to(dev), "item_embedding": r(7, 64).to(dev), "gating_weight": r(64, 64),
              "gating_bias": r(1, 64), "user_embedding_A": r(5, 16), "user_embedding_B": r(16, 64),
              "item_embedding_A": r(7, 16), "item_embedding_B": r(16, 64)} for _ in range(2)]
    out = interpolative_update(pre, saved, device=dev)
    assert sorted(out) == ["item_embedding", "user_embedding"]
    w = interpolation_weights(2)
    assert w.tolist() == [0.5, (0.5 * torch.tensor([1.0, 2.0]) / 3.0).flip(0).tolist()[0], (0.5 * torch.tensor([1.0]) / 3.0).item()]
    for k in out:                                                           # [pre, newest saved, oldest]
        ref = K.interp_normalize([pre[k].to(dev), saved[1][k], saved[0][k]], w)
        assert out[k].device.type == "cuda" and torch.equal(_bits(out[k]), _bits(ref)), k
    with pytest.raises(ValueError):
        interpolative_update(pre, [], device=dev)


def test_two_real_stages_on_g20(g20, tmp_path, dev):
    """run_stages end to end: D = 64, two epochs of batches of 8 per stage, device-drawn dropout.  Nothing here depends on
    how a training trajectory rounds."""
    from ragraph_amd.edge_data import EdgeListData
    from ragraph_amd.edge_eval import Metric
    from ragraph_amd.edge_train import interpolative_update, run_stages
    from ragraph_amd.RAGraph_edge import RAGraph

    files = {}
    for n in ("pretrain", "pretrain_val", "fine_tune", "test_1", "test_2"):
        p = tmp_path / f"{n}.txt"
        p.write_text(str(g20[f"{n}_txt"]))
        files[n] = str(p)
    K_RANK = 5      # 24 items: a ranking of 20 could not avoid a history of more than 4 items
    metric = Metric("recall;ndcg", str(K_RANK), 512)
    torch.manual_seed(20)
    pre_model = RAGraph(EdgeListData(files["pretrain"], files["pretrain_val"], device=dev), None, phase="pretrain", device=dev)
    pre_state = {k: v.detach().clone() for k, v in pre_model.state_dict().items()}
    assert sorted(pre_state) == ["item_embedding", "user_embedding"] and pre_state["user_embedding"].shape == (30, 64)
    seen = []

    def on_stage(stage, pre, model, trainer):
        ranked = trainer.metric.last_ranked.cpu().numpy()
        seen.append({"stage": stage, "pre": pre, "model": model, "trainer": trainer, "ranked": ranked,
                     "pre_tables": {k: v.detach().clone() for k, v in pre.state_dict().items()}})

    out = run_stages(files["pretrain"], files["pretrain_val"], files["fine_tune"], [files["test_1"], files["test_2"]], pre_state,
                     updt_inter=1, model_kwargs={"emb_size": 64, "dropout_rng": "device"},
                     trainer_kwargs={"num_epochs": 2, "batch_size": 8, "metric": metric}, device=dev, on_stage=on_stage)
    assert [s["stage"] for s in seen] == [1, 2] and len(out["states"]) == 2
    for s in seen:
        assert s["model"].dropout_rng == "device" and s["model"].phase == "finetune" and s["pre"].phase == "for_tune"
        assert not s["pre"].training
    # stage 1 starts from the raw pre-trained tables, stage 2 from their interpolative update with stage 1's best model
    for k in pre_state:
        assert torch.equal(_bits(seen[0]["pre_tables"][k]), _bits(pre_state[k])), k
    assert {"gating_weight", "gating_bias"} <= set(out["states"][0])
    upd = interpolative_update(pre_state, [out["states"][0]], device=dev)
    assert sorted(upd) == sorted(seen[1]["pre_tables"])
    for k in upd:
        assert torch.equal(_bits(seen[1]["pre_tables"][k]), _bits(upd[k])), k
        assert not torch.equal(upd[k], pre_state[k])
    # the returned recalls / ndcgs are the trainers' best_perform values
    assert out["recalls"] == [s["trainer"].best_perform["recall"][0] for s in seen]
    assert out["ndcgs"] == [s["trainer"].best_perform["ndcg"][0] for s in seen]
    assert all(r > 0 for r in out["recalls"])
    assert out["recall_mean"] == np.round(np.mean(out["recalls"]), 5)
    # the trainer's own last evaluation of stage 2: no item of a user's history, earlier files included, is ranked
    ds2, ranked = seen[1]["trainer"].dataloader, seen[1]["ranked"]
    assert ds2.phase == "finetune" and seen[1]["trainer"].metric is metric
    users = list(ds2.test_user_dict)
    assert ranked.shape == (len(users), K_RANK)
    earlier = False
    for row, u in zip(ranked, users):
        hist = set(ds2.user_hist_dict[u])
        assert ds2.num_items - len(hist) >= K_RANK, u                       # (enough unmasked items to fill the ranking)
        assert not hist & set(row.tolist()), (u, sorted(hist), row.tolist())
        earlier = earlier or bool(hist - set(ds2.train_user_dict.get(u, [])))
    assert earlier                                                          # some masked items come from earlier files only
