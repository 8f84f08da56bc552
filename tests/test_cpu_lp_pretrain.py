"""Link-prediction pre-training, host side: the g18 fixture (the reference's own sampler, forward and backward), a float64
restatement of compareloss against it, the sampler's rules on the reference's sample, and the new ABI entries."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g18_lp_pretrain.npz")
FLAVOURS = ("node", "graph")


@pytest.fixture(scope="module")
def g18():
    return np.load(GOLDEN)


def _compareloss_f64(h, t, temperature=1.5):
    """preprompt.py:80-103 in float64, with F.cosine_similarity's eps: x / max(||x||, 1e-8)."""
    h = h.astype(np.float64)
    hn = h / np.maximum(np.linalg.norm(h, axis=1, keepdims=True), 1e-8)
    sim = np.einsum("id,isd->is", hn, hn[t])
    e = np.exp(sim) / temperature
    return float(np.mean(-np.log(e[:, 0] / e[:, 1:].sum(axis=1))))


def test_g18_loads(g18):
    for f in FLAVOURS:
        n = g18[f"{f}_X"].shape[0]
        assert g18[f"{f}_sample"].shape == (n, 1 + int(g18[f"{f}_n_neg"]))
        assert g18[f"{f}_elu"].shape == (n, 256)
        for k in ("g_W", "g_bias", "g_alpha", "g_bn_weight", "g_bn_bias", "bn_running_mean", "bn_running_var"):
            assert np.isfinite(g18[f"{f}_{k}"]).all(), k
    assert int(g18["node_n_neg"]) == 100 and int(g18["graph_n_neg"]) == 50
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_compareloss_restated_matches_g18(g18, flavour):
    loss = _compareloss_f64(g18[f"{flavour}_elu"], g18[f"{flavour}_sample"].astype(np.int64))
    assert loss == pytest.approx(float(g18[f"{flavour}_loss"]), rel=1e-6)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_g18_sample_follows_the_sampler_rules(g18, flavour):
    rp, col = g18[f"{flavour}_raw_rowptr"], g18[f"{flavour}_raw_col"]
    t = g18[f"{flavour}_sample"].astype(np.int64)
    n, n_neg = t.shape[0], int(g18[f"{flavour}_n_neg"])
    assert ((t >= 0) & (t < n)).all()
    isolated = 0
    for i in range(n):
        nb = set(col[rp[i]:rp[i + 1]].tolist())
        if nb:
            assert t[i, 0] in nb
        else:
            assert t[i, 0] == i
            isolated += 1
        neg = t[i, 1:]
        assert len(set(neg.tolist())) == n_neg
        assert not (set(neg.tolist()) & nb)
    assert isolated >= 1


def test_lp_entries_in_header_and_bindings():
    from ragraph_amd import _native
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "ragraph_hip.h")).read()
    for name in ("ragraph_lp_workspace_bytes", "ragraph_lp_sample_i64", "ragraph_lp_compare_loss_fwd_f32",
                 "ragraph_lp_combine_f32"):
        assert name in _native.SIGNATURES and name + "(" in hdr


def test_preprompt_state_dict_unchanged():
    from ragraph_amd.preprompt import PrePrompt
    keys = set(PrePrompt(18, 256, "prelu", 1, 0.3).state_dict())
    assert keys == {"gcn.convs.0.fc.weight", "gcn.convs.0.act.weight", "gcn.convs.0.bias", "gcn.g_net.0.fc.weight",
                    "gcn.g_net.0.act.weight", "gcn.g_net.0.bias", "gcn.bns.0.weight", "gcn.bns.0.bias",
                    "gcn.bns.0.running_mean", "gcn.bns.0.running_var", "gcn.bns.0.num_batches_tracked"}
    assert "forward" in PrePrompt.__dict__
