"""tests/rowops_reference.py against torch itself, without a GPU: the restatements that tests/test_gpu_rowops_edges.py
holds the kernels to are checked here independently of the kernels -- the activation-gradient table against torch.autograd
of F.prelu / F.leaky_relu / F.elu / F.relu at the special points, the softmax and log-softmax gradients against float64
autograd, the time-rescale chain against RAGraph_edge's t.float(), subtract, divide."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rowops_reference as R

SLOPES = [0.25, 0.0, -0.3, 0.01, 0.5, 1.7]


def _table(seed=0):
    """The special points, twice (two upstream gradients of either sign at every point), inside ordinary values."""
    rng = np.random.default_rng(seed)
    z = np.concatenate([rng.standard_normal(7).astype(np.float32), R.SPECIAL_Z, rng.standard_normal(5).astype(np.float32),
                        R.SPECIAL_Z])
    gy = rng.standard_normal(z.size).astype(np.float32)
    gy[7:7 + R.SPECIAL_Z.size] = 2.0
    return z, gy


def test_issue_example_quarter_slope_at_zero():
    z = np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32)
    gy = np.full(4, 2.0, dtype=np.float32)
    for act in (R.ACT_PRELU, R.ACT_LEAKY):
        gz, _ = R.act_grad(z, gy, act, 0.25)
        assert gz.dtype == np.float32 and gz.tolist() == [0.5, 0.5, 2.0, 0.5]


@pytest.mark.parametrize("slope", SLOPES)
def test_prelu_gradient_table_matches_autograd(slope):
    z, gy = _table()
    zt = torch.from_numpy(z).reshape(1, -1).requires_grad_(True)
    # one slope per channel: the slope's gradient then arrives per element (the kernel's `alpha_terms`)
    at = torch.full((z.size,), slope, dtype=torch.float32, requires_grad=True)
    (F.prelu(zt, at) * torch.from_numpy(gy)).sum().backward()
    gz, terms = R.act_grad(z, gy, R.ACT_PRELU, slope)
    assert gz.dtype == np.float32 and np.array_equal(gz, zt.grad.numpy().reshape(-1))
    assert np.array_equal(terms.astype(np.float32), at.grad.numpy())
    assert np.array_equal(R.apply_act(z, R.ACT_PRELU, slope), F.prelu(zt, at).detach().numpy().reshape(-1))


@pytest.mark.parametrize("slope", SLOPES)
def test_leaky_relu_gradient_table_matches_autograd(slope):
    z, gy = _table(1)
    zt = torch.from_numpy(z).requires_grad_(True)
    (F.leaky_relu(zt, slope) * torch.from_numpy(gy)).sum().backward()
    gz, _ = R.act_grad(z, gy, R.ACT_LEAKY, slope)
    assert np.array_equal(gz, zt.grad.numpy())


def test_relu_gradient_table_matches_autograd():
    z, gy = _table(2)
    zt = torch.from_numpy(z).requires_grad_(True)
    (F.relu(zt) * torch.from_numpy(gy)).sum().backward()
    gz, _ = R.act_grad(z, gy, R.ACT_RELU)
    assert np.array_equal(gz, zt.grad.numpy())          # (gy * 0 is -0 for gy < 0, torch writes +0: equal as values)
    assert np.array_equal(R.apply_act(z, R.ACT_RELU), F.relu(zt).detach().numpy())


@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_elu_gradient_table_matches_autograd(alpha):
    z, gy = _table(3)
    z = np.concatenate([z, np.array([-20.0, -88.0, -104.0], dtype=np.float32)])
    gy = np.concatenate([gy, np.ones(3, dtype=np.float32)])
    zt = torch.from_numpy(z).double().requires_grad_(True)
    y = F.elu(zt, alpha)
    (y * torch.from_numpy(gy).double()).sum().backward()
    gz, _ = R.act_grad(z, gy, R.ACT_ELU, alpha)
    assert np.allclose(gz, zt.grad.numpy(), rtol=1e-12, atol=0)
    assert np.allclose(R.apply_act(z, R.ACT_ELU, alpha), y.detach().numpy(), rtol=1e-12, atol=0)
    # through the output, as the kernel is given it: y + alpha = alpha * exp(z) on the negative side
    assert np.allclose(R.elu_grad_from_output(y.detach().float().numpy(), gy, alpha), zt.grad.numpy(), rtol=0, atol=2e-7 * 3)
    # and fp32 torch agrees with the float64 table to fp32 rounding
    z32 = torch.from_numpy(z).requires_grad_(True)
    (F.elu(z32, alpha) * torch.from_numpy(gy)).sum().backward()
    assert np.allclose(z32.grad.numpy(), gz, rtol=1e-6, atol=1e-37)


@pytest.mark.parametrize("B,C", [(1, 1), (3, 2), (5, 70), (2, 1024)])
def test_softmax_and_log_softmax_gradients_match_autograd(B, C):
    rng = np.random.default_rng(B * 1000 + C)
    lg = (3 * rng.standard_normal((B, C))).astype(np.float32)
    lg[0, :] = 1.5                                     # equal logits
    if C > 2:
        lg[-1, 1] = -np.inf                            # a masked class
    go = rng.standard_normal((B, C)).astype(np.float32)
    rag = rng.random((B, C)).astype(np.float32)
    for scale in (1.0, 0.7):
        lt = torch.from_numpy(lg).double().requires_grad_(True)
        p = torch.softmax(lt, 1)
        (p * torch.from_numpy(go).double() * float(np.float32(scale))).sum().backward()
        assert np.allclose(R.softmax_grad(p.detach().numpy(), go, scale), lt.grad.numpy(), rtol=1e-12, atol=1e-15)
    lt = torch.from_numpy(lg).double().requires_grad_(True)
    lp = torch.log_softmax(lt, 1)
    (torch.where(torch.isinf(lp), torch.zeros_like(lp), lp) * torch.from_numpy(go).double()).sum().backward()
    gm = np.where(np.isinf(lg), np.float32(0), go)     # (no upstream gradient into a masked class: -inf * 0 otherwise)
    assert np.allclose(R.log_softmax_grad(lp.detach().numpy(), gm), lt.grad.numpy(), rtol=1e-12, atol=1e-15)
    # the forward restatement, both modes and the mix
    for lam in (0.0, 0.3, 1.0):
        ref = torch.softmax(torch.from_numpy(lg).double(), 1) * float(np.float32(1) - np.float32(lam)) + \
            torch.from_numpy(rag).double() * float(np.float32(lam))
        assert np.allclose(R.softmax_mix(lg, rag, lam), ref.numpy(), rtol=1e-12, atol=1e-15)
    got = R.softmax_mix(lg, None, 0.0, log_mode=True)
    assert np.array_equal(np.isneginf(got), np.isinf(lg)) and not np.isnan(got).any()
    fin = np.isfinite(got)
    assert np.allclose(got[fin], torch.log_softmax(torch.from_numpy(lg).double(), 1).numpy()[fin], rtol=1e-12, atol=1e-15)


def test_time_rescale_is_the_edge_flavours_chain():
    rng = np.random.default_rng(4)
    t = np.concatenate([rng.integers(1_690_000_000, 1_710_000_000, 200), rng.integers(-5000, 5000, 50),
                        np.array([2 ** 24 + 1, 2 ** 31 + 3, 2 ** 40 + 12345, -(2 ** 33) - 7])]).astype(np.int64)
    e = torch.from_numpy(t).float()                     # RAGraph_edge/modules/RAGraph.py:254-257
    ref = (e - e.min()) / (e.max() - e.min())
    got = R.time_rescale(t, float(t.min()), float(t.max()))
    assert got.dtype == np.float32 and R.same_bits(got, ref.numpy())
    # an explicit max_step, and the degenerate range
    ref = (e - e.min()) / (torch.tensor(2e9) - e.min())
    assert R.same_bits(R.time_rescale(t, float(t.min()), 2e9), ref.numpy())
    same = R.time_rescale(np.array([5, 7, 3]), 5.0, 5.0)
    assert np.isnan(same[0]) and same[1] == np.inf and same[2] == -np.inf


def test_bit_exact_restatements_are_torch_fp32():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(1000).astype(np.float32), rng.standard_normal(1000).astype(np.float32)
    a[:4] = [0.0, -0.0, 1e-40, -1e-45]
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    assert R.same_bits(R.axpby(a, 0.7, b, 0.3), (ta * 0.7 + tb * 0.3).numpy())
    w = rng.standard_normal(64).astype(np.float32)
    assert R.same_bits(R.axpby_dev(a, b, w, 63, 0), (ta * float(w[63]) + tb * float(w[0])).numpy())
    assert R.same_bits(R.axpby_dev(a, b, w, 0, -1), (ta * float(w[0]) + tb * 0.0).numpy())
    assert R.same_bits(R.mul(a, b), (ta * tb).numpy())
    x = rng.standard_normal((50, 20)).astype(np.float32)
    assert R.same_bits(R.mul_cols(x, w[:20]), (torch.from_numpy(x) * torch.from_numpy(w[:20])).numpy())
    ref = F.elu(torch.from_numpy(x).double() * torch.from_numpy(w[:20]).double())
    assert np.allclose(R.mul_cols(x, w[:20], R.ACT_ELU, 1.0), ref.numpy(), rtol=0, atol=1e-6)


def test_gate_rows_and_prototype_restatements():
    rng = np.random.default_rng(6)
    x, z, g = (rng.standard_normal(300).astype(np.float32) for _ in range(3))
    z[:6] = [88.0, -88.0, 104.0, -104.0, np.inf, -np.inf]
    xt, zt = torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(z).double().requires_grad_(True)
    out = xt * torch.sigmoid(zt)
    (out * torch.from_numpy(g).double()).sum().backward()
    assert np.allclose(R.sigmoid_gate(x, z), out.detach().numpy(), rtol=1e-12, atol=1e-300)
    gx, gz = R.sigmoid_gate_grad(x, z, g)
    assert np.allclose(gx, xt.grad.numpy(), rtol=1e-12, atol=1e-300)
    assert np.allclose(gz, zt.grad.numpy(), rtol=1e-9, atol=1e-300) and np.isfinite(gz).all()
    rp = np.array([0, 0, 3, 3, 4, 4])
    assert R.csr_row_ids(rp).tolist() == [1, 1, 1, 3]
    s = R.scatter_fill(np.zeros((5, 4)), rp, np.array([2, 0, 2, 1]), -1e8)
    assert (s != 0).sum() == 3 and s[1, 0] == s[1, 2] == s[3, 1] == np.float32(-1e8) and not s[:, 3].any()
    emb, proto = rng.standard_normal((9, 7)).astype(np.float32), rng.standard_normal((3, 7)).astype(np.float32)
    emb[1] = 0.0
    for mode in (0, 1, 2):
        cos = F.cosine_similarity(torch.from_numpy(emb).double()[:, None, :], torch.from_numpy(proto).double()[None], dim=-1,
                                  eps=1e-8)
        ref = cos if mode == 0 else (torch.softmax(cos, 1) if mode == 1 else torch.log_softmax(cos, 1))
        assert np.allclose(R.proto_cosine(emb, proto, mode), ref.numpy(), rtol=1e-12, atol=1e-15)
        out, gemb, gproto = R.proto_cosine(emb, proto, mode, rng.standard_normal((9, 3)).astype(np.float32))
        assert np.isfinite(gemb).all() and np.isfinite(gproto).all() and np.array_equal(out, R.proto_cosine(emb, proto, mode))
