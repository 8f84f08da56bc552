"""tests/autograd_reference.py checked on the host, independently of the kernels:
  * every lattice case of the table: the restatement in fp32 (torch-CPU, its own summation order) equals the float64 one bit
    for bit, no partial sum in ANY order can leave fp32's exact range (autograd_reference.exact_in_any_order on the absolute
    restatement), and no pre-activation is 0 -- so tests/test_gpu_autograd_edges.py may ask the device for equality;
  * every random-real case: the fp32 restatement stays within sum_bound of the float64 one, element by element -- the bound
    the device is held to is one that honest fp32 arithmetic meets;
  * every restatement agrees with numerical differentiation in double at one tiny shape: torch.autograd.gradcheck on a
    function that runs the restatement's own forward, and its returned gradients against the textbook expression."""
import pytest
import torch

import autograd_reference as AR

ACTS = (AR.ACT_RELU, AR.ACT_PRELU, AR.ACT_LEAKY)


def _keys(case):
    """What the device is compared on: the output, the gradients the case asks for (a slope gradient that is not requested
    is outside the exact range at the wide shapes) and the pre-activation."""
    return [k for k in case.ref if k in ("y", "z") or k in case.grads]


@pytest.mark.parametrize("cid", list(AR.LATTICE_CASES))
def test_lattice_case_is_exact_in_fp32(cid):
    case = AR.build(AR.LATTICE_CASES, cid)
    r32 = AR.reference(case, dtype=torch.float32)
    assert set(r32) == set(case.ref)
    for k in _keys(case):
        v = case.ref[k]
        assert r32[k].dtype == torch.float32 and torch.equal(r32[k].double(), v), (cid, k)
        assert AR.exact_in_any_order(case.abs[k], AR.LATTICE_UNITS.get(k, AR.LATTICE_UNIT)), (cid, k, float(case.abs[k].max()))
        assert torch.equal(v * 16, torch.round(v * 16)), (cid, k)                   # on the lattice
    if case.opt.get("act", AR.ACT_NONE) in ACTS:
        assert int((case.ref["z"] == 0).sum()) == 0, cid


@pytest.mark.parametrize("cid", list(AR.REAL_CASES))
def test_fp32_restatement_is_within_sum_bound(cid):
    case = AR.build(AR.REAL_CASES, cid)
    mask = case.ref["z"] > 0 if "z" in case.ref else None          # (one branch for both precisions)
    r32 = AR.reference(case, dtype=torch.float32, mask=mask)
    worst = 0.0
    for k in _keys(case):
        v = case.ref[k]
        bound = AR.sum_bound(case.L[k], case.abs[k])
        err = (r32[k].double() - v).abs()
        assert bool((err <= bound).all()), (cid, k, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((v.abs() <= case.abs[k] * (1 + 1e-12)).all()), (cid, k)        # the absolute restatement dominates
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    assert worst <= 1.0


def test_sum_bound_is_the_documented_formula():
    a = torch.tensor([[2.0, 0.0], [1.0, 4.0]])
    assert torch.equal(AR.sum_bound(3, a), 11 * 2.0 ** -24 * a.double())
    assert torch.equal(AR.sum_bound(torch.tensor([[0.0], [8.0]]), a), torch.tensor([[8.0], [16.0]], dtype=AR.F64) * 2.0 ** -24 * a)


def test_hub_graph_has_the_rows_the_table_asks_for():
    for mirror in (False, True):
        r, c, v = AR.hub_graph(4200, 5, seed=10, mirror=mirror)
        if mirror:
            r, c = c, r
        dr, dc = AR.degrees(r, 4200).reshape(-1), AR.degrees(c, 4200).reshape(-1)
        assert int(dr[7]) == 0 and int(dc[9]) == 0 and int(dc[0]) == 4199 and int(dr.max()) == 6
        assert 4096 < int(dc.max()) and r.numel() < 26000 and set(v.tolist()) == {1.0, 2.0, 3.0}
        assert not torch.equal(r, c)


# ---- gradcheck: the restatements themselves, in double, at tiny shapes ---------------------------------------------------
def _check(fn, *inputs):
    inputs = [t.double().requires_grad_(True) for t in inputs]
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-6, rtol=1e-5)


def _gradcheck_restatement(call, inputs, keys, go):
    """The restatement `call(*inputs, go)` itself against numerical differentiation: the gradients it RETURNS for
    sum(y * go) are handed to torch.autograd.gradcheck as the analytic side (a Function whose forward is the restatement's
    own output and whose backward is what the restatement returned), central differences of that forward on the other."""
    go = go.double()

    class Restated(torch.autograd.Function):
        @staticmethod
        def forward(ctx, *xs):
            with torch.enable_grad():        # (the restatement differentiates inside)
                r = call(*[x.detach() for x in xs], go)
            ctx.grads = [r[k].reshape(x.shape) for k, x in zip(keys, xs)]
            return (r["y"] * go.expand_as(r["y"])).sum()

        @staticmethod
        def backward(ctx, g):
            return tuple(g * gr for gr in ctx.grads)

    xs = [t.double().requires_grad_(True) for t in inputs]
    assert torch.autograd.gradcheck(Restated.apply, xs, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_every_restatement_passes_gradcheck():
    g = AR.gauss
    x, w, b = g((5, 3), 1), g((4, 3), 2), g(4, 3)
    for act, alpha in ((AR.ACT_NONE, 0.0), (AR.ACT_LEAKY, 0.25), (AR.ACT_LEAKY, -0.5)):
        _gradcheck_restatement(lambda x_, w_, b_, go: AR.linear(x_, w_, b_, go, act, alpha), (x, w, b), ("gx", "gw", "gb"), g((5, 4), 4))
    xs, bs, al = g((4, 3), 5), g(3, 6), torch.tensor([-0.5])
    _gradcheck_restatement(lambda x_, b_, a_, go: AR.spmm_csr(COO, 4, x_, b_, go, AR.ACT_PRELU, a_), (xs, bs, al),
                           ("gx", "gb", "galpha"), g((4, 3), 7))
    _gradcheck_restatement(lambda x_, b_, go: AR.spmm_csr(COO, 4, x_, b_, go, AR.ACT_RELU), (xs, bs), ("gx", "gb"), g((4, 3), 7))
    rows = torch.tensor([3, 1, 3, 0])
    _gradcheck_restatement(lambda x_, go: AR.spmm_csr_rows(COO, 4, x_, rows, go), (xs,), ("gx",), g((4, 3), 8))
    a, b2, go2 = g((3, 5), 9), g((3, 5), 10), g((3, 5), 11)
    _gradcheck_restatement(lambda a_, b_, go: AR.axpby(a_, -2.0, b_, 0.5, go), (a, b2), ("ga", "gb"), go2)
    _gradcheck_restatement(lambda a_, b_, w_, go: AR.mix2(a_, b_, w_, go), (a, b2, torch.tensor([[0.75, -0.5]])),
                           ("ga", "gb", "gw"), go2)
    for act, alpha in ((AR.ACT_NONE, 0.0), (AR.ACT_RELU, 0.0), (AR.ACT_PRELU, 0.25), (AR.ACT_ELU, 1.0)):
        _gradcheck_restatement(lambda x_, w_, go: AR.mul_cols(x_, w_, go, act, alpha), (a, g(5, 12)), ("gx", "gw"), go2)
    idx = torch.tensor([2, 0, 2, 2])
    _gradcheck_restatement(lambda v_, go: AR.gather_rows(v_, idx, go), (a,), ("gv",), g((4, 5), 13))
    ptr = torch.tensor([0, 0, 2, 2, 3])
    _gradcheck_restatement(lambda x_, go: AR.segment_sum(x_, ptr, go), (a,), ("gx",), g((4, 5), 14))
    _gradcheck_restatement(lambda x_, z_, go: AR.sigmoid_gate(x_, z_, go), (a, b2), ("gx", "gz"), go2)
    rag = torch.rand(3, 5, generator=torch.Generator().manual_seed(4))
    _gradcheck_restatement(lambda l_, go: AR.softmax_mix(l_, rag, 0.5, go), (a,), ("glogits",), go2)
    _gradcheck_restatement(lambda l_, go: AR.softmax_mix(l_, None, 0.0, go), (a,), ("glogits",), go2)
    emb, proto = g((6, 5), 5), g((3, 5), 6)
    for mode in (0, 1, 2):
        _gradcheck_restatement(lambda e_, p_, go: AR.proto_cosine(e_, p_, mode, go), (emb, proto), ("gemb", "gproto"), g((6, 3), 7))
    t = torch.tensor([[1, 2, 3], [0, 0, 4], [2, 1, 0], [4, 4, 4], [3, 0, 1]])
    _gradcheck_restatement(lambda h_, go: AR.compare_loss(h_, t, 1.5, go), (g((5, 4), 8),), ("gh",), torch.tensor(1.0))


def _same(ref, keys, autograd_grads):
    for k, g in zip(keys, autograd_grads):
        torch.testing.assert_close(ref[k], g, rtol=1e-12, atol=1e-12)


def _plain(f, go, *inputs):
    """Output and gradients of the textbook expression f under torch.autograd in double."""
    leaves = [t.double().requires_grad_(True) for t in inputs]
    y = f(*leaves)
    return y.detach(), torch.autograd.grad(y, leaves, go.double().expand_as(y))


COO = (torch.tensor([0, 0, 2, 3, 3, 3]), torch.tensor([1, 3, 0, 0, 2, 3]), torch.tensor([1.0, 2.0, 0.5, 3.0, 1.5, 0.25]))


def _dense(coo, n):
    return torch.zeros(n, n, dtype=AR.F64).index_put_((coo[0], coo[1]), coo[2].double(), accumulate=True)


def test_restatements_agree_with_textbook_autograd():
    import torch.nn.functional as F
    g = AR.gauss
    x, w, b, go = g((5, 3), 1), g((4, 3), 2), g(4, 3), g((5, 4), 4)
    for act, alpha, f in ((AR.ACT_NONE, 0.0, lambda t: t), (AR.ACT_LEAKY, 0.25, lambda t: F.leaky_relu(t, 0.25)),
                          (AR.ACT_LEAKY, -0.5, lambda t: F.leaky_relu(t, -0.5)), (AR.ACT_RELU, 0.0, torch.relu)):
        r = AR.linear(x, w, b, go, act, alpha)
        y, gs = _plain(lambda x_, w_, b_: f(F.linear(x_, w_, b_)), go, x, w, b)
        torch.testing.assert_close(r["y"], y, rtol=1e-12, atol=1e-12)
        _same(r, ("gx", "gw", "gb"), gs)
    _check(lambda x_, w_, b_: F.linear(x_, w_, b_), x, w, b)
    # spmm_csr against the dense product, slope as a tensor
    A = _dense(COO, 4)
    xs, bs, gs_, al = g((4, 3), 5), g(3, 6), g((4, 3), 7), torch.tensor([-0.5])
    r = AR.spmm_csr(COO, 4, xs, bs, gs_, AR.ACT_PRELU, al)
    y, gr = _plain(lambda x_, b_, a_: F.prelu(A @ x_ + b_, a_), gs_, xs, bs, al)
    torch.testing.assert_close(r["y"], y, rtol=1e-12, atol=1e-12)
    _same(r, ("gx", "gb", "galpha"), gr)
    _check(lambda x_, b_, a_: F.prelu(A @ x_ + b_, a_), xs, bs, al)
    rows = torch.tensor([3, 1, 3, 0])
    r = AR.spmm_csr_rows(COO, 4, xs, rows, g((4, 3), 8))
    y, gr = _plain(lambda x_: (A @ x_)[rows], g((4, 3), 8), xs)
    torch.testing.assert_close(r["y"], y, rtol=1e-12, atol=1e-12)
    _same(r, ("gx",), gr)
    # axpby, mix2, mul_cols, gather, segment sum
    a, b2, go2 = g((3, 5), 9), g((3, 5), 10), g((3, 5), 11)
    r = AR.axpby(a, -2.0, b2, 0.5, go2)
    _same(r, ("ga", "gb"), _plain(lambda a_, b_: a_ * -2.0 + b_ * 0.5, go2, a, b2)[1])
    wm = torch.tensor([[0.75, -0.5]])
    r = AR.mix2(a, b2, wm, go2)
    _same(r, ("ga", "gb", "gw"), _plain(lambda a_, b_, w_: a_ * w_[0, 0] + b_ * w_[0, 1], go2, a, b2, wm)[1])
    wc = g(5, 12)
    for act, alpha, f in ((AR.ACT_NONE, 0.0, lambda t: t), (AR.ACT_PRELU, 0.25, lambda t: F.leaky_relu(t, 0.25)),
                          (AR.ACT_ELU, 1.0, F.elu)):
        r = AR.mul_cols(a, wc, go2, act, alpha)
        y, gr = _plain(lambda x_, w_: f(x_ * w_), go2, a, wc)
        torch.testing.assert_close(r["y"], y, rtol=1e-12, atol=1e-12)
        _same(r, ("gx", "gw"), gr)
    idx = torch.tensor([2, 0, 2, 2])
    r = AR.gather_rows(a, idx, g((4, 5), 13))
    _same(r, ("gv",), _plain(lambda v_: v_[idx], g((4, 5), 13), a)[1])
    assert torch.equal(r["gv"][1], torch.zeros(5, dtype=AR.F64))
    ptr = torch.tensor([0, 0, 2, 2, 3])
    r = AR.segment_sum(a, ptr, g((4, 5), 14))
    y, gr = _plain(lambda x_: torch.stack([x_[0:0].sum(0), x_[0:2].sum(0), x_[2:2].sum(0), x_[2:3].sum(0)]), g((4, 5), 14), a)
    torch.testing.assert_close(r["y"], y, rtol=1e-12, atol=1e-12)
    _same(r, ("gx",), gr)


def test_transcendental_restatements_agree_with_textbook_autograd():
    import torch.nn.functional as F
    g = AR.gauss
    x, z, go = g((4, 3), 1), g((4, 3), 2), g((4, 3), 3)
    _same(AR.sigmoid_gate(x, z, go), ("gx", "gz"), _plain(lambda x_, z_: x_ * torch.sigmoid(z_), go, x, z)[1])
    _check(lambda x_, z_: x_ * torch.sigmoid(z_), x, z)
    rag = torch.rand(4, 3, generator=torch.Generator().manual_seed(4))
    r = AR.softmax_mix(x, rag, 0.5, go)                     # (0.5: 1 - lam is the same number in fp32 and double)
    y, gr = _plain(lambda l_: torch.softmax(l_, 1) * 0.5 + rag.double() * 0.5, go, x)
    torch.testing.assert_close(r["y"], y, rtol=1e-12, atol=1e-12)
    _same(r, ("glogits",), gr)
    emb, proto, gp = g((6, 5), 5), g((3, 5), 6), g((6, 3), 7)
    for mode, f in ((0, lambda c: c), (1, lambda c: torch.softmax(c, 1)), (2, lambda c: torch.log_softmax(c, 1))):
        r = AR.proto_cosine(emb, proto, mode, gp)
        y, gr = _plain(lambda e_, p_: f(F.cosine_similarity(e_[:, None, :], p_[None, :, :], dim=-1, eps=1e-8)), gp, emb, proto)
        torch.testing.assert_close(r["y"], y, rtol=1e-12, atol=1e-12)
        _same(r, ("gemb", "gproto"), gr)
    h, t = g((5, 4), 8), torch.tensor([[1, 2, 3], [0, 0, 4], [2, 1, 0], [4, 4, 4], [3, 0, 1]])

    def chain(h_):   # preprompt.py's op chain (tests/test_gpu_lp_pretrain.py: _ref_compareloss)
        n, S = t.shape
        sim = F.cosine_similarity(h_[:, None, :].expand(n, S, -1), h_[t.reshape(-1)].reshape(n, S, -1), dim=2)
        e = (torch.exp(sim) / 1.5).permute(1, 0)
        return (-1 * torch.log(e[0].reshape(-1, 1) / e[1:].permute(1, 0).sum(dim=1, keepdim=True))).mean()
    r = AR.compare_loss(h, t, 1.5, torch.tensor(1.0))
    y, gr = _plain(chain, torch.tensor(1.0), h)
    torch.testing.assert_close(r["y"], y, rtol=1e-12, atol=1e-12)
    _same(r, ("gh",), gr)
    _check(chain, h)
