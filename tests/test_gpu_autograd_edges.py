"""The twelve autograd functions of ragraph_amd/autograd.py, backward included, at the shapes where their host-side switches
flip (LINEAR_TN_MIN_ROWS, COLSUM_SINGLE_MAX / COLSUM_ROWS, ROW_BLOCK on the transposed graph, the three lane-group widths),
for every subset of inputs that asks for a gradient and for every way autograd hands a gradient over -- against the float64
restatements of tests/autograd_reference.py (which tests/test_cpu_autograd_reference.py checks without a GPU).

  * lattice cases: output and every gradient EQUAL the float64 reference (no tolerance: every sum is exact in any order);
  * random-real cases (the sum / product family): every element within autograd_reference.sum_bound of float64, the
    activation's branch taken from the device's own saved tensor (y, or z when the forward keeps z), and that branch equal
    to z64 > 0 wherever |z64| exceeds the forward's bound;
  * transcendental functions: float64 under the tolerance the existing test of the same kernel uses (named per test);
  * every case: a second run gives the same bits.
All through the A.* entry points."""
import numpy as np
import pytest
import torch

import autograd_reference as AR
import rowops_reference as R

pytestmark = pytest.mark.gpu

SAVED_BRANCH = {"linear": 2, "spmm_csr": 0, "mul_cols": 2}      # which saved tensor of the Function carries the branch's sign
_graphs = {}


def _graph(case, dev):
    from ragraph_amd.graph import CSRGraph
    r, c, v = case.inp["coo"]
    key = (id(v), str(dev))
    if key not in _graphs:
        _graphs[key] = (CSRGraph.from_coo(r.to(dev), c.to(dev), v.to(dev), case.inp["n"])[0], v)
    return _graphs[key][0]


def _call(case, t, dev):
    from ragraph_amd import autograd as A
    o = case.opt
    if case.fn == "linear":
        return A.linear(t["x"], t["w"], t.get("b"), o["act"], o["alpha"])
    if case.fn == "axpby":
        return A.axpby(t["a"], o["wa"], t["b"], o["wb"])
    if case.fn == "spmm_csr":
        return A.spmm_csr(_graph(case, dev), t["x"], t.get("b"), o["act"], t.get("alpha"), None if o["mode"] == "dev" else o["alpha"])
    if case.fn == "spmm_csr_rows":
        return A.spmm_csr_rows(_graph(case, dev), t["x"], t["rows"])
    if case.fn == "gather_rows":
        return A.gather_rows(t["v"], t["idx"])
    if case.fn == "segment_sum":
        return A.segment_sum(t["x"], t["ptr"])
    if case.fn == "mix2":
        return A.mix2(t["a"], t["b"], t["w"])
    if case.fn == "mul_cols":
        return A.mul_cols(t["x"], t["w"], o["act"], o["alpha"])
    if case.fn == "sigmoid_gate":
        return A.sigmoid_gate(t["x"], t["z"])
    if case.fn == "softmax_mix":
        return A.softmax_mix(t["logits"], t.get("rag"), o["lam"])
    if case.fn == "proto_cosine":
        return A.proto_cosine(t["emb"], t["proto"], o["mode"])
    if case.fn == "compare_loss":
        return A.compare_loss(t["h"], t["tuples"], o["T"])
    raise ValueError(case.fn)


def run(case, dev, req, backward=None):
    """case.fn through ragraph_amd.autograd with the inputs named in `req` requiring a gradient; backward(y) (default: the
    case's own dense gradient).  -> {"y", the requested gradients, "branch": pre-activation > 0 as the device saved it}."""
    t = {k: v.to(dev).requires_grad_(k in req) if v.dtype == torch.float32 else v.to(dev)
         for k, v in case.inp.items() if torch.is_tensor(v)}
    y = _call(case, t, dev)
    assert y.grad_fn is not None and type(y.grad_fn).__name__.startswith("_"), "not on the autograd.Function path"
    out = {"y": y.detach()}
    if case.opt.get("act", AR.ACT_NONE) != AR.ACT_NONE:
        out["branch"] = (y.grad_fn.saved_tensors[SAVED_BRANCH[case.fn]] > 0).cpu()
    if backward is None:
        y.backward(case.go.to(dev).reshape(y.shape))
    else:
        backward(y)
    for k, name in case.grads.items():
        if name in req:
            assert t[name].grad is not None and t[name].grad.shape == t[name].shape, (k, name)
            out[k] = t[name].grad
        else:
            assert t[name].grad is None, (k, name)
    return out


def subsets(case):
    """Every differentiable input alone, then all of them."""
    names = list(case.grads.values())
    return [(n,) for n in names] + ([tuple(names)] if len(names) > 1 else [])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def assert_equals_reference(out, ref, what):
    for k, v in out.items():
        if k != "branch":
            got = v.double().cpu()
            assert torch.equal(got, ref[k].reshape(got.shape)), (what, k, int((got != ref[k].reshape(got.shape)).sum()))


def assert_repeats(case, dev, first, req):
    again = run(case, dev, req)
    for k, v in first.items():
        assert same_bits(v, again[k]) if k != "branch" else torch.equal(v, again[k]), k


def test_hub_graphs_cross_the_long_row_switch_where_the_table_says(dev):
    """The hub graph has no long row and its transposed graph has one; the mirror graph the reverse -- the two facts
    _SpmmCsr.forward and .backward read separately."""
    from ragraph_amd import kernels as K
    for name, fwd, bwd in (("hub", False, True), ("mirror", True, False)):
        g = _graph(AR.build(AR.LATTICE_CASES, f"spmm-{name}-D8-act0-0.0-bias1-host-ga0"), dev)
        assert int((g.rowptr[1:] - g.rowptr[:-1]).max()) == (4199 if fwd else 6) and 4199 > K.ROW_BLOCK
        assert g.has_long_rows is fwd and g.transposed().has_long_rows is bwd, name


# ---- (a) lattice --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(AR.LATTICE_CASES))
def test_lattice_equals_float64(dev, cid):
    case = AR.build(AR.LATTICE_CASES, cid)
    for req in subsets(case):
        out = run(case, dev, req)
        assert_equals_reference(out, case.ref, (cid, req))
        if "branch" in out:
            assert torch.equal(out["branch"], case.ref["z"] > 0), (cid, req)
    assert_repeats(case, dev, out, req)


# ---- (b) random-real ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(AR.REAL_CASES))
def test_real_within_sum_bound(dev, cid):
    case = AR.build(AR.REAL_CASES, cid)
    ref = None
    for req in subsets(case):
        out = run(case, dev, req)
        if ref is None:
            ref = case.ref
            if "branch" in out:         # the device's branch; it must be z64's wherever z64 is clear of the forward's error
                branch = out["branch"]
                clear = case.ref["z"].abs() > AR.sum_bound(case.L["z"], case.abs["z"])
                assert torch.equal(branch[clear], (case.ref["z"] > 0)[clear]), cid
                ref = AR.reference(case, mask=branch)
        elif "branch" in out:
            assert torch.equal(out["branch"], branch), cid
        for k, v in out.items():
            if k == "branch":
                continue
            got = v.double().cpu()
            err = (got - ref[k].reshape(got.shape)).abs()
            bound = AR.sum_bound(case.L[k], case.abs[k]).reshape(got.shape)
            assert bool((err <= bound).all()), (cid, req, k, float((err / bound.clamp_min(1e-300)).max()), int((err > bound).sum()))
    assert_repeats(case, dev, out, req)


# ---- the cases of the table that are statements of their own ----------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3, 7, 30, 66])
def test_gather_rows_unhit_rows_get_exact_zeros(dev, D):
    case = AR.build(AR.LATTICE_CASES, f"gather-300-300-{D}")
    gv = run(case, dev, ("v",))["gv"]
    unhit = AR.degrees(case.inp["idx"], 300).reshape(-1) == 0
    assert int(unhit.sum()) == 150
    assert same_bits(gv[unhit.to(dev)], torch.zeros(150, D, device=dev))           # +0, not -0, nothing left behind


def test_gather_rows_empty_index_gives_a_zero_gradient(dev):
    from ragraph_amd import autograd as A
    for D in (7, 64):
        v = AR.ints((10, D), 30).to(dev).requires_grad_(True)
        y = A.gather_rows(v, torch.zeros(0, dtype=torch.int64, device=dev))
        assert y.shape == (0, D)
        y.sum().backward()
        assert same_bits(v.grad, torch.zeros(10, D, device=dev))


def test_gather_rows_backward_at_width_64_keeps_the_unpadded_path_bits(dev):
    """D in 4Z: the gradient is the SpMM over the hit pattern on the gradient as it is -- no padding, no copy, no other bit."""
    from ragraph_amd import kernels as K
    from ragraph_amd.graph import CSRGraph
    case = AR.build(AR.REAL_CASES, "gather-50-7-64")
    gv = run(case, dev, ("v",))["gv"]
    idx, m = case.inp["idx"].to(dev), 7
    hits, _ = CSRGraph.from_coo(idx, torch.arange(m, device=dev), torch.ones(m, device=dev), 50)
    assert same_bits(gv, K.spmm_csr(hits.rowptr, hits.col, hits.val, case.go.to(dev)))


def test_fewshot_mean_logits_chain_at_width_7(dev):
    """segment_sum(gather_rows(x, perm), ptr) exactly as ragraph_utils.utility.fewshot_mean_logits builds it: a 7-class logit
    table (a width outside 4Z through the gather's backward), lattice logits, counts that divide exactly (1, 2, 4, 8 ...)."""
    from ragraph_amd.ragraph_utils.utility import fewshot_mean_logits
    counts = [1, 2, 4, 8, 16, 4, 2]
    labels = torch.repeat_interleave(torch.arange(7), torch.tensor(counts))
    labels = labels[torch.randperm(labels.numel(), generator=torch.Generator().manual_seed(31))]
    x = AR.ints((labels.numel(), 7), 32)
    go = AR.ints((7, 7), 33)
    xd = x.to(dev).requires_grad_(True)
    out = fewshot_mean_logits(xd, labels.to(dev))
    out.backward(go.to(dev))
    x64 = x.double().requires_grad_(True)
    ref = torch.zeros(7, 7, dtype=AR.F64).index_add_(0, labels, x64) / torch.tensor(counts, dtype=AR.F64)[:, None]
    ref.backward(go.double())
    assert torch.equal(out.detach().double().cpu(), ref.detach()) and torch.equal(xd.grad.double().cpu(), x64.grad)
    # and the bare chain on an unsorted lattice input, segments with a leading and a trailing empty one
    from ragraph_amd import autograd as A
    perm = torch.randperm(37, generator=torch.Generator().manual_seed(34))
    ptr = torch.tensor([0, 0, 5, 36, 37, 37])
    x, go = AR.ints((37, 7), 35), AR.ints((5, 7), 36)
    xd = x.to(dev).requires_grad_(True)
    y = A.segment_sum(A.gather_rows(xd, perm.to(dev)), ptr.to(dev))
    y.backward(go.to(dev))
    x64 = x.double().requires_grad_(True)
    r = AR.segment_sum(x64[perm].detach(), ptr, go)
    assert torch.equal(y.detach().double().cpu(), r["y"])
    gx = torch.zeros(37, 7, dtype=AR.F64).index_add_(0, perm, r["gx"])
    assert torch.equal(xd.grad.double().cpu(), gx)


# ---- transcendental functions: structure, the existing tolerances -------------------------------------------------------
def _np(t):
    return t.detach().double().cpu().numpy()


def _transcendental(fn, inp, opt, go, grads):
    case = AR.Case(fn, inp, opt, go, grads, {}, False)
    case.ref = AR.reference(case)
    return case


@pytest.mark.parametrize("req", [("x",), ("z",), ("x", "z")])
def test_sigmoid_gate_subsets(dev, req):
    """x only, z only, both -- R.close (1e-4 of the largest entry), as test_gpu_rowops_edges holds ragraph_sigmoid_gate*_f32."""
    case = _transcendental("sigmoid_gate", {"x": AR.gauss((300, 64), 40), "z": 3 * AR.gauss((300, 64), 41)}, {},
                           AR.gauss((300, 64), 42), {"gx": "x", "gz": "z"})
    out = run(case, dev, req)
    for k, v in out.items():
        assert R.close(_np(v), case.ref[k].numpy()), k
    assert_repeats(case, dev, out, req)


@pytest.mark.parametrize("rag,lam", [(False, 0.3), (True, 1.0), (True, 0.3)])
def test_softmax_mix_without_labels_and_at_lambda_one(dev, rag, lam):
    """rag_label = None (plain softmax), lam = 1 (the gradient is 0 * ...: exact zeros), and the ordinary mix -- R.close, as
    test_gpu_rowops_edges holds ragraph_softmax_mix_f32 / ragraph_softmax_grad_f32."""
    inp = {"logits": 4 * AR.gauss((40, 7), 43)}
    if rag:
        inp["rag"] = torch.rand(40, 7, generator=torch.Generator().manual_seed(44))
    case = _transcendental("softmax_mix", inp, {"lam": lam}, AR.gauss((40, 7), 45), {"glogits": "logits"})
    out = run(case, dev, ("logits",))
    assert R.close(_np(out["y"]), case.ref["y"].numpy()) and R.close(_np(out["glogits"]), case.ref["glogits"].numpy())
    if lam == 1.0:
        assert not out["glogits"].any()
    assert_repeats(case, dev, out, ("logits",))


@pytest.mark.parametrize("n,D", [(1, 1), (300, 3), (2049, 256)])
def test_mul_cols_elu(dev, n, D):
    """ELU through mul_cols: R.close, as test_gpu_rowops_edges holds mul_cols / act_grad with ACT_ELU; gw crosses
    COLSUM_SINGLE_MAX at 2049 rows."""
    case = _transcendental("mul_cols", {"x": AR.gauss((n, D), 46), "w": AR.gauss(D, 47)}, {"act": AR.ACT_ELU, "alpha": 1.0},
                           AR.gauss((n, D), 48), {"gx": "x", "gw": "w"})
    for req in subsets(case):
        out = run(case, dev, req)
        for k, v in out.items():
            if k != "branch":
                assert R.close(_np(v), case.ref[k].numpy().reshape(v.shape)), (req, k)
    assert_repeats(case, dev, out, req)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("req", [("emb",), ("proto",), ("emb", "proto")])
def test_proto_cosine_subsets(dev, req, mode):
    """emb only, proto only, both, at C * D = 8192 (the prototype gradient's LDS limit) -- R.close and, row by row,
    R.proto_cosine_grad_bounds, as test_proto_cosine_zero_norm_rows holds the kernels."""
    G, C, D = 257, 64, 128
    emb, proto, go = AR.gauss((G, D), 49), AR.gauss((C, D), 50), AR.gauss((G, C), 51)
    case = _transcendental("proto_cosine", {"emb": emb, "proto": proto}, {"mode": mode}, go, {"gemb": "emb", "gproto": "proto"})
    out = run(case, dev, req)
    assert R.close(_np(out["y"]), case.ref["y"].numpy())
    bounds = dict(zip(("gemb", "gproto"), R.proto_cosine_grad_bounds(emb.numpy(), proto.numpy(), go.numpy(),
                                                                     case.ref["gemb"].numpy(), case.ref["gproto"].numpy())))
    for k in ("gemb", "gproto"):
        if k in out:
            assert R.close(_np(out[k]), case.ref[k].numpy()), k
            err = np.abs(_np(out[k]) - case.ref[k].numpy())
            assert (err <= bounds[k]).all(), (k, float((err / bounds[k]).max()))
    assert_repeats(case, dev, out, req)


def _compare_hub_case(positive="hub"):
    n, S, D = 200, 30, 64
    h = AR.gauss((n, D), 52)
    h[5] = 0.0                                                     # one zero row
    t = torch.zeros(n, S, dtype=torch.int64)
    if positive == "ring":
        t[:, 0] = (torch.arange(n) + 1) % n
    return _transcendental("compare_loss", {"h": h, "tuples": t}, {"T": 1.5}, torch.tensor(1.0), {"gh": "h"})


@pytest.mark.parametrize("positive", ["hub", "ring"])
def test_compare_loss_with_a_hub(dev, positive):
    """Every slot of every row points at row 0: 6000 > ROW_BLOCK transposed entries in one row of the own + transposed pattern,
    and one zero row of h.  rtol = 1e-4, atol = 1e-5 * scale, as test_compare_loss_matches_torch_chain (the zero row to its
    own scale, as there).
    "hub", the case as stated: with every partner the same row, e_i0 / sum_s e_is = 1 / (S - 1) whatever h is -- the loss is
    log(S - 1) and its gradient is exactly 0, the positive slot's term cancelling the negatives'.  The largest entry of the
    float64 gradient (1e-18 of round-off) is then no scale; the scale is the largest entry of ONE of the two terms that cancel,
    the float64 gradient of the positive slots' part mean_i -cos(h_i, h_0).  Measured on the MI355X: the device gradient's
    largest entry is 6.9e-10.
    "ring": the positive of row i is row i + 1 instead, the 5800 > ROW_BLOCK negatives stay on row 0 -- a gradient that does
    not cancel, held to its own largest entry exactly as the existing test does."""
    import torch.nn.functional as F
    case = _compare_hub_case(positive)
    out = run(case, dev, ("h",))
    ref = case.ref
    assert float(out["y"]) == pytest.approx(float(ref["y"]), rel=1e-5)
    got, want = out["gh"].double().cpu(), ref["gh"]
    assert torch.isfinite(got).all()
    scale = want
    if positive == "hub":
        assert float(ref["y"]) == pytest.approx(float(np.log(29.0)), rel=1e-12)
        h64 = case.inp["h"].double().requires_grad_(True)
        (-F.cosine_similarity(h64, h64[:1].expand_as(h64), dim=1)).mean().backward()
        scale = h64.grad
        assert float(want.abs().max()) < 1e-12 * float(scale.abs().max())
    rest = torch.ones(200, dtype=torch.bool)
    rest[5] = False
    torch.testing.assert_close(got[rest], want[rest], rtol=1e-4, atol=1e-5 * float(scale[rest].abs().max()))
    torch.testing.assert_close(got[5], want[5], rtol=1e-4, atol=1e-5 * float(scale[5].abs().max()))
    assert_repeats(case, dev, out, ("h",))


# ---- how the gradient arrives -------------------------------------------------------------------------------------------
def _arrival_cases():
    L = AR.LATTICE_CASES
    pick = {"linear": "linear-300x3x256-act3-0.25", "axpby": "axpby-257-0.75-0.25",
            "spmm_csr": "spmm-hub-D68-act0-0.0-bias1-host-ga0", "spmm_csr_rows": "spmm_rows-hub-D68",
            "gather_rows": "gather-300-300-7", "gather_rows-D64": "gather-50-7-64", "segment_sum": "segment-edges-D7", "segment_sum-D64": "segment-edges-D64", "mix2": "mix2-37x64",
            "mul_cols": "mul_cols-300x3-act0-0.0", "mul_cols-D256": "mul_cols-2049x256-act0-0.0"}
    for cid in pick.values():
        assert cid in L, cid
    return pick


ARRIVAL_LATTICE = _arrival_cases()
ARRIVAL_FNS = list(ARRIVAL_LATTICE) + ["sigmoid_gate", "softmax_mix", "proto_cosine", "compare_loss"]


def _arrival_case(fn):
    if fn in ARRIVAL_LATTICE:
        return AR.build(AR.LATTICE_CASES, ARRIVAL_LATTICE[fn])
    g = AR.gauss
    if fn == "sigmoid_gate":
        return _transcendental(fn, {"x": g((300, 64), 60), "z": g((300, 64), 61)}, {}, g((300, 64), 62), {"gx": "x", "gz": "z"})
    if fn == "softmax_mix":
        return _transcendental(fn, {"logits": g((40, 8), 63), "rag": torch.rand(40, 8, generator=torch.Generator().manual_seed(64))},
                               {"lam": 0.3}, g((40, 8), 65), {"glogits": "logits"})
    if fn == "proto_cosine":
        return _transcendental(fn, {"emb": g((100, 30), 66), "proto": g((5, 30), 67)}, {"mode": 1}, g((100, 5), 68),
                               {"gemb": "emb", "gproto": "proto"})
    return _compare_hub_case()


@pytest.mark.parametrize("fn", ARRIVAL_FNS)
def test_gradient_arrival(dev, fn):
    """The output gradient handed over four ways -- (i) dense, from (y * w).sum(); (ii) stride 0, from y.sum(); (iii)
    non-contiguous, from a weighted sum behind torch.cat([y, y2], dim=1); (iv) contiguous but 4 or 12 bytes off a 16-byte
    boundary, from a weighted sum behind torch.cat([pad, y.reshape(-1)]) -- gives the bits of the same values handed over as a
    fresh dense tensor, and on the lattice cases the float64 reference.  (iv) reaches the SpMM-backed backwards (spmm_csr
    without an activation, spmm_csr_rows, gather_rows at a width in 4Z -- at another width the padded copy is aligned anyway),
    whose kernels take 16-byte-aligned rows only, and at widths in 4Z the kernels that choose a float4 path by the address
    (the gather behind segment_sum's backward, the segment reduce behind every column sum)."""
    case = _arrival_case(fn)
    req = tuple(case.grads.values())
    shape = tuple(case.ref["y"].shape)
    n = int(np.prod(shape)) if shape else 1
    two_d = (shape[0], n // shape[0]) if shape and shape[0] > 1 else (n, 1)       # (more than one row: a slice of columns is strided)
    seen = {}

    def arrive(way, pad=0):
        w = AR.ints((two_d[0], 2 * two_d[1]), 70).to(dev) if way == "cat1" else AR.ints(pad + n, 71).to(dev)

        def backward(y):
            y.register_hook(lambda g: seen.__setitem__((way, pad), (g.data_ptr() % 16, g.is_contiguous(), g.stride())))
            if way == "dense":
                (y * w[:n].reshape(y.shape)).sum().backward()
            elif way == "sum":
                y.sum().backward()
            elif way == "cat1":
                y2 = y.reshape(two_d)
                (torch.cat([y2, y2.detach() + 1.0], dim=1) * w).sum().backward()
            else:
                (torch.cat([torch.ones(pad, device=dev), y.reshape(-1)]) * w).sum().backward()
        if way == "sum":
            go = torch.ones(shape)
        elif way == "cat1":
            go = w[:, : two_d[1]].reshape(shape).cpu()
        else:
            go = w[pad:].reshape(shape).cpu()
        return run(case, dev, req, backward), go

    for way, pad in (("dense", 0), ("sum", 0), ("cat1", 0), ("cat0", 1), ("cat0", 3)):
        out, go = arrive(way, pad)
        plain = run(case, dev, req, lambda y: y.backward(go.to(dev).clone()))
        for k in case.grads:
            assert same_bits(out[k], plain[k]), (fn, way, pad, k)
        if case.lattice:
            assert_equals_reference(out, AR.reference(case, go=go), (fn, way, pad))
    if n > 1:       # the four ways are what they claim to be
        assert seen[("sum", 0)][2] == (0,) * len(shape)
        assert not seen[("cat1", 0)][1]
        assert seen[("cat0", 1)][0] == 4 and seen[("cat0", 3)][0] == 12 and seen[("cat0", 1)][1]
