"""Edge tests of the small kernels every fine-tuning step runs through -- csrc/rowops.hip (elementwise, softmax, activation
gradients, prototype cosine), scatter_fill (rows.hip), csr_row_ids (ingest.hip) -- against tests/rowops_reference.py, which
tests/test_cpu_rowops_reference.py pins to torch without a GPU.

Bars: kernels that are one rounded fp32 operation after the other (axpby, axpby_dev, mul, mul_cols without ELU, the ReLU /
PReLU / LeakyReLU gz, time_rescale) keep the BITS of the fp32 restatement; everything through expf / expm1f / logf is held to
float64 at `close(..., 1e-4)` (tests/test_gpu_backward.py's bound), softmax_mix at the suite's 1e-6 (probabilities) / 1e-5
(log-probabilities).

Sizes: an elementwise launch is capped at 2048 x 256 = 524 288 threads; R.GRID_SIZES sits on both sides of one block, of
the cap, and three strides beyond it."""
import numpy as np
import pytest
import torch

import rowops_reference as R

pytestmark = pytest.mark.gpu

NMAX = R.GRID_SIZES[-1]
_rng = np.random.default_rng(20240611)
_A = _rng.standard_normal(NMAX).astype(np.float32)      # shared inputs: every case takes a prefix
_B = _rng.standard_normal(NMAX).astype(np.float32)
_G = _rng.standard_normal(NMAX).astype(np.float32)
_Z3 = (3 * _rng.standard_normal(NMAX)).astype(np.float32)
_T = _rng.integers(1_690_000_000, 1_710_000_000, NMAX).astype(np.int64)
_dev_cache = {}


def _d(name, dev, n=None):
    """The shared input `name` on the device (uploaded once), its first n elements."""
    if name not in _dev_cache:
        _dev_cache[name] = torch.from_numpy(globals()[name]).to(dev)
    t = _dev_cache[name]
    return t if n is None else t[:n]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


# ---- (a) grid-stride loops and tails -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.GRID_SIZES)
def test_axpby_mul_bits_at_grid_sizes(dev, n):
    from ragraph_amd import kernels as K

    a, b = _d("_A", dev, n), _d("_B", dev, n)
    assert R.same_bits(_np(K.axpby(a, 0.7, b, -0.3)), R.axpby(_A[:n], 0.7, _B[:n], -0.3))
    assert R.same_bits(_np(K.mul(a, b)), R.mul(_A[:n], _B[:n]))


@pytest.mark.parametrize("n", R.GRID_SIZES)
def test_axpby_dev_bits_at_grid_sizes(dev, n):
    from ragraph_amd import kernels as K

    w = np.random.default_rng(3).standard_normal(65).astype(np.float32)
    a, b, wd = _d("_A", dev, n), _d("_B", dev, n), _t(w, dev)
    pairs = [(0, 1), (1, 0), (0, -1), (-1, -1), (63, 0)] if n in (257, R.GRID_CAP + 1) else [(0, 1), (63, 0)]
    for ia, ib in pairs:
        assert R.same_bits(_np(K.axpby_dev(a, b, wd, ia, ib)), R.axpby_dev(_A[:n], _B[:n], w, ia, ib)), (ia, ib)


def test_axpby_dev_rejects_weight_index_64(dev):
    from ragraph_amd import kernels as K

    a, b = _d("_A", dev, 100), _d("_B", dev, 100)
    w = torch.ones(65, device=dev)                       # (wide enough for the wrapper: the entry's own bound speaks)
    for ia, ib in ((64, 0), (0, 64)):
        with pytest.raises(K.RagraphNativeError, match="index out of range"):
            K.axpby_dev(a, b, w, ia, ib)
    with pytest.raises(K.RagraphNativeError):
        K.axpby_dev(a, b, torch.ones(2, device=dev), 2, 0)


@pytest.mark.parametrize("D", [1, 3, 256, 1433])
def test_mul_cols_column_index_wraps_inside_the_stride(dev, D):
    """n * D crosses the launch cap, so a thread's second element sits at i + 524 288 and its column is (i + 524 288) % D."""
    from ragraph_amd import kernels as K

    n = (R.GRID_CAP + 77) // D + 2
    assert n * D > R.GRID_CAP and n * D <= NMAX
    x = _A[:n * D].reshape(n, D)
    w = np.random.default_rng(D).standard_normal(D).astype(np.float32)
    xd, wd = _d("_A", dev, n * D).reshape(n, D), _t(w, dev)
    assert R.same_bits(_np(K.mul_cols(xd, wd)), R.mul_cols(x, w))
    assert R.same_bits(_np(K.mul_cols(xd, wd, K.ACT_PRELU, 0.25)), R.mul_cols(x, w, R.ACT_PRELU, 0.25))
    assert R.same_bits(_np(K.mul_cols(xd, wd, K.ACT_RELU)), R.mul_cols(x, w, R.ACT_RELU))
    assert R.close(_np(K.mul_cols(xd, wd, K.ACT_ELU, 1.0)), R.mul_cols(x, w, R.ACT_ELU, 1.0))


@pytest.mark.parametrize("n", R.GRID_SIZES)
def test_sigmoid_gate_and_gradient_at_grid_sizes(dev, n):
    from ragraph_amd import kernels as K

    x, z, g = _d("_A", dev, n), _d("_Z3", dev, n), _d("_G", dev, n)
    assert R.close(_np(K.sigmoid_gate(x, z)), R.sigmoid_gate(_A[:n], _Z3[:n]))
    gx, gz = K.sigmoid_gate_grad(x, z, g)
    rx, rz = R.sigmoid_gate_grad(_A[:n], _Z3[:n], _G[:n])
    assert R.close(_np(gx), rx) and R.close(_np(gz), rz)


@pytest.mark.parametrize("n", R.GRID_SIZES)
@pytest.mark.parametrize("act,alpha", [("relu", 0.0), ("prelu", 0.25), ("leaky", 0.01), ("elu", 1.0)])
def test_act_grad_at_grid_sizes(dev, act, alpha, n):
    """ragraph_act_grad_f32 is given the OUTPUT y = act(z); gz against torch's derivative at z, with and without the slope terms
    (gy * z on the negative side, recovered as y / alpha: a tolerance, not bits)."""
    from ragraph_amd import kernels as K

    code = {"relu": K.ACT_RELU, "prelu": K.ACT_PRELU, "leaky": K.ACT_LEAKY, "elu": K.ACT_ELU}[act]
    z, gy = _A[:n], _G[:n]
    zd, gd = _d("_A", dev, n), _d("_G", dev, n)
    y = K.mul_cols(zd.reshape(n, 1), torch.ones(1, device=dev), code, alpha).reshape(n)     # the forward's output
    if act != "elu":
        assert R.same_bits(_np(y), R.apply_act(z, code, alpha))
    rz, rt = R.act_grad(z, gy, code, alpha)
    gz = K.act_grad(y, gd, code, alpha)
    gz2, t = K.act_grad(y, gd, code, alpha, want_alpha_terms=True)
    assert torch.equal(gz, gz2)
    if act == "elu":
        assert R.close(_np(gz), rz)
    else:
        assert R.same_bits(_np(gz), rz)
    if act in ("prelu", "leaky"):                        # (the terms are a PReLU slope's; elementwise bound)
        assert R.close_rows(_np(t).reshape(n, 1), rt.reshape(n, 1))


@pytest.mark.parametrize("n", R.GRID_SIZES)
@pytest.mark.parametrize("slope", [0.25, 0.0, -0.3])
def test_act_grad_prelu_dev_at_grid_sizes(dev, slope, n):
    from ragraph_amd import kernels as K

    z, gy = _A[:n], _G[:n]
    zd, gd, a = _d("_A", dev, n), _d("_G", dev, n), torch.full((1,), slope, device=dev)
    rz, rt = R.act_grad(z, gy, R.ACT_PRELU, slope)
    gz = K.act_grad_prelu_dev(zd, gd, a)
    gz2, t = K.act_grad_prelu_dev(zd, gd, a, want_alpha_terms=True)
    assert torch.equal(gz, gz2)
    assert R.same_bits(_np(gz), rz)
    assert R.close_rows(_np(t).reshape(n, 1), rt.reshape(n, 1))


@pytest.mark.parametrize("n", R.GRID_SIZES)
def test_time_rescale_bits_at_grid_sizes(dev, n):
    from ragraph_amd import kernels as K

    t = _T[:n]
    lo, hi = float(_T.min()), float(_T.max())
    assert R.same_bits(_np(K.time_rescale(_d("_T", dev, n), lo, hi)), R.time_rescale(t, lo, hi))


# ---- (b) special values of the activation gradients ----------------------------------------------------------------------
def _special_vector(seed):
    """R.SPECIAL_Z twice (upstream gradient 2, then a random one of either sign) inside 700 ordinary values: several blocks."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(700).astype(np.float32)
    gy = rng.standard_normal(700).astype(np.float32)
    k = R.SPECIAL_Z.size
    z[100:100 + k] = R.SPECIAL_Z
    gy[100:100 + k] = 2.0
    z[509:509 + k] = R.SPECIAL_Z
    return z, gy


@pytest.mark.parametrize("act,alpha", [("relu", 0.0), ("prelu", 0.25), ("prelu", 0.5), ("prelu", 1.7), ("leaky", 0.01),
                                       ("leaky", 0.25), ("elu", 1.0), ("elu", 0.5)])
def test_act_grad_special_values_match_torch(dev, act, alpha):
    """Through the output, as _Linear / _SpmmCsr / _MulCols call it (slope > 0).  At z = +-0 and where alpha * z underflows to -0
    the derivative of PReLU / LeakyReLU is alpha (torch: z > 0 ? 1 : alpha)."""
    from ragraph_amd import kernels as K

    code = {"relu": K.ACT_RELU, "prelu": K.ACT_PRELU, "leaky": K.ACT_LEAKY, "elu": K.ACT_ELU}[act]
    z, gy = _special_vector(1)
    n = z.size
    y = K.mul_cols(_t(z, dev).reshape(n, 1), torch.ones(1, device=dev), code, alpha).reshape(n)
    gz, t = K.act_grad(y, _t(gy, dev), code, alpha, want_alpha_terms=True)
    rz, rt = R.act_grad(z, gy, code, alpha)
    gz, t = _np(gz), _np(t)
    assert np.isfinite(gz).all() and np.isfinite(t).all()
    if act == "elu":
        assert R.close(gz, rz)
    else:
        assert np.array_equal(gz, rz), np.flatnonzero(gz != rz)
        assert R.same_bits(gz, rz)
    if act in ("prelu", "leaky"):                        # every element to its own bound: 1e30 beside 1e-45
        assert R.close_rows(t.reshape(n, 1), rt.reshape(n, 1))
    if act == "prelu" and alpha == 0.25:                 # the issue's example, as the kernel sees it
        got = _np(K.act_grad(_t(np.array([0.0, -0.0, 1.0, -0.25], dtype=np.float32), dev), torch.full((4,), 2.0, device=dev),
                             code, alpha))
        assert got.tolist() == [0.5, 0.5, 2.0, 0.5]


@pytest.mark.parametrize("slope", [0.25, 0.5, 1.7, 0.0, -0.3])
def test_act_grad_prelu_dev_special_values_match_torch(dev, slope):
    """From the pre-activation with the slope on the device -- both branches of the kernel (slope > 0, slope <= 0) -- and the
    host-scalar path's bits at the same points (act_grad on y for a positive slope, on z itself otherwise)."""
    from ragraph_amd import kernels as K

    z, gy = _special_vector(2)
    n = z.size
    zd, gd = _t(z, dev), _t(gy, dev)
    gz, t = K.act_grad_prelu_dev(zd, gd, torch.full((1,), slope, device=dev), want_alpha_terms=True)
    rz, rt = R.act_grad(z, gy, R.ACT_PRELU, slope)
    assert np.array_equal(_np(gz), rz), np.flatnonzero(_np(gz) != rz)
    assert R.same_bits(_np(gz), rz)
    assert np.isfinite(_np(t)).all() and R.close_rows(_np(t).reshape(n, 1), rt.reshape(n, 1))
    ones = torch.ones(1, device=dev)
    if slope > 0:
        y = K.mul_cols(zd.reshape(n, 1), ones, K.ACT_PRELU, slope).reshape(n)
        gz_h, t_h = K.act_grad(y, gd, K.ACT_PRELU, slope, want_alpha_terms=True)
    else:
        gz_h = K.act_grad(zd, gd, K.ACT_PRELU, slope)
        t_h = K.mul(gd, K.axpby(zd, 1.0, K.mul_cols(zd.reshape(n, 1), ones, K.ACT_RELU).reshape(n), -1.0))
    assert torch.equal(gz, gz_h) and torch.equal(t, t_h)


# ---- (c) saturation --------------------------------------------------------------------------------------------------------
def test_sigmoid_gate_saturates_to_finite_values(dev):
    from ragraph_amd import kernels as K

    zs = np.array([20, 88, 89, 104, 1e4, np.inf], dtype=np.float32)
    z = np.tile(np.concatenate([zs, -zs]), 40)
    rng = np.random.default_rng(7)
    x, g = rng.standard_normal(z.size).astype(np.float32), rng.standard_normal(z.size).astype(np.float32)
    out = _np(K.sigmoid_gate(_t(x, dev), _t(z, dev)))
    gx, gz = (_np(v) for v in K.sigmoid_gate_grad(_t(x, dev), _t(z, dev), _t(g, dev)))
    assert np.isfinite(out).all() and np.isfinite(gx).all() and np.isfinite(gz).all()
    rx, rz = R.sigmoid_gate_grad(x, z, g)
    assert R.close(out, R.sigmoid_gate(x, z).astype(np.float32))
    assert R.close(gx, rx.astype(np.float32)) and R.close(gz, rz.astype(np.float32))
    # saturated ends: expf(89) is beyond FLT_MAX (sigmoid = 0), and 1 - sigmoid(z) = 0 in fp32 from z = 17.4 on
    sat = np.abs(z) >= 89
    assert (gz[sat] == 0).all() and (gz[z == 20] == 0).all()
    assert np.array_equal(out[z >= 20], x[z >= 20]) and (out[z <= -89] == 0).all() and (gx[z <= -89] == 0).all()


@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_elu_gradient_near_minus_alpha(dev, alpha):
    """The ELU derivative through the output is y + alpha: at the floor y = -alpha (z below -17: alpha * expm1f(z) rounds to
    -alpha) it is exactly 0, one ulp above it one ulp of gradient -- never negative, never NaN."""
    from ragraph_amd import kernels as K

    a32 = np.float32(alpha)
    y = np.array([-a32, np.nextafter(-a32, np.float32(0)), -a32 + np.float32(1e-6), -a32 / 2, -0.0, 0.0,
                  np.float32(1e-45), 3.0], dtype=np.float32)
    y = np.tile(y, 50)
    g = np.random.default_rng(8).standard_normal(y.size).astype(np.float32)
    gz = _np(K.act_grad(_t(y, dev), _t(g, dev), K.ACT_ELU, alpha))
    ref = R.elu_grad_from_output(y, g, alpha)
    assert np.isfinite(gz).all() and R.close(gz, ref)
    assert (gz[y == -a32] == 0).all()
    assert np.array_equal(np.sign(gz[y > -a32]), np.sign(g[y > -a32]))
    # and from z: the forward's output at z far below zero, then the gradient
    z = np.array([-5, -16, -17.5, -20, -88, -104, -1e4], dtype=np.float32)
    yd = K.mul_cols(_t(z, dev).reshape(-1, 1), torch.ones(1, device=dev), K.ACT_ELU, alpha).reshape(-1)
    assert R.close(_np(yd), R.apply_act(z, R.ACT_ELU, alpha)) and (_np(yd) >= -a32).all()
    gz = _np(K.act_grad(yd, torch.ones(z.size, device=dev), K.ACT_ELU, alpha))
    assert R.close(gz, R.act_grad(z, np.ones(z.size), R.ACT_ELU, alpha)[0]) and (gz >= 0).all()


# ---- (d) softmax_mix and softmax_grad ------------------------------------------------------------------------------------
def _softmax_rows(B, C):
    """Logits [B, C] of magnitude ~3 with, in turn (row index mod 8): an equal-logits row, rows scaled to +-1e4, rows with
    masked (-inf) classes beside finite ones.  Returns (logits, scaled-row mask)."""
    rng = np.random.default_rng(B * 10007 + C)
    lg = (3 * rng.standard_normal((B, C))).astype(np.float32)
    r = np.arange(B) % 8
    lg[r == 1] = 2.5
    lg[r == 2] *= np.float32(1e4 / 3)
    lg[r == 3] = -1e4 + lg[r == 3]
    if C >= 2:
        m = rng.random((B, C)) < 0.3
        m[:, 0] = False                                  # (at least one finite class in every row)
        lg[(r == 5)[:, None] & m] = -np.inf
    if B == 1:                                           # one row: make it the hardest ordinary one, scaled
        lg *= np.float32(1e4 / 3)
    scaled = (r == 2) | (r == 3) | (B == 1)
    return lg, scaled


def _softmax_tol(lg, scaled, base):
    """base, plus on the scaled rows 2^-22 * max |x - max(x)|: the rounding of the kernel's one fp32 subtraction."""
    fin = np.where(np.isfinite(lg), lg, np.nan)
    spread = np.nanmax(np.abs(fin - np.nanmax(fin, axis=1, keepdims=True)), axis=1)
    return (base + np.where(scaled, 2.0 ** -22 * spread, 0.0))[:, None]


@pytest.mark.parametrize("B", [1, 255, 256, 257])
@pytest.mark.parametrize("C", [1, 2, 70, 1023, 1024])
def test_softmax_mix_rows(dev, C, B):
    """Against float64 of the same formula: 1e-6 on probabilities, 1e-5 on log-probabilities, plus the subtraction's rounding
    on the scaled rows.  With the normaliser as ONE chain of C adds the probabilities of C = 1023 rows were up to 1.65e-6
    off (B = 255, 256, 257: ~sqrt(C) roundings of the whole sum); the kernel now sums it in blocks of 64 classes."""
    from ragraph_amd import kernels as K

    lg, scaled = _softmax_rows(B, C)
    rag = np.random.default_rng(C).random((B, C)).astype(np.float32)
    lgd, ragd = _t(lg, dev), _t(rag, dev)
    for log_mode in (False, True):
        tol = _softmax_tol(lg, scaled, 1e-5 if log_mode else 1e-6)
        for lam, r, rd in ((0.0, None, None), (0.0, rag, ragd), (0.3, rag, ragd), (1.0, rag, ragd)):
            got = _np(K.softmax_mix(lgd, rd, lam, log_mode=log_mode)).astype(np.float64)
            ref = R.softmax_mix(lg, r, lam, log_mode)
            what = f"log_mode={log_mode} lam={lam} rag={r is not None}"
            # non-finite results only where the formula has them (a masked class in log mode), and the same ones
            assert np.array_equal(np.isnan(got), np.isnan(ref)), what
            inf = np.isinf(ref)
            assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref[inf]), what
            if not log_mode:
                assert np.isfinite(got).all(), what
            fin = np.isfinite(ref)
            err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)), 0.0)
            assert (err <= tol).all(), (what, float((err - tol).max()), np.argwhere(err > tol)[:4])


def test_softmax_mix_and_grad_reject_bad_class_counts(dev):
    from ragraph_amd import kernels as K

    from ragraph_amd import _native as N

    with pytest.raises(K.RagraphNativeError, match="1024"):
        K.softmax_mix(torch.zeros(2, 1025, device=dev), None)
    # a class count below 1 cannot be a tensor's last axis behind the wrappers' reshape: the entries themselves
    L = N.lib()
    buf = torch.zeros(8, device=dev)
    for C in (0, -1):
        rc = L.ragraph_softmax_mix_f32(buf.data_ptr(), None, 2, C, 0.0, 0, buf.data_ptr(), None)
        with pytest.raises(K.RagraphNativeError, match="softmax_mix: C="):
            N.check(rc, "softmax_mix")
        rc = L.ragraph_softmax_grad_f32(buf.data_ptr(), buf.data_ptr(), 2, C, 1.0, buf.data_ptr(), None)
        with pytest.raises(K.RagraphNativeError, match="softmax_grad: C="):
            N.check(rc, "softmax_grad")


@pytest.mark.parametrize("B", [1, 255, 256, 257])
@pytest.mark.parametrize("C", [1, 2, 70, 1023, 1024])
def test_softmax_grad_rows(dev, C, B):
    """ragraph_softmax_grad_f32 on the fp32-rounded float64 probabilities, against float64 autograd of
    sum(softmax(logits) * go * scale)."""
    from ragraph_amd import kernels as K

    lg, _ = _softmax_rows(B, C)
    go = np.random.default_rng(B + C).standard_normal((B, C)).astype(np.float32)
    lt = torch.from_numpy(lg).double().requires_grad_(True)
    p = torch.softmax(lt, 1)
    (p * torch.from_numpy(go).double()).sum().backward()
    ref1 = lt.grad.numpy()
    p32 = p.detach().float()
    assert R.close(R.softmax_grad(p32.numpy(), go, 1.0), ref1, 1e-6)          # (the restatement, on the rounded p)
    for scale in (1.0, 0.7):
        got = _np(K.softmax_grad(p32.to(dev), _t(go, dev), scale))
        assert np.isfinite(got).all()
        assert R.close(got, ref1 * float(np.float32(scale))), scale


# ---- (e) time_rescale ------------------------------------------------------------------------------------------------------
def test_time_rescale_large_negative_and_degenerate_ranges(dev):
    """int64 time steps beyond 2^24 (where fp32 stops holding every integer) and 2^31, negative ones, and t_min == t_max:
    the bits of the reference's t.float(), subtract, divide on torch-CPU -- the build has no fast-math and a correctly
    rounded fp32 division -- and its inf / NaN placement for the empty range."""
    from ragraph_amd import kernels as K

    rng = np.random.default_rng(9)
    t = np.concatenate([rng.integers(1_690_000_000, 1_710_000_000, 600), rng.integers(2 ** 24, 2 ** 25, 100),
                        rng.integers(2 ** 31, 2 ** 33, 100), rng.integers(-(2 ** 33), 0, 100), rng.integers(-300, 300, 100),
                        np.array([2 ** 24 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 129, 2 ** 53 + 1, -(2 ** 40) - 1, 0])])
    t = t.astype(np.int64)
    td = _t(t, dev)
    for lo, hi in ((float(t.min()), float(t.max())), (1.69e9, 1.71e9), (-300.0, 300.0), (0.0, 2.0 ** 31), (1.7e9, 1.7e9 + 128)):
        assert R.same_bits(_np(K.time_rescale(td, lo, hi)), R.time_rescale(t, lo, hi)), (lo, hi)
    # the empty range: (t - t_min) / 0
    for v in (5.0, 1.7e9, -300.0):
        u = np.array([v, v + 1000, v - 1000, v], dtype=np.float64).astype(np.int64)
        got, ref = _np(K.time_rescale(_t(u, dev), v, v)), R.time_rescale(u, v, v)
        assert np.isnan(ref[0]) and ref[1] == np.inf and ref[2] == -np.inf
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(got[~np.isnan(ref)], ref[~np.isnan(ref)])


# ---- (f) csr_row_ids and scatter_fill_ -----------------------------------------------------------------------------------
_ROW_LENGTHS = {
    "empty_start_middle_end": [0, 0, 3, 1, 0, 0, 0, 7, 256, 0, 2, 0, 0],
    "single_row": [9],
    "single_long_row": [2 * 256 + 2],
    "long_rows": [255, 0, 256, 257, 0, 2 * 256 + 2, 1, 0],
    "all_empty": [0, 0, 0, 0],
    "many_rows": list(np.random.default_rng(10).integers(0, 4, 1500)),
}


@pytest.mark.parametrize("case", sorted(_ROW_LENGTHS))
def test_csr_row_ids_matches_repeat(dev, case):
    from ragraph_amd import kernels as K

    rowptr = np.concatenate([[0], np.cumsum(_ROW_LENGTHS[case])]).astype(np.int64)
    nnz = int(rowptr[-1])
    got = K.csr_row_ids(_t(rowptr, dev), nnz)
    assert got.dtype == torch.int64 and got.shape == (nnz,)
    assert np.array_equal(_np(got), R.csr_row_ids(rowptr))


@pytest.mark.parametrize("case", sorted(_ROW_LENGTHS))
def test_scatter_fill_matches_a_loop(dev, case):
    """Rows of the score matrix get `value` at their listed columns -- duplicates inside a row included; every other element
    keeps its bits, the last column (never listed) among them."""
    from ragraph_amd import kernels as K

    lens = _ROW_LENGTHS[case]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    B, nnz, N = len(lens), int(rowptr[-1]), 301
    rng = np.random.default_rng(len(case))
    col = rng.integers(0, N - 1, nnz).astype(np.int64)               # (column N - 1 stays untouched)
    if nnz >= 3:
        col[1] = col[0]                                              # duplicates inside a row
    for b in range(B):
        if lens[b] >= 256:
            col[rowptr[b] + 255] = col[rowptr[b]]                    # ... also across the 256-thread stride
    S = rng.standard_normal((B, N)).astype(np.float32)
    Sd = _t(S, dev)
    cold = _t(col, dev) if nnz else torch.zeros(0, dtype=torch.int64, device=dev)
    out = K.scatter_fill_(Sd, _t(rowptr, dev), cold, -1e8)
    assert out is Sd
    ref = R.scatter_fill(S, rowptr, col, -1e8)
    assert R.same_bits(_np(Sd), ref) and R.same_bits(_np(Sd)[:, -1], S[:, -1])


def test_scatter_fill_without_rows(dev):
    from ragraph_amd import kernels as K

    S = torch.zeros(0, 17, device=dev)
    out = K.scatter_fill_(S, torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), 1.0)
    assert out.shape == (0, 17)
    assert K.csr_row_ids(torch.zeros(2, dtype=torch.int64, device=dev), 0).shape == (0,)


# ---- (g) zero-norm rows in proto_cosine and its two gradients ------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("G", [1, 5, 257])
@pytest.mark.parametrize("D", [1, 63, 65, 256])
@pytest.mark.parametrize("C", [1, 64])
def test_proto_cosine_zero_norm_rows(dev, C, D, G, mode):
    """An all-zero embedding, an all-zero prototype and a row whose squared norm is a denormal (entries 1e-20): the norms clamp
    at eps = 1e-8, the cosine is 0 / tiny, the gradients 1 / eps large -- and finite.  Against float64 autograd of
    x.y / (max(|x|, eps) max(|y|, eps)) (+ softmax / log_softmax): `close(..., 1e-4)` over the whole array, and row by row
    the tighter bounds of R.proto_cosine_grad_bounds (a 1e8-large row must not hide the ordinary ones)."""
    from ragraph_amd import kernels as K

    rng = np.random.default_rng(1000 * C + 10 * D + G + mode)
    emb = rng.standard_normal((G, D)).astype(np.float32)
    proto = rng.standard_normal((C, D)).astype(np.float32)
    if G >= 3:
        emb[1] = 0.0
        emb[2] = np.float32(1e-20) * np.sign(emb[2])
    elif D % 2:
        emb[0] = 0.0
    else:
        emb[0] = np.float32(1e-20) * np.sign(emb[0])
    if C >= 2:
        proto[C // 2] = 0.0
        proto[1] = np.float32(1e-20) * np.sign(proto[1])
    elif G == 5:
        proto[0] = 0.0
    go = rng.standard_normal((G, C)).astype(np.float32)
    ref_out, ref_gemb, ref_gproto = R.proto_cosine(emb, proto, mode, go)
    ed, pd, gd = _t(emb, dev), _t(proto, dev), _t(go, dev)
    out = K.proto_cosine(ed, pd, mode)
    assert torch.isfinite(out).all() and R.close(_np(out), ref_out)
    b_emb, b_proto = R.proto_cosine_grad_bounds(emb, proto, go, ref_gemb, ref_gproto)
    gemb = K.proto_cosine_grad(ed, pd, mode, out, gd)
    assert torch.isfinite(gemb).all() and R.close(_np(gemb), ref_gemb)
    err = np.abs(_np(gemb) - ref_gemb)
    assert (err <= b_emb).all(), (float((err / b_emb).max()), np.argwhere(err > b_emb)[:4])
    if C * D <= 8192:
        gproto = K.proto_cosine_grad_proto(ed, pd, mode, out, gd)
        assert torch.isfinite(gproto).all() and R.close(_np(gproto), ref_gproto)
        err = np.abs(_np(gproto) - ref_gproto)
        assert (err <= b_proto).all(), (float((err / b_proto).max()), np.argwhere(err > b_proto)[:4])
    else:                                                # (the LDS accumulators hold C * D <= 8192)
        with pytest.raises(K.RagraphNativeError, match="8192"):
            K.proto_cosine_grad_proto(ed, pd, mode, out, gd)


# ---- (h) where users meet it: through autograd -----------------------------------------------------------------------------
def _graph_with_empty_rows(dev, n=150, seed=12):
    """A non-symmetric graph of n nodes in which 10 rows are empty (isolated nodes / padded rows) and 6 more have neighbours
    only among the nodes of `zero_nodes` (whose features are zero): the pre-activation of those 16 rows is exactly +0 with a
    zero bias.  Returns (dense float64 adjacency on the host, CSRGraph, zero_nodes)."""
    from ragraph_amd.graph import CSRGraph

    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(n, n, generator=g) < 0.06).float() * (0.1 + torch.rand(n, n, generator=g))
    zero_nodes = torch.arange(20, 32)
    a[:, zero_nodes] = 0.0                               # (ordinary rows do not read them: their gradient comes from the 6 rows)
    empty = torch.tensor([0, 1, 40, 41, 42, 77, 100, 147, 148, n - 1])
    a[empty] = 0.0
    only_zero = torch.tensor([5, 6, 60, 61, 120, 121])
    a[only_zero] = 0.0
    for i, r in enumerate(only_zero):
        a[r, zero_nodes[i:i + 3]] = 0.5 + 0.1 * i
    assert not torch.equal(a, a.t())
    csr = CSRGraph.from_dense(a.to(dev))
    assert int((csr.rowptr[1:] == csr.rowptr[:-1]).sum()) == 10
    return a.double(), csr, zero_nodes


@pytest.mark.parametrize("mode", ["host", "dev"])
@pytest.mark.parametrize("slope", [0.25, 0.0, -0.3])
def test_spmm_autograd_at_exact_zeros(dev, slope, mode):
    """autograd.spmm_csr (host-scalar slope and device slope) with a zero bias on a graph with empty rows: the gradients of x,
    the bias and the slope against float64 torch of PReLU(A x + b).  16 of 150 rows sit at z = +0, where torch's derivative
    is the slope."""
    from ragraph_amd import autograd as A
    from ragraph_amd import kernels as K

    a64, csr, zero_nodes = _graph_with_empty_rows(dev)
    n, D = a64.shape[0], 64
    g = torch.Generator().manual_seed(13)
    x0 = torch.randn(n, D, generator=g)
    x0[zero_nodes] = 0.0
    w = torch.randn(n, D, generator=g)
    x = x0.to(dev).requires_grad_(True)
    bias = torch.zeros(D, device=dev, requires_grad=True)
    alpha = torch.full((1,), slope, device=dev, requires_grad=True)
    y = A.spmm_csr(csr, x, bias, K.ACT_PRELU, alpha, slope if mode == "host" else None)
    (y * w.to(dev)).sum().backward()
    x2, b2 = x0.double().requires_grad_(True), torch.zeros(D, dtype=torch.float64, requires_grad=True)
    a2 = torch.full((1,), float(np.float32(slope)), dtype=torch.float64, requires_grad=True)
    z = a64 @ x2 + b2
    assert int((z == 0).all(dim=1).sum()) == 16
    ref = torch.nn.functional.prelu(z, a2)
    (ref * w.double()).sum().backward()
    assert R.close(_np(y), ref.detach().numpy(), 1e-5)
    assert R.close(_np(bias.grad), b2.grad.numpy()), float((bias.grad.cpu() - b2.grad).abs().max())
    assert R.close(_np(x.grad), x2.grad.numpy()), float((x.grad.cpu() - x2.grad).abs().max())
    assert R.close(_np(alpha.grad), a2.grad.numpy())


@pytest.mark.parametrize("slope", [0.01, 0.25, 0.0, -0.3])
def test_linear_autograd_leaky_at_exact_zeros(dev, slope):
    """autograd.linear with LeakyReLU, all-zero input rows and a zero bias (pre-activation exactly +0), for positive slopes
    (backward through the output) and for slopes <= 0 (the output no longer determines the pre-activation's sign: the layer
    keeps it) -- output and the gradients of x, weight and bias against float64 torch."""
    import torch.nn.functional as F
    from ragraph_amd import autograd as A
    from ragraph_amd import kernels as K

    g = torch.Generator().manual_seed(14)
    n, Fin, Fout = 70, 40, 33
    x0 = torch.randn(n, Fin, generator=g)
    x0[::7] = 0.0
    w0 = 0.3 * torch.randn(Fout, Fin, generator=g)
    tgt = torch.randn(n, Fout, generator=g)
    x, w = x0.to(dev).requires_grad_(True), w0.to(dev).requires_grad_(True)
    b = torch.zeros(Fout, device=dev, requires_grad=True)
    y = A.linear(x, w, b, K.ACT_LEAKY, slope)
    (y * tgt.to(dev)).sum().backward()
    x2, w2 = x0.double().requires_grad_(True), w0.double().requires_grad_(True)
    b2 = torch.zeros(Fout, dtype=torch.float64, requires_grad=True)
    ref = F.leaky_relu(F.linear(x2, w2, b2), float(np.float32(slope)))
    (ref * tgt.double()).sum().backward()
    assert R.close(_np(y), ref.detach().numpy(), 1e-5)
    assert torch.equal(y.detach(), K.linear(x.detach(), w.detach(), b.detach(), act=K.ACT_LEAKY, alpha=slope))
    assert R.close(_np(b.grad), b2.grad.numpy()), float((b.grad.cpu() - b2.grad).abs().max())
    assert R.close(_np(x.grad), x2.grad.numpy()) and R.close(_np(w.grad), w2.grad.numpy())


@pytest.mark.parametrize("slope", [0.25, 0.0, -0.3])
def test_decode_step_at_exact_zeros_eager_and_captured(dev, slope):
    """One GcnLayers.decode training step on the graph with empty rows, zero bias, zero input rows: the gradients of weight,
    bias and slope against float64 torch; then the same steps eagerly and through CapturedTrainStep (the device-slope
    path), bit for bit."""
    import torch.nn.functional as F
    from ragraph_amd.capture import CapturedTrainStep
    from ragraph_amd.gcnlayers import GcnLayers

    a64, csr, zero_nodes = _graph_with_empty_rows(dev)
    n, D = a64.shape[0], 64
    g = torch.Generator().manual_seed(15)
    h0 = torch.randn(n, D, generator=g)
    h0[zero_nodes] = 0.0
    w0 = torch.randn(n, D, generator=g)
    h, w = h0.to(dev), w0.to(dev)

    def make():
        torch.manual_seed(16)
        net = GcnLayers(18, D, 2, 0.3).to(dev)
        with torch.no_grad():
            net.convs[1].act.weight.fill_(slope)
        assert not net.convs[1].bias.any()
        opt = torch.optim.Adam(net.convs[1].parameters(), lr=1e-2, capturable=True)

        def step(hh, ww):
            return ((net.decode(hh, csr) - ww) ** 2).mean()
        return net, step, opt

    net, step, opt = make()
    c = net.convs[1]
    step(h, w).backward()
    W2 = c.fc.weight.detach().cpu().double().requires_grad_(True)
    b2 = c.bias.detach().cpu().double().requires_grad_(True)
    a2 = c.act.weight.detach().cpu().double().requires_grad_(True)
    z = a64 @ (h0.double() @ W2.t()) + b2
    assert int((z == 0).all(dim=1).sum()) == 16
    ((F.prelu(z, a2) - w0.double()) ** 2).mean().backward()
    for name, got, ref in (("weight", c.fc.weight.grad, W2.grad), ("bias", c.bias.grad, b2.grad), ("slope", c.act.weight.grad, a2.grad)):
        assert R.close(_np(got) * n * D, ref.numpy() * n * D), (name, float((got.cpu() - ref).abs().max()))
    # eager against captured from the same state (gradients dropped: the eager loop below starts with zero_grad)
    net_e, step_e, opt_e = make()
    net_c, step_c, opt_c = make()
    cap = CapturedTrainStep(step_c, opt_c, h, w)
    for i in range(3):
        opt_e.zero_grad()
        le = step_e(h, w)
        le.backward()
        opt_e.step()
        lc = cap(h, w)
        assert torch.equal(le.detach(), lc), f"loss differs at step {i + 1}"
        for (name, p), q in zip(net_e.named_parameters(), net_c.parameters()):
            assert torch.equal(p.detach(), q.detach()), f"{name} differs at step {i + 1}"
