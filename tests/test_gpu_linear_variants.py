"""Every kernel behind ragraph_linear_f32 against the oracle's fmaf chains, bit for bit, at the smallest shapes that reach it.

A case first asserts that ragraph_linear_plan -- the function the dispatcher itself launches from -- names the kernel the case
was written for (and, for the streaming kernel, the stages per workgroup), then compares ALL outputs with oracle.cref.linear.
A retuned threshold therefore fails the case on its variant assertion instead of moving it silently onto another kernel.

Inputs: X standard normal, W standard normal / sqrt(K); all-zero rows in X and in W; a bias with a +0 and a -0 entry; and a
subnormal band -- ten rows of X scaled by 1e-22 against a few rows of W scaled by 1e-20, whose outputs (~1e-42) are fp32
subnormals in the oracle: the MFMA chains (generic, small, tile, stream) and the VALU chain (narrow) must produce them too.

The forced plans (RAGRAPH_LINEAR_WGS / _MIN_STAGES / _TILE / _NARROW are read once per process) run in child processes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, S, T, ST, NA = "generic", "small", "tile", "stream", "narrow"
TINY = np.finfo(np.float32).tiny   # smallest normal fp32


def _data(M, K_, N_):
    rng = np.random.default_rng(1000003 * M + 1009 * K_ + N_)
    X = rng.standard_normal((M, K_), dtype=np.float32)
    W = (rng.standard_normal((N_, K_), dtype=np.float32) / np.sqrt(K_)).astype(np.float32)
    b = rng.standard_normal(N_, dtype=np.float32)
    xsub = np.r_[3:7, M - 6:M]                 # the first tile and the (ragged) last one
    wsub = np.array([2, N_ // 2, N_ - 1] if N_ >= 16 else [N_ - 1])
    X[xsub] *= np.float32(1e-22)
    W[wsub] *= np.float32(1e-20)
    X[[0, M // 2]] = 0.0
    W[[0, N_ - 2] if N_ >= 16 else [0]] = 0.0
    b[N_ - 1] = 0.0                             # (a subnormal column: the sum survives the bias)
    b[1] = -0.0
    return X, W, b, xsub, wsub


def _compare(got, ref, what):
    """np.array_equal over ALL outputs (NaN never equal).  Equal values whose bits differ can only be zeros of opposite sign: a
    chain whose last step underflows to zero from below is -0 in the oracle's fmaf and +0 out of the MFMA.  Printed, not
    asserted: as a value, and to every consumer here (bias add, activations, top-k), the two are one number."""
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
    differ = int((got != ref).sum() + (np.isnan(got) | np.isnan(ref)).sum())
    zero_sign = int((got.view(np.uint32) != ref.view(np.uint32)).sum()) - differ
    print(f"  {what}: {differ} of {ref.size} outputs differ from the oracle ({zero_sign} more are zeros of the other sign)", flush=True)
    assert np.array_equal(got, ref), f"{what}: {differ} of {ref.size} outputs differ from the oracle"


def _plan_of(xd, wd):
    from ragraph_amd import kernels as K

    p = K.linear_plan(xd.shape[0], xd.shape[1], wd.shape[0], x_aligned=xd.data_ptr() % 16 == 0, w_aligned=wd.data_ptr() % 16 == 0)
    return K.LINEAR_VARIANTS[p.variant], p


def run_case(dev, M, K_, N_, act, variant, steps=None, unaligned=False):
    """Plan assertion, then every output against the oracle: with bias and activation, and without either.  unaligned: once more
    with X starting 4 bytes off a 16-byte boundary, which must take a scalar-staging kernel and give the same bits."""
    from ragraph_amd import kernels as K

    X, W, b, xsub, wsub = _data(M, K_, N_)
    xd, wd, bd = torch.from_numpy(X).to(dev), torch.from_numpy(W).to(dev), torch.from_numpy(b).to(dev)
    name, p = _plan_of(xd, wd)
    print(f"linear {M} x {K_} -> {N_}: {name} grid {p.grid_x} x {p.grid_y}, steps {p.steps}", flush=True)
    assert name == variant, f"{M} x {K_} -> {N_} runs on the {name} kernel, the case is written for {variant}"
    if steps is not None:
        assert p.steps == steps, f"{M} x {K_} -> {N_}: {p.steps} stages per workgroup, the case is written for {steps}"
    ref_b = cref.linear(X, W, b, act=act, alpha=0.25)
    ref_0 = cref.linear(X, W)
    block = ref_0[np.ix_(xsub, wsub)]
    n_sub = int(((block != 0) & (np.abs(block) < TINY)).sum())
    print(f"  subnormal outputs in the oracle's band: {n_sub} of {block.size}", flush=True)
    assert n_sub >= block.size // 2, "the subnormal band of the reference holds no subnormals: the case is vacuous"
    assert not ref_0[0].any() and not ref_0[:, 0].any()
    got_b = K.linear(xd, wd, bd, act=act, alpha=0.25).cpu().numpy()
    got_0 = K.linear(xd, wd).cpu().numpy()
    _compare(got_b, ref_b, f"{name} kernel, bias + act")
    _compare(got_0, ref_0, f"{name} kernel, plain")
    if unaligned:
        buf = torch.empty(M * K_ + 4, dtype=torch.float32, device=dev)
        xu = buf[1:1 + M * K_].view(M, K_)
        xu.copy_(xd)
        assert xu.is_contiguous() and xu.data_ptr() % 16 == 4
        uname, up = _plan_of(xu, wd)
        print(f"  X 4 bytes off a 16-byte boundary: {uname} grid {up.grid_x} x {up.grid_y}", flush=True)
        assert uname in (G, S), f"unaligned X on the {uname} kernel"
        got_u = K.linear(xu, wd, bd, act=act, alpha=0.25).cpu().numpy()
        _compare(got_u, ref_b, f"{uname} kernel on unaligned X, bias + act")


CASES = [
    # ---- the 128 x 128 tile kernel (from 2048 tiles) ----
    (4100, 36, 8059, 2, T, None, True),      # ragged last tile in M and N, one full chunk + one float4; and unaligned X
    (4100, 4, 8059, 0, T, None, False),      # a single float4 of K
    (4000, 64, 8400, 1, T, None, False),     # two full chunks; M < 4096, so not the streaming kernel
    (5800, 260, 5800, 3, T, None, False),    # nine chunks (odd), the last one a single float4
    (129, 36, 130950, 1, T, None, False),    # one live row in the second row tile, grid.y = 1024
    (4096, 36, 8192, 0, T, None, False),     # 32 x 64 = 2048 tiles: the threshold ...
    (4096, 36, 8064, 2, G, None, False),     # ... and 32 x 63 = 2016 below it
    # ---- the streaming kernel, several stages per workgroup ----
    (8193, 256, 256, 3, ST, 2, False),       # the last workgroup: one stage holding a single live row
    (32773, 64, 700, 1, ST, 4, False),       # three column blocks, the last ragged; ragged last stage
    (131073, 256, 193, 2, ST, 9, False),     # 4097 stages: the 512-workgroup target; the last workgroup has two stages
    (4095, 128, 256, 0, G, None, False), (4096, 128, 256, 2, ST, 1, False),     # rows 4095 | 4096
    (4096, 128, 191, 3, G, None, False), (4096, 128, 192, 1, ST, 1, False),     # columns 191 | 192
    # ---- the narrow kernel: widths 4, 5, 6, the largest LDS request, and its exits ----
    (4096, 32, 4, 0, NA, None, False),
    (4099, 64, 5, 1, NA, None, False),
    (4100, 256, 6, 2, NA, None, True),       # and unaligned X
    (4096, 2048, 8, 3, NA, None, False),
    (4095, 256, 3, 1, S, None, False),       # M below 4096
    (4096, 48, 3, 2, G, None, False),        # K % 32 != 0
    (4096, 2080, 8, 0, S, None, False),      # K > 2048
    # ---- small | generic: 192 | 193 blocks of 64 x 64, K 256 | 255 ----
    (768, 256, 1024, 3, S, None, False),
    (769, 256, 1024, 1, G, None, False),
    (768, 255, 1024, 2, G, None, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("M,K_,N_,act,variant,steps,unaligned", CASES,
                         ids=[f"{c[4]}-{c[0]}x{c[1]}x{c[2]}" for c in CASES])
def test_linear_variant_bit_exact(dev, M, K_, N_, act, variant, steps, unaligned):
    run_case(dev, M, K_, N_, act, variant, steps, unaligned)


CHILD = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import torch
import test_gpu_linear_variants as V
dev = torch.device("cuda:0")
bad = 0
for (M, K_, N_, act, variant, steps) in {cases!r}:
    try:
        V.run_case(dev, M, K_, N_, act, variant, steps)
        print("OK ", M, K_, N_, variant, flush=True)
    except AssertionError as e:
        print("BAD", M, K_, N_, variant, e, flush=True)
        bad += 1
sys.exit(1 if bad else 0)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("env,cases", [
    # deep pipelines at ~4100 rows: 17, 33 and 5 stages per workgroup (odd and even), a shorter last workgroup
    ({"RAGRAPH_LINEAR_WGS": "8"}, [(4100, 256, 256, 2, ST, 17), (4133, 128, 700, 3, ST, 33), (4229, 64, 250, 1, ST, 5)]),
    ({"RAGRAPH_LINEAR_MIN_STAGES": "4"}, [(4100, 256, 256, 0, ST, 4)]),
    # "interchangeable", from the other side: a tile and a streaming shape on the 64 x 64 kernel, a narrow one on 32 x 32
    ({"RAGRAPH_LINEAR_TILE": "0"}, [(4100, 36, 8059, 2, G, None), (8193, 256, 256, 3, G, None)]),
    ({"RAGRAPH_LINEAR_NARROW": "0"}, [(4100, 256, 6, 2, S, None)]),
], ids=["wgs8", "min_stages4", "tile0", "narrow0"])
def test_forced_plans_bit_exact(dev, env, cases):
    full = {k: v for k, v in os.environ.items() if not k.startswith("RAGRAPH_LINEAR_")}
    full.update(env)
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), cases=cases)
    r = subprocess.run([sys.executable, "-c", code], env=full, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("OK ") == len(cases), r.stdout
