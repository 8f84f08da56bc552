"""ragraph_linear_plan (host arithmetic, no GPU): which of the five dense kernels ragraph_linear_f32 runs for a shape, and its
launch geometry.  The dispatcher launches what this function returns, so pinning it here pins the dispatch: a retuned threshold
fails this table, and tests/test_gpu_linear_variants.py (which asserts the variant before it compares bits) with it."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("RAGRAPH_LINEAR_TILE", "RAGRAPH_LINEAR_NARROW", "RAGRAPH_LINEAR_WGS", "RAGRAPH_LINEAR_MIN_STAGES")

G, S, T, ST, NA = "generic", "small", "tile", "stream", "narrow"

# (M, K, N) -> (variant, grid.x, grid.y, plan[3]): today's dispatch with no switch set
TABLE = [
    ((1, 1, 1), (G, 1, 1, 1)),
    ((33, 18, 256), (G, 1, 4, 1)),
    ((200, 1433, 256), (S, 7, 8, 45)),
    ((65, 256, 256), (S, 3, 8, 8)),
    ((300, 128, 256), (G, 5, 4, 4)),
    ((1000, 260, 384), (S, 32, 12, 9)),
    ((2708, 1433, 128), (S, 85, 4, 45)),
    ((4096, 128, 256), (ST, 64, 1, 1)),
    ((4133, 256, 250), (ST, 130, 1, 1)),
    ((5000, 64, 512), (ST, 40, 2, 1)),
    ((4100, 128, 700), (ST, 65, 3, 1)),
    ((9000, 128, 193), (ST, 141, 1, 1)),
    ((8193, 256, 256), (ST, 129, 1, 2)),
    ((32773, 64, 700), (ST, 65, 3, 4)),
    ((131073, 256, 193), (ST, 456, 1, 9)),
    ((4096, 256, 3), (NA, 16, 1, 8)),
    ((4096, 2048, 8), (NA, 16, 1, 64)),
    ((129, 36, 130950), (T, 2, 1024, 2)),
    ((4100, 36, 8059), (T, 33, 63, 2)),
    ((5800, 260, 5800), (T, 46, 46, 9)),
]


@pytest.fixture(autouse=True)
def _no_switch_set():
    # (read once per process by the library: the in-process tests below describe the default dispatch)
    assert not [v for v in SWITCHES if v in os.environ], "unset the RAGRAPH_LINEAR_* switches to run this file"


def _plan(M, K_, N_, xa=True, wa=True):
    from ragraph_amd import kernels as K

    p = K.linear_plan(M, K_, N_, x_aligned=xa, w_aligned=wa)
    return (K.LINEAR_VARIANTS[p.variant], p.grid_x, p.grid_y, p.steps)


def _cdiv(a, b):
    return -(-a // b)


def test_variant_constants_match_the_header():
    from ragraph_amd import kernels as K

    txt = open(os.path.join(ROOT, "include", "ragraph_hip.h")).read()
    for name in ("GENERIC", "SMALL", "TILE", "STREAM", "NARROW"):
        line = [ln for ln in txt.splitlines() if ln.startswith(f"#define RAGRAPH_LINEAR_PLAN_{name} ")]
        assert len(line) == 1 and int(line[0].split()[2]) == getattr(K, f"LINEAR_{name}")
        assert K.LINEAR_VARIANTS[getattr(K, f"LINEAR_{name}")] == name.lower()
    p = K.linear_plan(4096, 128, 256)
    assert p.variant == K.LINEAR_STREAM and p._fields == ("variant", "grid_x", "grid_y", "steps")


@pytest.mark.parametrize("shape,want", TABLE, ids=["x".join(map(str, s)) for s, _ in TABLE])
def test_todays_dispatch_is_pinned(shape, want):
    assert _plan(*shape) == want


def test_both_sides_of_every_boundary():
    # rows: 4095 | 4096
    assert _plan(4095, 128, 256)[0] == G and _plan(4096, 128, 256)[0] == ST
    # the last 256-column block at least three quarters full: 191 | 192
    assert _plan(4096, 128, 191)[0] == G and _plan(4096, 128, 192)[0] == ST
    # 128 x 128 tiles: 32 x 63 = 2016 | 32 x 64 = 2048
    assert _plan(4096, 36, 8064) == (G, 64, 126, 2) and _plan(4096, 36, 8192) == (T, 32, 64, 2)
    # 64 x 64 blocks: 192 | 193, and K 256 | 255
    assert _plan(768, 256, 1024) == (S, 24, 32, 8)
    assert _plan(769, 256, 1024) == (G, 13, 16, 8) and _plan(768, 255, 1024) == (G, 12, 16, 8)
    # the narrow kernel's exits
    assert _plan(4095, 256, 3) == (S, 128, 1, 8) and _plan(4096, 256, 9) == (S, 128, 1, 8)
    assert _plan(4096, 256, 8)[0] == NA and _plan(4096, 256, 1)[0] == NA
    assert _plan(4096, 48, 3)[0] == G and _plan(4096, 2080, 8)[0] == S
    assert _plan(4096, 2048, 8)[0] == NA and _plan(4096, 32, 3)[0] == NA


def test_unaligned_operands_fall_to_the_scalar_staging_kernels():
    """The tile, stream and narrow kernels read X (tile, stream: W too) in 16-byte pieces; an operand that starts off a
    16-byte boundary takes a kernel that stages scalars.  The narrow kernel reads W by scalars."""
    for shape, (variant, *_rest) in TABLE:
        if variant in (T, ST, NA):
            assert _plan(*shape, xa=False)[0] in (G, S), shape
            assert _plan(*shape, xa=False, wa=False)[0] in (G, S), shape
            if variant == NA:
                assert _plan(*shape, wa=False) == _plan(*shape), shape
            else:
                assert _plan(*shape, wa=False)[0] in (G, S), shape
        else:
            assert _plan(*shape, xa=False, wa=False) == _plan(*shape), shape


def test_error_codes():
    import ctypes

    from ragraph_amd import _native as N

    L = N.lib()
    plan = (ctypes.c_int64 * 4)()
    for M, K_, N_ in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-5, 8, 8)):
        assert L.ragraph_linear_plan(M, K_, N_, 1, 1, plan) == N.EINVAL
    assert L.ragraph_linear_plan(1, 1, 1, 1, 1, None) == N.EINVAL and b"null" in L.ragraph_last_error()
    assert L.ragraph_linear_plan(64, 64, 65535 * 64, 1, 1, plan) == N.OK and plan[2] == 65535
    assert L.ragraph_linear_plan(64, 64, 65535 * 64 + 1, 1, 1, plan) == N.EUNSUPPORTED
    assert b"too large" in L.ragraph_last_error()
    # the same answers as the launch entry gives before it touches the device
    assert L.ragraph_linear_f32(None, 1, 1, None, 1, None, 0, 0.0, None, None) == N.EINVAL


def test_grid_covers_the_output_over_a_random_sweep():
    """Every plan's grid covers M x N with no idle row or column of workgroups, and the streaming kernel's workgroups, each of
    plan[3] stages, cover its stages with none of them empty."""
    rng = np.random.default_rng(20)
    tile_of = {G: 64, S: 32, T: 128}
    seen = set()
    for it in range(6000):
        kind = it % 6
        M = int(rng.integers(1, 300_000)) if kind < 4 else int(rng.integers(1, 5000))
        if kind == 0:      # stream / narrow territory
            K_ = int(rng.choice([32, 64, 128, 256, 512, 2048, 2080]))
            N_ = int(rng.choice([1, 3, 8, 9, 191, 192, 193, 250, 256, 449, 512, 700, 1000]))
        elif kind == 1:    # many tiles
            K_ = 4 * int(rng.integers(1, 100))
            N_ = int(rng.integers(128, 200_000))
        else:
            K_ = int(rng.integers(1, 3000))
            N_ = int(rng.integers(1, 3000)) if kind < 5 else int(rng.integers(1, 4_000_000))
        xa, wa = bool(it % 7), bool(it % 11)
        v, gx, gy, steps = _plan(M, K_, N_, xa, wa)
        seen.add(v)
        if v in tile_of:
            t = tile_of[v]
            assert (gx, gy, steps) == (_cdiv(M, t), _cdiv(N_, t), _cdiv(K_, 32)), (M, K_, N_)
        elif v == NA:
            assert (gx, gy, steps) == (_cdiv(M, 256), 1, K_ // 32) and N_ <= 8 and K_ % 32 == 0 and xa, (M, K_, N_)
        else:
            assert v == ST and K_ in (64, 128, 256) and xa and wa, (M, K_, N_)
            total = _cdiv(M, 32 * (256 // K_))
            assert gy == _cdiv(N_, 256) and steps >= 1
            assert gx * steps >= total > (gx - 1) * steps, (M, K_, N_, gx, steps)
        if v == T:
            assert K_ % 4 == 0 and xa and wa and gx * gy >= 2048
    assert seen == {G, S, T, ST, NA}


CHILD = r"""
import sys
sys.path.insert(0, {root!r})
from ragraph_amd import kernels as K
for (M, K_, N_) in {shapes!r}:
    p = K.linear_plan(M, K_, N_)
    print("PLAN", K.LINEAR_VARIANTS[p.variant], p.grid_x, p.grid_y, p.steps, flush=True)
"""


@pytest.mark.parametrize("env,shapes,want", [
    ({"RAGRAPH_LINEAR_WGS": "8"}, [(4100, 256, 256), (4133, 128, 700), (4229, 64, 250)],
     [(ST, 8, 1, 17), (ST, 2, 3, 33), (ST, 7, 1, 5)]),
    ({"RAGRAPH_LINEAR_MIN_STAGES": "4"}, [(4100, 256, 256), (4096, 256, 3), (4100, 36, 8059)],
     [(ST, 33, 1, 4), (NA, 16, 1, 8), (T, 33, 63, 2)]),
    # no tile and no streaming kernel (one switch, as before); the narrow kernel stays
    ({"RAGRAPH_LINEAR_TILE": "0"}, [(4100, 36, 8059), (4100, 256, 256), (4096, 256, 3), (65, 256, 256)],
     [(G, 65, 126, 2), (G, 65, 4, 8), (NA, 16, 1, 8), (S, 3, 8, 8)]),
    # no narrow kernel; everything else stays
    ({"RAGRAPH_LINEAR_NARROW": "0"}, [(4096, 256, 3), (4100, 256, 6), (4100, 36, 8059), (4100, 256, 256)],
     [(S, 128, 1, 8), (S, 129, 1, 8), (T, 33, 63, 2), (ST, 129, 1, 1)]),
], ids=["wgs8", "min_stages4", "tile0", "narrow0"])
def test_environment_switches(env, shapes, want):
    """The switches are read once per process: one child per setting, which only calls the plan (no GPU)."""
    full = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    full.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, shapes=shapes)], env=full, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = [tuple(ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("PLAN ")]
    assert got == [(v, str(a), str(b), str(c)) for v, a, b, c in want], r.stdout
