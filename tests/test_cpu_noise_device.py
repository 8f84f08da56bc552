"""Device noise for noisy fine-tuning, the parts a machine without a GPU can check: the three entries are declared and bound
alike, the Python restatement of the draw (tests/noise_oracle.py, the GPU test's oracle) is pinned and uniform, and the
`noise_rng` attribute defaults to "host" and rejects other values where it is set."""
import os
import re

import pytest

import noise_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ragraph_noise_rows_i64", "ragraph_gather_reduce_noisy_f32", "ragraph_add_normal_noise_f32")


def test_entries_declared_and_bound_with_matching_argument_counts():
    from ragraph_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ragraph_hip.h")).read()
    for name in ENTRIES:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, f"{name} is not declared in ragraph_hip.h"
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert name in N.SIGNATURES, f"{name} is not bound in _native.SIGNATURES"
        res, args = N.SIGNATURES[name]
        assert res is N._i32 and len(args) == n_args, f"{name}: {len(args)} bound arguments, {n_args} declared"
    src = os.path.join(ROOT, "ragraph_amd", "csrc")
    assert os.path.exists(os.path.join(src, "noise.hip"))
    # the hash lives in one shared header; the samplers include it instead of carrying a copy
    assert "splitmix64(uint64_t x) {" in open(os.path.join(src, "rng.h")).read()
    pre = open(os.path.join(src, "pretrain.hip")).read()
    assert '#include "rng.h"' in pre and "splitmix64(uint64_t x) {" not in pre


def test_restated_draw_pinned_values():
    assert O.noise_row(1, 5, 0, 2 ** 40) == 709106395545
    for seed, row, j in ((1, 5, 0), (2 ** 62 - 1, 2 ** 40 + 3, 2), (0, 0, 0)):
        assert O.noise_row(seed, row, j, 1) == 0
        assert 0 <= O.noise_row(seed, row, j, 7) < 7
        assert 0 <= O.lp_draw(seed, row, j) < 2 ** 64


@pytest.mark.parametrize("seed", [1, 2, 3, 12345])
def test_restated_draw_is_uniform(seed):
    rows, draws, bins = 16384, 4, 64
    counts = [0] * bins
    for r in range(rows):
        for j in range(draws):
            counts[O.noise_row(seed, r, j, bins)] += 1
    expect = rows * draws / bins
    chi2 = sum((c - expect) ** 2 / expect for c in counts)
    print(f"seed {seed}: chi-square {chi2:.1f}")
    assert chi2 < 103.4   # the 0.999 quantile at 63 degrees of freedom


def test_noise_rng_defaults_to_host_and_rejects_other_values():
    from ragraph_amd.RAGraph_edge import RAGraph as EdgeRAGraph
    from ragraph_amd.RAGraph_fewshot import ToyGraphBaseFewShot
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    for cls in (ToyGraphBase, ToyGraphBaseFewShot, EdgeRAGraph):
        assert cls.noise_rng == "host"
        obj = cls.__new__(cls)               # (no constructor: it allocates on the device)
        assert obj.noise_rng == "host" and obj.last_noise_seed is None
        obj.noise_rng = "device"
        assert obj.noise_rng == "device" and cls.noise_rng == "host"
        with pytest.raises(ValueError, match="noise_rng"):
            obj.noise_rng = "cpu"
        assert obj.noise_rng == "device"
        obj.noise_rng = "host"
        assert obj.noise_rng == "host"
