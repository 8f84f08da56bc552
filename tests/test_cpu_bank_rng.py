"""Bank construction with the draws made on the device, the parts a machine without a GPU can check: the numpy oracle of the
GPU tests (tests/bank_rng_oracle.py) agrees with the Python-int restatement of the hash (tests/noise_oracle.py), the five
entries and their workspace functions are declared, bound and exported alike, and the `build_rng` attribute defaults to "host"
and rejects other values where it is set."""
import os
import re

import numpy as np
import pytest

import bank_rng_oracle as B
import noise_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ragraph_edge_rewrite_csr", "ragraph_multinomial_segments_i64", "ragraph_csr_induced_blocks_f32",
           "ragraph_blocks_to_csr_f32", "ragraph_augment_features_f32")
WORKSPACES = ("ragraph_edge_rewrite_workspace_bytes", "ragraph_multinomial_segments_workspace_bytes",
              "ragraph_blocks_to_csr_workspace_bytes")


def test_numpy_oracle_agrees_with_python_ints_on_random_words():
    rng = np.random.default_rng(7)
    words = rng.integers(0, 2 ** 64, 4000, dtype=np.uint64)
    seeds = [0, 1, 2 ** 62 - 1, 2 ** 64 - 1] + [int(x) for x in rng.integers(0, 2 ** 62, 4)]
    rows = rng.integers(0, 2 ** 64, 500, dtype=np.uint64)
    draws = rng.integers(0, 2 ** 40, 500, dtype=np.uint64)
    assert [int(x) for x in B.splitmix64(words)] == [O.splitmix64(int(x)) for x in words]
    for seed in seeds:
        got = B.lp_draw(seed, rows, draws)
        assert [int(x) for x in got] == [O.lp_draw(seed, int(r), int(d)) for r, d in zip(rows, draws)]
    mods = np.concatenate([rng.integers(1, 2 ** 63, 3990, dtype=np.uint64),
                           np.array([1, 2, 7, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40, 2 ** 62, 2 ** 63 - 1, 2 ** 64 - 1], np.uint64)])
    assert [int(x) for x in B.lp_below(words, mods)] == [O.lp_below(int(h), int(m)) for h, m in zip(words, mods)]
    assert int(B.lp_below(np.uint64(2 ** 64 - 1), np.uint64(2 ** 64 - 1))) == 2 ** 64 - 2
    # u53: the top 53 bits as an exact double in [0, 1)
    u = B.u53(words)
    assert [float(x) for x in u] == [(int(w) >> 11) / 2.0 ** 53 for w in words] and u.min() >= 0 and u.max() < 1
    assert float(B.u53(np.uint64(2 ** 64 - 1))) == 1 - 2.0 ** -53


def test_event_rules_and_weight_quantisation():
    w = np.array([0, 2 ** 11, 2 ** 63, 2 ** 64 - 1], np.uint64)
    assert B.event(w, np.float32(0)).tolist() == [False] * 4            # probability 0 never happens
    assert B.event(w, np.float32(1)).tolist() == [True] * 4             # probability 1 always (u53 < 1)
    assert B.event(w, np.float32(np.nan)).tolist() == [False] * 4
    assert B.event(w, np.float32(2e-9)).tolist() == [True, True, False, False]   # 2^-53 < 2e-9: a 24-bit uniform cannot tell
    assert B.event(w, np.float32(0.5)).tolist() == [True, True, False, False]    # strict: u = 0.5 is not below 0.5
    # the edge threshold is float32 arithmetic: one add, one multiply
    a, b = np.float32(0.1), np.float32(0.7)
    assert B.edge_threshold(a, b) == np.float32(np.float32(a + b) * np.float32(0.5)) and B.edge_threshold(a, b).dtype == np.float32
    p = np.array([0.0, -0.0, -1.0, np.nan, 1.0, 2.0, np.inf, 0.25, 2.0 ** -41, 2.0 ** -40, 1e-30], np.float32)
    assert B.weights(p).tolist() == [0, 0, 0, 0, 2 ** 40, 2 ** 40, 2 ** 40, 2 ** 38, 0, 1, 0]
    assert B.weights(p).dtype == np.uint64
    # the pick: inverse CDF on exact integer prefixes; a zero weight is never returned, an all-zero segment gives -1
    prob = np.array([0.5, 0, 0.25, 0.25, 0, 0, 1.0], np.float32)
    got = B.multinomial_segments(5, prob, np.array([0, 4, 6, 7]), 64)
    assert got.shape == (3, 64) and set(got[0].tolist()) <= {0, 2, 3} and (got[1] == -1).all() and (got[2] == 6).all()
    cum = [2 ** 39, 2 ** 39, 2 ** 39 + 2 ** 38, 2 ** 40]
    for s in range(64):
        t = O.lp_below(O.lp_draw(5, 0, s), 2 ** 40)
        assert got[0, s] == min(i for i in range(4) if cum[i] > t)
    keep = B.rows_kept(9, np.arange(2000), np.full(2000, 0.5, np.float32), 0.5)
    assert [bool(k) for k in keep[:50]] == [(O.lp_draw(9, r, 0) >> 11) * 2.0 ** -53 < 0.25 for r in range(50)]
    assert abs(int(keep.sum()) - 500) < 6 * np.sqrt(2000 * 0.25 * 0.75)


def test_entries_declared_bound_and_exported():
    from ragraph_amd import _native as N

    header = open(os.path.join(ROOT, "include", "ragraph_hip.h")).read()
    for name in ENTRIES + WORKSPACES:
        decl = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, f"{name} is not declared in ragraph_hip.h"
        n_args = len([a for a in decl.group(2).split(",") if a.strip()])
        assert name in N.SIGNATURES, f"{name} is not bound in _native.SIGNATURES"
        res, args = N.SIGNATURES[name]
        assert res is (N._i32 if decl.group(1) == "int" else N._sz) and len(args) == n_args, \
            f"{name}: {len(args)} bound arguments, {n_args} declared"
    lib = N.lib()                                           # (dlopen only: no device is touched)
    for name in ENTRIES + WORKSPACES:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    # the workspace functions are host arithmetic: counts + the scan's scratch, never the node pairs
    assert 4 * 20001 <= lib.ragraph_edge_rewrite_workspace_bytes(20000) < 200_000
    assert 8 * (4_000_000 // 64 + 1) <= lib.ragraph_multinomial_segments_workspace_bytes(4_000_000) < 600_000
    assert 4 * 40961 <= lib.ragraph_blocks_to_csr_workspace_bytes(4096, 10) < 400_000
    src = open(os.path.join(ROOT, "ragraph_amd", "csrc", "bank.hip")).read()
    for name in ENTRIES:
        assert 'extern "C" int ' + name + "(" in src


def test_build_rng_defaults_to_host_and_rejects_other_values():
    from ragraph_amd import kernels as K
    from ragraph_amd.RAGraph_edge import RAGraph as EdgeRAGraph
    from ragraph_amd.RAGraph_fewshot import ToyGraphBaseFewShot
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    for cls in (ToyGraphBase, ToyGraphBaseFewShot, EdgeRAGraph):
        assert cls.build_rng == "host"
        obj = cls.__new__(cls)               # (no constructor: it allocates on the device)
        assert obj.build_rng == "host" and obj.last_build_seed is None
        obj.build_rng = "device"
        assert obj.build_rng == "device" and cls.build_rng == "host"
        for bad in ("cpu", "", None, "Device"):
            with pytest.raises(ValueError, match="build_rng"):
                obj.build_rng = bad
        assert obj.build_rng == "device"
        obj.build_rng = "host"
        assert obj.build_rng == "host"
    assert K.BUILD_SEED_COLUMNS == 7
    assert sorted([K.BUILD_SEED_FEATURE_NOISE, K.BUILD_SEED_NODE_DROP, K.BUILD_SEED_EDGE_SLOT, K.BUILD_SEED_PICK,
                   K.BUILD_SEED_ANCHOR, K.BUILD_SEED_VALUE_NOISE, K.BUILD_SEED_VALUE_DROP]) == list(range(7))
