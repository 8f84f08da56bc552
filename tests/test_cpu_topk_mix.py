"""Structure-aware retrieval (ragraph_topk_cosine_mix_f32), the parts that need no GPU: the ABI, the workspace rule, argument
validation, the bank's host logic (weights, position codes in bank files) and the sanity of the inputs the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import cref, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ENTRIES = ("ragraph_topk_cosine_mix_workspace_bytes", "ragraph_topk_cosine_mix_f32")


def _lib():
    from ragraph_amd import _native

    return _native, _native.lib()


def test_header_declares_and_library_exports_the_entries():
    header = open(os.path.join(ROOT, "include", "ragraph_hip.h")).read()
    native, lib = _lib()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name + " is not declared in ragraph_hip.h"
        assert name in native.SIGNATURES
        assert getattr(lib, name) is not None
    assert re.search(r"ragraph_topk_cosine_mix_f32\(const float\* Q,\s*int64_t B,\s*const float\* Kn,\s*int64_t N,\s*int D,\s*"
                     r"const float\* Pq,\s*const float\* Pn,\s*int A,\s*float w_struct,\s*float w_sem,\s*int k,\s*"
                     r"int64_t idx_base,", header)


def test_workspace_is_a_host_computation_far_below_a_score_matrix():
    _, lib = _lib()
    for B, N, D, A, k in ((4096, 1 << 20, 256, 10, 10), (1, 1 << 20, 256, 10, 10), (16, 1 << 20, 128, 16, 32),
                          (256, 1 << 20, 64, 4, 1), (100000, 1 << 20, 256, 10, 10)):
        ws = lib.ragraph_topk_cosine_mix_workspace_bytes(B, N, D, A, k)
        assert 0 < ws < B * N * 4 // 8, (B, N, D, A, k, ws)
    assert lib.ragraph_topk_cosine_mix_workspace_bytes(4096, 1 << 20, 256, 10, 10) < 4096 * (1 << 20) * 4 // 8
    # the fallback shapes keep their two slabs inside ~1 GiB
    for B, N, D, A, k in ((4096, 1 << 20, 96, 10, 10), (4096, 1 << 20, 256, 10, 33), (700, 33333, 256, 10, 200)):
        assert 0 < lib.ragraph_topk_cosine_mix_workspace_bytes(B, N, D, A, k) < (5 << 28)
    for bad in ((0, 100, 64, 10, 5), (4, 0, 64, 10, 5), (4, 100, 64, 0, 5), (4, 100, 64, 17, 5), (4, 100, 64, 10, 0)):
        assert lib.ragraph_topk_cosine_mix_workspace_bytes(*bad) == 0


def test_argument_validation_returns_einval_without_a_device():
    native, lib = _lib()
    buf = (ctypes.c_char * 8192)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16   # never dereferenced: every case must be refused before any launch
    big = 1 << 40

    def call(A=10, k=5, pn=a, ws_bytes=big, q=a, w_struct=0.3):
        return lib.ragraph_topk_cosine_mix_f32(q, 4, a, 100, 64, a, pn, A, w_struct, 0.7, k, 0, a, a, a, ws_bytes, None)

    assert call(A=0) == native.EINVAL and "A=0" in native.last_error()
    assert call(A=17) == native.EINVAL
    assert call(k=0) == native.EINVAL
    assert call(k=101) == native.EINVAL          # k > N
    assert call(pn=None) == native.EINVAL and "null" in native.last_error()
    assert call(q=None) == native.EINVAL
    assert call(w_struct=float("nan")) == native.EINVAL
    need = lib.ragraph_topk_cosine_mix_workspace_bytes(4, 100, 64, 10, 5)
    assert need > 16
    assert call(ws_bytes=need - 1) == native.EWORKSPACE and "workspace" in native.last_error()
    assert call(ws_bytes=16) == native.EWORKSPACE   # (the code every entry refuses a short workspace with)


def _bank(flavour="node", n=12, D=8, C=3, with_positions=True):
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    g = torch.Generator().manual_seed(n)
    tgb = ToyGraphBase(None, C, D, 3, device="cpu", flavour=flavour)
    keys = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=-1)
    vals = torch.randn(n, D, generator=g)
    labs = torch.nn.functional.one_hot(torch.randint(0, C, (n,), generator=g), C).float()
    pos = 1.0 / (torch.randint(0, 6, (n, tgb.num_anchors), generator=g).float() + 1.0)
    tgb.add_resources(keys, vals, labs, pos if with_positions else None)
    return tgb, keys, vals, labs, pos


@pytest.mark.parametrize("flavour", ["node", "graph"])
def test_default_weights_are_the_reference_s(flavour):
    tgb, *_ = _bank(flavour)
    assert (tgb.structure_weight, tgb.semantic_weight) == (0.0, 0.999)   # RAGraph_node/ragraph_utils/ToyGraphBase.py:28-29


def test_bank_file_v2_keeps_positions_and_v1_still_loads(tmp_path):
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    tgb, keys, vals, labs, pos = _bank()
    path = str(tmp_path / "bank.pt")
    tgb.save(path)
    blob = torch.load(path, map_location="cpu")
    assert blob["format"] == "ragraph_amd.bank.v2" and torch.equal(blob["positions"], pos)
    back = ToyGraphBase(None, 3, 8, 3, device="cpu")
    back.load(path)
    assert torch.equal(back.resource_positions, pos) and torch.equal(back.resource_keys, keys)
    assert torch.equal(back.resource_values, vals) and torch.equal(back.resource_labels, labs)
    back.load(path, append=True)
    assert back.resource_positions.shape[0] == back.resource_keys.shape[0] == 2 * keys.shape[0]
    # a file of the earlier format: keys, values and labels load; the bank then has no codes
    v1 = str(tmp_path / "bank_v1.pt")
    torch.save({"format": "ragraph_amd.bank.v1", "keys": keys, "values": vals, "labels": labs}, v1)
    old = ToyGraphBase(None, 3, 8, 3, device="cpu")
    old.load(v1)
    assert torch.equal(old.resource_keys, keys) and old.resource_positions.shape[0] == 0
    other = str(tmp_path / "other.pt")
    torch.save({"format": "something.else"}, other)
    with pytest.raises(ValueError):
        old.load(other)


def test_structural_retrieval_without_bank_positions_raises_before_any_kernel(tmp_path):
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    q = torch.randn(4, 8)
    codes = torch.rand(4, 10)
    for make in ("add", "set", "v1"):
        if make == "add":
            tgb, *_ = _bank(with_positions=False)
        elif make == "set":
            tgb, keys, vals, labs, _ = _bank()
            tgb.set_resources(keys, vals, labs)            # adopting tensors without positions drops the old codes
        else:
            src, keys, vals, labs, _ = _bank()
            p = str(tmp_path / "v1.pt")
            torch.save({"format": "ragraph_amd.bank.v1", "keys": keys, "values": vals, "labels": labs}, p)
            tgb = ToyGraphBase(None, 3, 8, 3, device="cpu")
            tgb.load(p)
        tgb.structure_weight = 0.3
        for call in (lambda: tgb.topk(q, 2, codes), lambda: tgb.retrieve_indices(q, False, search_positions=codes),
                     lambda: tgb.retrieve(q, None, False, search_positions=codes),
                     lambda: tgb.retrieve_reduced(q, search_positions=codes),
                     lambda: tgb.retrieve_reduced_noisy(q, search_positions=codes)):
            with pytest.raises(ValueError, match="position"):
                call()
    # with codes in the bank the same call gets as far as the kernels (which need a GPU: no CPU fallback)
    tgb, keys, vals, labs, pos = _bank()
    tgb.structure_weight = 0.3
    with pytest.raises(ValueError, match="search_adj"):
        tgb.retrieve_indices(q, False)                      # neither the query graph nor ready codes
    from ragraph_amd.kernels import RagraphNativeError
    with pytest.raises(RagraphNativeError):
        tgb.topk(q, 2, codes)
    tgb.set_resources(keys, vals, labs, pos)
    assert torch.equal(tgb.resource_positions, pos)
    with pytest.raises(ValueError):
        tgb.set_resources(keys, vals, labs, pos[:-1])


def _top_sets(scores, k):
    s, i = cref.topk_rows(scores, k + 1)
    return i[:, :k], s[:, k - 1] == s[:, k]


def test_g8_inputs_tell_the_structural_term_apart():
    """The GPU tests take g8 at (0.3, 0.7) and (0.5, 0.5) because there every row's top-5 SET differs from the semantic-only
    one and no row has a tie at the k / k+1 boundary; at the reference's (0.001, 0.999) no row differs, so that weight
    alone could not show that the structural term is applied at all."""
    g = dict(np.load(os.path.join(GOLD, "g8_fewshot_retrieve.npz")))
    k = int(g["k"])
    assert k == 5 and g["Q"].shape[0] == 60
    sem, _ = pipeline.fewshot_scores(g["Q"], g["adj"], g["anchors"], g["keys"], g["positions"], 0.0, 1.0)
    sem_idx, _ = _top_sets(sem, k)
    for ws, wm, differ in ((0.3, 0.7, 60), (0.5, 0.5, 60), (0.001, 0.999, 0)):
        sc, _ = pipeline.fewshot_scores(g["Q"], g["adj"], g["anchors"], g["keys"], g["positions"], ws, wm)
        idx, tie = _top_sets(sc, k)
        n_diff = sum(set(a) != set(b) for a, b in zip(idx, sem_idx))
        assert n_diff == differ, (ws, wm, n_diff)
        assert not tie.any(), (ws, wm)
