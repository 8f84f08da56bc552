"""Position codes of large graphs (ragraph_position_codes_csr_global_f32), the parts that need no GPU: the ABI, the workspace
rule, argument validation on both sides of the C ABI, and the bank's two attributes."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ragraph_position_codes_csr_global_workspace_bytes", "ragraph_position_codes_csr_global_f32")


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
    assert re.search(r"ragraph_position_codes_csr_global_f32\(const int64_t\* rowptr,\s*const int32_t\* col,\s*const float\* val,\s*"
                     r"int64_t n,\s*const int64_t\* anchors,\s*int A,\s*float dis_q,\s*float\* codes,\s*float\* dist,\s*"
                     r"int rounds,\s*int resume,\s*int32_t\* converged,\s*void\* ws,\s*size_t ws_bytes,\s*void\* stream\)", header)
    m = re.search(r"#define RAGRAPH_POSITION_CODES_LONG_ROW (\d+)", header)
    assert m and int(m.group(1)) == native.POSITION_CODES_LONG_ROW
    assert len(native.SIGNATURES["ragraph_position_codes_csr_global_f32"][1]) == 15


def test_workspace_grows_with_n_and_with_chunks_of_16_anchors():
    _, lib = _lib()
    size = lib.ragraph_position_codes_csr_global_workspace_bytes
    sizes = [size(n, 10) for n in (1, 1000, 40001, 100000, 4000000, (1 << 31) - 1)]
    assert all(s > 0 for s in sizes) and sizes == sorted(set(sizes))
    for n in (1000, 100000):
        assert size(n, 1) == size(n, 10) == size(n, 16) < size(n, 17) == size(n, 32) < size(n, 33)
        assert size(n, 10) >= n * (16 * 4 + 2)                       # the [n, 16] state and the two dirty bytes
        assert size(n, 17) - size(n, 16) >= n * (16 * 4 + 2) - 512   # (each part is rounded up to 256 bytes)
    assert size(100000, 10) < 100000 * 80 + 4096                      # ... and little else: far from an n x n matrix
    for bad in ((0, 10), (-5, 10), (100, 0), (100, -1), (1 << 31, 10), (1 << 40, 10)):
        assert size(*bad) == 0, bad


def test_c_entry_refuses_bad_arguments_before_any_launch():
    native, lib = _lib()
    buf = (ctypes.c_char * 8192)()
    a = (ctypes.addressof(buf) + 63) // 64 * 64   # never dereferenced: every case must be refused before any launch
    need = lib.ragraph_position_codes_csr_global_workspace_bytes(100, 10)

    def call(n=100, A=10, rounds=4, ws=a, ws_bytes=1 << 40, codes=a, rowptr=a):
        return lib.ragraph_position_codes_csr_global_f32(rowptr, a, a, n, a, A, 10.0, codes, None, rounds, 0, None, ws, ws_bytes,
                                                         None)

    assert call(n=0) == native.EINVAL
    assert call(A=0) == native.EINVAL
    assert call(n=1 << 31) == native.EUNSUPPORTED
    assert call(rounds=0) == native.EINVAL and "rounds" in native.last_error()
    assert call(codes=None) == native.EINVAL and "null" in native.last_error()
    assert call(rowptr=None) == native.EINVAL
    assert call(ws=None) == native.EINVAL
    assert call(ws_bytes=need - 1) == native.EWORKSPACE and "workspace" in native.last_error()
    assert call(ws=a + 4) == native.EINVAL


def test_wrapper_validates_method_and_rounds_before_touching_a_device():
    from ragraph_amd import kernels as K

    rp, c, v, a = torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0), torch.zeros(1, dtype=torch.int64)
    for method in ("lds", "Global", 1):
        with pytest.raises(ValueError, match="method"):
            K.position_codes_csr(rp, c, v, a, method=method)
    for rounds in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="rounds"):
            K.position_codes_csr(rp, c, v, a, rounds=rounds)
        with pytest.raises(ValueError, match="rounds"):
            K.position_codes_csr(rp, c, v, a, rounds=rounds, method="global")
    # valid arguments get as far as the device check (no CPU fallback)
    with pytest.raises(K.RagraphNativeError):
        K.position_codes_csr(rp, c, v, a, rounds=4, method="global")
    assert K.POSITION_CODES_ROUNDS_PER_READBACK >= 1


@pytest.mark.parametrize("flavour", ["node", "graph"])
def test_banks_have_the_two_position_attributes(flavour):
    import inspect

    from ragraph_amd.RAGraph_fewshot import PositionAwareEncoder, ToyGraphBaseFewShot
    from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase

    tgb = ToyGraphBase(None, 3, 8, 3, device="cpu", flavour=flavour)
    assert tgb.position_rounds is None and tgb.last_position_converged is None
    few = ToyGraphBaseFewShot(None, 3, 8, 3, 5, device="cpu")
    assert few.position_rounds is None and few.last_position_converged is None
    assert inspect.signature(PositionAwareEncoder.encode_position_aware_code).parameters["rounds"].default is None
