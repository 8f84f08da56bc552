"""tests/guarded_workspace.py on host tensors (no device needed): the exact view, the detection of a write one byte in front
of and one byte behind a workspace -- the only place where a guard is dirtied on purpose; no test writes outside a
workspace on the GPU -- and the completeness of the table of tests/test_gpu_workspace_contracts.py: every function of
ragraph_amd/kernels.py that asks kernels._workspace for scratch memory has at least one guarded case there."""
import ast
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_workspace as GW  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@pytest.mark.parametrize("fill", GW.FILLS)
@pytest.mark.parametrize("nbytes", [0, 1, 511, 512, 513, 4096, 100_003])
def test_view_is_exact_aligned_and_filled(fill, nbytes):
    gw = GW.GuardedWorkspace(fill=fill)
    ws = gw(nbytes, CPU)
    assert ws.dtype == torch.uint8 and ws.numel() == nbytes and ws.is_contiguous()
    buf, asked, given = gw.requests[0]
    assert asked == nbytes and given == nbytes
    assert buf.numel() == GW.G + GW.align_up(nbytes) + GW.G and GW.align_up(nbytes) % 512 == 0
    assert GW.align_up(nbytes) - nbytes in range(512)
    if nbytes:   # (torch gives every EMPTY tensor a null data_ptr: a 0-byte request passes a null workspace of 0 bytes)
        assert ws.data_ptr() - buf.data_ptr() == GW.G and GW.G % 512 == 0   # the allocation's base + a multiple of 512
    assert bool((buf == fill).all())
    assert gw.check() == 1 and gw.interior_untouched()
    ws2 = gw(nbytes + 7, CPU)
    assert ws2.numel() == nbytes + 7 and ws2.data_ptr() != ws.data_ptr()   # a fresh buffer per request
    assert gw.check() == 2
    if nbytes:
        ws.fill_(fill ^ 0x5A)          # writing ALL of the workspace is what an entry may do
        assert gw.check() == 2 and not gw.interior_untouched()


def test_short_view_is_one_byte_short_and_zero_requests_are_left_alone():
    gw = GW.GuardedWorkspace(fill=0xA5, short=True)
    assert gw(0, CPU).numel() == 0
    ws = gw(1000, CPU)
    assert ws.numel() == 999 and ws.data_ptr() - gw.requests[1][0].data_ptr() == GW.G
    assert gw(1, CPU).numel() == 0
    assert gw.check() == 3 and gw.interior_untouched()
    assert [v.numel() for v in gw.views()] == [0, 999, 0]


def test_fill_is_one_of_the_three():
    with pytest.raises(ValueError):
        GW.GuardedWorkspace(fill=0x11)


@pytest.mark.parametrize("fill", GW.FILLS)
@pytest.mark.parametrize("nbytes", [1, 512, 777])
def test_a_write_one_byte_outside_is_detected_and_located(fill, nbytes):
    for where, offset in (("behind", 0), ("in front of", -nbytes - 1)):
        gw = GW.GuardedWorkspace(fill=fill)
        gw(64, CPU)                     # request 0 stays clean
        gw(nbytes, CPU)
        buf = gw.requests[1][0]
        buf[GW.G + nbytes + offset] = fill ^ 0xFF      # one host byte, end + offset
        assert gw.dirty() == [(1, nbytes, offset)]
        with pytest.raises(AssertionError) as e:
            gw.check()
        msg = str(e.value)
        assert f"request 1 of {nbytes} bytes" in msg and f"workspace end {offset:+d}" in msg and where in msg
        assert gw.interior_untouched()


def test_a_write_of_the_last_interior_byte_is_not_an_overrun():
    gw = GW.GuardedWorkspace(fill=0xFF)
    ws = gw(777, CPU)
    ws[776] = 0
    ws[0] = 0
    assert gw.check() == 1 and not gw.interior_untouched()


def test_far_overrun_is_located_at_its_first_byte():
    gw = GW.GuardedWorkspace(fill=0x00)
    gw(100, CPU)
    buf = gw.requests[0][0]
    buf[GW.G + 100 + 300:GW.G + 100 + 400] = 1
    buf[-1] = 1
    assert gw.dirty() == [(0, 100, 300)]


ALLOCATORS = ("_workspace", "_hub_workspace")   # _hub_workspace: the hub-row workspace of the CSR wrappers, from _workspace


def _functions_calling_workspace():
    """The functions that ask for scratch memory: from _workspace itself, or through the one private helper that does
    nothing but size a workspace and ask _workspace for it (the helper is checked to do so, and is no wrapper itself)."""
    with open(os.path.join(ROOT, "ragraph_amd", "kernels.py")) as f:
        tree = ast.parse(f.read())
    names = set()
    for fn in ast.walk(tree):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
            for node in ast.walk(fn):
                if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in ALLOCATORS:
                    names.add(fn.name)
    assert "_hub_workspace" in names     # (it calls _workspace: a guarded allocator reaches its callers)
    return names - {"_hub_workspace"}


def test_every_wrapper_that_takes_a_workspace_has_a_guarded_case():
    """A wrapper added later cannot ship without a case: the set of functions of kernels.py whose body calls _workspace(
    must equal the set of wrapper names that the GPU table declares."""
    import test_gpu_workspace_contracts as T

    found = _functions_calling_workspace()
    assert "_workspace" not in found and len(found) >= 30
    declared = T.declared_wrappers()
    assert found - declared == set(), f"wrappers without a guarded case: {sorted(found - declared)}"
    assert declared - found == set(), f"cases for functions that take no workspace: {sorted(declared - found)}"
    short = T.short_wrappers()
    assert found - short == set(), f"wrappers without a short-workspace case: {sorted(found - short)}"
