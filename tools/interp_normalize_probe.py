#!/usr/bin/env python3
"""The interpolative update at the c5 table shape (n = 4 000 000 rows x D = 64), S tables, three ways on one GPU
(profiles/edge_stages.txt):

  fused        kernels.interp_normalize: S tables read, one written
  composition  the existing entries whose bits it has: axpby chain + normalize_rows (3 (S - 1) + 2 passes)
  torch        the reference's lines, finetune_rag.py:83-86: F.normalize(torch.sum(torch.stack(tables) * w, dim=0), dim=1)

The three alternate inside one process after all are warm: ROUNDS x (fused, composition, torch), each a window of as many
back-to-back calls as fill >= WINDOW_S seconds, timed with device events.  Printed per variant: the median, the lowest and
the highest window (ms per call), the fraction of the HBM peak (8.0 TB/s) that (S + 1) * n * D * 4 bytes in the median time
amount to, and the peak memory one call allocates beyond the S input tables (its result included).

Usage:  python tools/interp_normalize_probe.py [--rows N] [--dim D] [--tables 2 4] [--rounds R]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragraph_amd import kernels as K  # noqa: E402
from ragraph_amd.edge_train import interpolation_weights  # noqa: E402

WINDOW_S = 0.5
HBM_PEAK = 8.0e12


def variants(tables, w):
    wl = w.tolist()
    wd = w.to(tables[0].device).unsqueeze(1).unsqueeze(1)

    def fused():
        return K.interp_normalize(tables, wl)

    def composition():
        acc = K.axpby(tables[0], wl[0], tables[1], wl[1])
        for t, ws in zip(tables[2:], wl[2:]):
            acc = K.axpby(acc, 1.0, t, ws)
        return K.normalize_rows(acc)

    def torch_chain():
        return F.normalize(torch.sum(torch.stack(tables) * wd, dim=0), dim=1)

    return {"fused": fused, "composition": composition, "torch": torch_chain}


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--tables", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, D = a.rows, a.dim
    for S in a.tables:
        g = torch.Generator(device=dev).manual_seed(S)
        tables = [torch.randn(n, D, device=dev, generator=g) for _ in range(S)]
        fns = variants(tables, interpolation_weights(S - 1))
        ref = fns["fused"]()
        same = torch.equal(ref.view(torch.int32), fns["composition"]().view(torch.int32))
        err = float((ref - fns["torch"]()).abs().max())
        del ref
        calls, extra = {}, {}
        for name, fn in fns.items():                                  # warm, size the window, peak memory of one call
            fn()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            extra[name] = torch.cuda.max_memory_allocated() - base
            calls[name] = max(3, int(WINDOW_S * 1e3 / window(fn, 3)) + 1)
        times = {name: [] for name in fns}
        for _ in range(a.rounds):
            for name, fn in fns.items():
                times[name].append(window(fn, calls[name]))
        nbytes = (S + 1) * n * D * 4
        print(f"S = {S}, n = {n}, D = {D}: {nbytes / 1e9:.3f} GB moved at least; fused == composition bit for bit: {same}; "
              f"max |fused - torch| = {err:.2e}")
        for name in fns:
            t = times[name]
            med = statistics.median(t)
            print(f"  {name:12s} median {med:7.3f} ms  (min {min(t):7.3f}, max {max(t):7.3f}; {a.rounds} windows of {calls[name]} "
                  f"calls)  {nbytes / (med * 1e-3) / HBM_PEAK * 100:5.1f} % of 8.0 TB/s on (S + 1) n D 4 bytes  "
                  f"peak extra memory {extra[name] / 2 ** 30:.2f} GiB")
        print(f"  fused vs composition x{statistics.median(times['composition']) / statistics.median(times['fused']):.2f} "
              f"(the byte counts predict x{(3 * S - 1) / (S + 1):.2f}), vs torch "
              f"x{statistics.median(times['torch']) / statistics.median(times['fused']):.2f}")
        del tables, fns


if __name__ == "__main__":
    main()
