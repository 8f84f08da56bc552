#!/usr/bin/env python3
"""Ordered top-k beyond k = 64 (csrc/topk_large.hip), on one GPU.  Device-event times after warm-up, medians, A/B
alternated on the same matrix:
  (a) selection alone over a [1024, 1 M] fp32 matrix at k in {128, 1024, 4096}: topk_rows (ordered, large-k kernel)
      next to topk_select_rows (the unordered set, five passes);
  (b) topk_cosine at 1 M x 256, B = 1024, k = 128, and its split: the dense kernel over one [256, 1 M] slab and the
      selection of that slab (four slabs per call);
  (c) the node flavour's retrieval at an ogbn-arxiv-like shape (169 343 queries against a 169 343 x 256 bank) at
      k = 41 (retrieve_num = num_class + 1; 32 < k <= 64 already takes score slabs + topk_rows) and k = 82 (noise:
      2 x retrieve_num, score slabs + the large-k selection).

Usage:  python tools/topk_large_probe.py [--only abc] [--reps 5]
        python tools/topk_large_probe.py --counters K   (under rocprofv3: two topk_rows calls at k = K and one
                                                        topk_select_rows call on the (a) matrix, nothing timed)"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragraph_amd import kernels as K  # noqa: E402
from ragraph_amd.ragraph_utils import ToyGraphBase  # noqa: E402


def ev_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="abc")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--counters", type=int, default=0, metavar="K")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    if args.counters:
        S = torch.randn(1024, 1 << 20, device=dev, generator=g)
        for _ in range(2):
            K.topk_rows(S, args.counters)
        K.topk_select_rows(S, args.counters)
        torch.cuda.synchronize()
        return
    print(f"device: {torch.cuda.get_device_name(0)}; medians of {args.reps} after one warm-up call")

    if "a" in args.only:
        B, N = 1024, 1 << 20
        S = torch.randn(B, N, device=dev, generator=g)
        gb = B * N * 4 / 1e9
        print(f"(a) selection over [{B}, {N}] fp32 ({gb:.2f} GB)")
        for k in (128, 1024, 4096):
            t_sel, t_ord = [], []
            for _ in range(2):   # A/B alternated
                t_sel.append(ev_ms(lambda: K.topk_select_rows(S, k), args.reps))
                t_ord.append(ev_ms(lambda: K.topk_rows(S, k), args.reps))
            ts, to = min(t_sel), min(t_ord)
            print(f"    k={k:5d}  topk_select_rows {ts:8.3f} ms ({gb / ts:6.2f} TB/s)   topk_rows (ordered) {to:8.3f} ms "
                  f"({gb / to:6.2f} TB/s)   ratio {to / ts:.2f}")
        del S

    if "b" in args.only:
        B, N, D, k = 1024, 1 << 20, 256, 128
        kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
        q = torch.randn(B, D, device=dev, generator=g)
        t_all = ev_ms(lambda: K.topk_cosine(q, kn, k), args.reps)
        qn = K.normalize_rows(q[:256])
        t_dense = ev_ms(lambda: K.linear(qn, kn), args.reps)
        S = K.linear(qn, kn)
        t_sel = ev_ms(lambda: K.topk_rows(S, k), args.reps)
        print(f"(b) topk_cosine {N} x {D}, B={B}, k={k}: {t_all:.3f} ms (4 slabs of 256 queries)")
        print(f"    per slab: dense kernel {t_dense:.3f} ms, ordered selection {t_sel:.3f} ms "
              f"(selection / dense = {t_sel / t_dense:.2f})")
        del kn, S

    if "c" in args.only:
        n, D = 169343, 256
        keys = torch.randn(n, D, device=dev, generator=g)
        tgb = ToyGraphBase(None, 40, D, 3, device=dev)
        tgb.add_resources(keys, torch.randn(n, D, device=dev, generator=g),
                          torch.nn.functional.one_hot(torch.randint(0, 40, (n,), device=dev, generator=g), 40).float())
        q = keys + 0.5 * torch.randn(n, D, device=dev, generator=g)
        t41 = ev_ms(lambda: tgb.topk(q, 41), args.reps)
        t82 = ev_ms(lambda: tgb.topk(q, 82), args.reps)
        print(f"(c) node retrieval, {n} queries x {n} keys x {D}: k=41 {t41:.2f} ms, k=82 {t82:.2f} ms "
              f"(x{t82 / t41:.1f})")


if __name__ == "__main__":
    main()
