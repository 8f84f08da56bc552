#!/usr/bin/env python3
"""Lists of 33 .. 64 keys: the wide filtered call against the fp32 score slabs it replaces (K.topk_cosine), with the k = 32
filtered call of the same shape next to them.  Device events, a warm-up per shape, the contenders alternating inside one
process; every pair is repeated and printed with its spread, and every wide call is compared bit for bit with the slab result.
kernels.filter_wide_helps keeps a shape class only where this file shows the wide call faster by more than that spread.

    python tools/filter_wide_probe.py --out profiles/filter_wide.txt [--reps 5] [--quick]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragraph_amd import kernels as K  # noqa: E402

SHAPES = [(256, 1_000_000, 256), (4096, 1_000_000, 256), (100_000, 1_000_000, 256), (4096, 4_000_000, 64)]
# (--quick) every class of filter_helps' rule at k = 32, which filter_wide_helps starts from, and its neighbours outside the rule
QUICK = [(600, 70_000, 256), (256, 70_000, 256), (4096, 200_000, 128), (1, 1_000_000, 256), (16, 1_000_000, 256),
         (64, 1_000_000, 256), (16, 70_000, 64),                                       # >= 65 536 keys: every batch size
         (128, 40_000, 256), (2100, 40_000, 256), (64, 40_000, 256),                  # 32 768 ..: from 128 queries
         (700, 20_000, 128), (1024, 10_000, 256), (256, 10_000, 128),                 # 8192 ..: D >= 128 from 512 queries
         (2048, 20_000, 64), (1024, 16_384, 64), (8192, 10_000, 64), (2708, 10_000, 64)]   # D = 64: from 2048 / 8192 queries


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def fmt(xs):
    return f"{statistics.median(xs):9.3f} ms (min {min(xs):9.3f}, max {max(xs):9.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/filter_wide.txt")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="also the small banks at the lower edge of the dispatch rule")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"# tools/filter_wide_probe.py on {torch.cuda.get_device_name(0)}: slab = K.topk_cosine (fp32 score slabs), wide = "
             "K.topk_cosine_filtered at 32 < k <= 64,", f"# k32 = the filtered call of the same shape at k = 32.  {args.reps} "
             "alternating repetitions per pair behind one warm-up each; median (min, max); 'exact': wide == slab, bit for bit."]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for B, N, D in SHAPES + (QUICK if args.quick else []):
        g = torch.Generator(device=dev).manual_seed(B + N + D)
        kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
        kb = K.keys_to_bf16(kn)
        q = torch.randn(B, D, device=dev, generator=g)
        reps = args.reps if B * N < 5e10 else max(3, args.reps // 2)
        say(f"\n== {B} queries x {N} keys x {D}   (filter_helps at k = 32: {K.filter_helps(B, N, D, 32)}, "
            f"filter_wide_helps at k = 41: {K.filter_wide_helps(B, N, D, 41)})")
        K.topk_cosine_filtered(q, kn, kb, 32)
        torch.cuda.synchronize()
        t32 = [timed(lambda: K.topk_cosine_filtered(q, kn, kb, 32))[0] for _ in range(reps)]
        say(f"   k = 32  k32  {fmt(t32)}")
        for k in (33, 41, 64):
            ref = K.topk_cosine(q, kn, k)                       # warm-up of both, and the comparison
            s, i, over, st = K.topk_cosine_filtered(q, kn, kb, k, return_stats=True)
            torch.cuda.synchronize()
            exact = torch.equal(i, ref[1]) and torch.equal(s, ref[0])
            w = st.cpu().tolist()
            cand = " + ".join(f"{(w[2 + l] / w[5 + l]) if w[5 + l] else 0:.0f}{'i' if w[8 + l] else 'b'}" for l in range(w[1]))
            del ref, s, i
            ts, tw, t2 = [], [], []
            for _ in range(reps):                               # slab, wide, k32, slab, wide, k32, ...
                ts.append(timed(lambda: K.topk_cosine(q, kn, k))[0])
                tw.append(timed(lambda: K.topk_cosine_filtered(q, kn, kb, k))[0])
                t2.append(timed(lambda: K.topk_cosine_filtered(q, kn, kb, 32))[0])
            spread = max(max(ts) - min(ts), max(tw) - min(tw))
            gain = statistics.median(ts) - statistics.median(tw)
            say(f"   k = {k}  slab {fmt(ts)}\n           wide {fmt(tw)}   exact: {exact}  overflowed: {int(over)}  "
                f"candidates per query and level: {cand}\n           k32  {fmt(t2)}\n"
                f"           slab - wide = {gain:+.3f} ms, spread of the pair {spread:.3f} ms, slab / wide = "
                f"{statistics.median(ts) / statistics.median(tw):.2f}, wide / k32 = {statistics.median(tw) / statistics.median(t2):.2f}"
                f"  -> {'WIDE' if gain > spread else ('slab' if -gain > spread else 'draw')}")
        del kn, kb, q
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
