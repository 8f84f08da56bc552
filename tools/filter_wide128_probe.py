#!/usr/bin/env python3
"""Lists of 65 .. 128 keys: the wide128 filtered call against the fp32 score slabs it replaces (K.topk_cosine), over the shapes
of profiles/filter_wide.txt at k = 65 / 96 / 128.  The two contenders alternate inside one process; every measurement is a
window of back-to-back calls between two device events that lasts at least 0.5 s (one call where a call is longer), behind a
warm-up of both; every pair is repeated and printed with its spread, with the candidates per query and level, whether a list
overflowed, and whether the wide128 result equals the slab result bit for bit.  kernels.filter_wide128_helps keeps a shape
class only where this file shows the wide128 call faster by more than that spread.

    python tools/filter_wide128_probe.py --out profiles/filter_wide128.txt [--reps 3] [--quick]
    python tools/filter_wide128_probe.py --below65 [--bench-line FILE]    # the no-regression rows: 100 000 x 1M x 256 at k = 41 / 64
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragraph_amd import kernels as K  # noqa: E402

SHAPES = [(256, 1_000_000, 256), (4096, 1_000_000, 256), (100_000, 1_000_000, 256), (4096, 4_000_000, 64)]
QUICK = [(600, 70_000, 256), (256, 70_000, 256), (4096, 200_000, 128), (1, 1_000_000, 256), (16, 1_000_000, 256),
         (64, 1_000_000, 256), (16, 70_000, 64),
         (128, 40_000, 256), (2100, 40_000, 256), (64, 40_000, 256),
         (700, 20_000, 128), (1024, 10_000, 256), (256, 10_000, 128),
         (2048, 20_000, 64), (1024, 16_384, 64), (8192, 10_000, 64), (2708, 10_000, 64)]
WINDOW_MS = 500.0


def window(fn, calls):
    """ms per call over `calls` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def calls_for(fn):
    """Warm-up, then how many calls fill a window."""
    fn()
    torch.cuda.synchronize()
    one = max(window(fn, 1), window(fn, 3), 1e-3)
    return max(1, min(20000, int(WINDOW_MS / one) + 1))


def fmt(xs):
    return f"{statistics.median(xs):9.3f} ms (min {min(xs):9.3f}, max {max(xs):9.3f})"


def bank(dev, B, N, D):
    g = torch.Generator(device=dev).manual_seed(B + N + D)
    kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
    return kn, K.keys_to_bf16(kn), torch.randn(B, D, device=dev, generator=g)


def below65(dev, reps):
    """The wide entry's row that must not move: printed by one process per library (RAGRAPH_HIP_SO), run alternately."""
    kn, kb, q = bank(dev, 100_000, 1_000_000, 256)
    for k in (41, 64):
        fn = lambda: K.topk_cosine_filtered(q, kn, kb, k)   # noqa: E731
        n = calls_for(fn)
        ts = [window(fn, n) for _ in range(reps)]
        print(f"100000 x 1000000 x 256  k = {k}  wide {fmt(ts)}  ({n} calls per window)  lib = {K.N.SO_PATH}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/filter_wide128.txt")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="also the small banks at the lower edge of the dispatch rule")
    ap.add_argument("--below65", action="store_true", help="only the k = 41 / 64 rows of 100 000 x 1M x 256 (before / after runs)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.below65:
        below65(dev, args.reps)
        return
    lines = [f"# tools/filter_wide128_probe.py on {torch.cuda.get_device_name(0)}: slab = K.topk_cosine (fp32 score slabs), w128 = "
             "K.topk_cosine_filtered at 64 < k <= 128.", f"# {args.reps} alternating windows per pair behind a warm-up of both; a "
             "window is back-to-back calls between two device events for >= 0.5 s; ms per call, median (min, max);",
             "# 'exact': w128 == slab, bit for bit; candidates per query and level: sampled mean, b = bf16 level, i = int8 level."]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for B, N, D in SHAPES + (QUICK if args.quick else []):
        kn, kb, q = bank(dev, B, N, D)
        say(f"\n== {B} queries x {N} keys x {D}   (filter_wide128_helps at k = 65 / 96 / 128: "
            f"{[K.filter_wide128_helps(B, N, D, k) for k in (65, 96, 128)]})")
        for k in (65, 96, 128):
            slab = lambda: K.topk_cosine(q, kn, k)                      # noqa: E731
            wide = lambda: K.topk_cosine_filtered(q, kn, kb, k)         # noqa: E731
            ref = slab()
            s, i, over, st = K.topk_cosine_filtered(q, kn, kb, k, return_stats=True)
            torch.cuda.synchronize()
            exact = torch.equal(i, ref[1]) and torch.equal(s, ref[0])
            w = st.cpu().tolist()
            cand = " + ".join(f"{(w[2 + l] / w[5 + l]) if w[5 + l] else 0:.0f}{'i' if w[8 + l] else 'b'}" for l in range(w[1]))
            del ref, s, i
            ns, nw = calls_for(slab), calls_for(wide)
            ts, tw = [], []
            for _ in range(args.reps):                                  # slab, w128, slab, w128, ...
                ts.append(window(slab, ns))
                tw.append(window(wide, nw))
            spread = max(max(ts) - min(ts), max(tw) - min(tw))
            gain = statistics.median(ts) - statistics.median(tw)
            say(f"   k = {k:3d}  slab {fmt(ts)}  ({ns} calls per window)\n            w128 {fmt(tw)}  ({nw} calls per window)   "
                f"exact: {exact}  overflowed: {int(over)}  candidates per query and level: {cand}\n"
                f"            slab - w128 = {gain:+.3f} ms, spread of the pair {spread:.3f} ms, slab / w128 = "
                f"{statistics.median(ts) / statistics.median(tw):.2f}"
                f"  -> {'W128' if gain > spread else ('slab' if -gain > spread else 'draw')}")
        del kn, kb, q
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
