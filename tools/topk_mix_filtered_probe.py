#!/usr/bin/env python3
"""Mixed retrieval through the filter (KeyIndex.topk_mix: filtered semantic top-k', K.topk_mix_rerank, one read-back, exact
repair) against the exact fused call it falls back to (K.topk_cosine_mix), on the data of profiles/topk_mix.txt: Gaussian
embeddings, codes 1 / (d + 1) with 30 % unreachable anchors, A = 10.  Both run through ToyGraphBase.topk in one process and
alternate; RAGRAPH_MIX_FILTER is toggled per call.  A measurement is a window of back-to-back calls between two device events
(the route's read-back lies inside its window) that lasts at least --window-ms (one call where a call is longer), behind a
warm-up of both that also lets the filter learn its priors; every pair is repeated and printed with its spread, the unproven
share of the route's calls and whether the two results are equal bit for bit.  The measured rule (K.mix_filter_measured) is
opened for the probe and a demotion is cleared before every routed call, so that the route itself is what is timed.
Section 2 forces a share of unproven rows (flags set behind the kernel) at the weights (0.001, 0.999), where none arise, to
price the repair: KeyIndex.MIX_FILTER_MAX_UNPROVEN is the largest of 1/16, 1/8, 1/4, 1/2 at which the route still wins by
more than the spread at B = 4096 and at B = 100 000 (N = 1M, D = 256).

    python tools/topk_mix_filtered_probe.py --out profiles/topk_mix_filtered.txt [--reps 3] [--window-ms 200]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragraph_amd import kernels as K  # noqa: E402
from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase  # noqa: E402

BATCHES = (16, 256, 4096, 100_000)
BANKS = (65_536, 1 << 20)
WIDTHS = (128, 256)
KS = (10, 20, 40)
WEIGHTS = ((0.001, 0.999), (0.05, 0.95), (0.3, 0.7))
SHARES = (1 / 16, 1 / 8, 1 / 4, 1 / 2)
A = 10


def codes(n, dev, g):
    d = torch.randint(0, 7, (n, A), device=dev, generator=g).float()
    c = 1.0 / (d + 1.0)
    c[torch.rand(n, A, device=dev, generator=g) < 0.3] = 0.0
    return c


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def calls_for(fn, window_ms, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    one = max(window(fn, 1), window(fn, 2), 1e-3)
    return max(1, min(5000, int(window_ms / one) + 1))


def fmt(xs):
    return f"{statistics.median(xs):9.3f} ms (min {min(xs):9.3f}, max {max(xs):9.3f})"


def contenders(tgb, q, pq, k):
    def routed():
        os.environ["RAGRAPH_MIX_FILTER"] = "1"
        tgb._index._mix_demoted.clear()
        return tgb.topk(q, k, pq)

    def exact():
        os.environ["RAGRAPH_MIX_FILTER"] = "0"
        return tgb.topk(q, k, pq)

    return routed, exact


def pair(say, label, tgb, q, pq, k, reps, window_ms):
    """One alternating pair; returns (verdict, median exact / median routed, unproven share)."""
    routed, exact = contenders(tgb, q, pq, k)
    ref = exact()
    st = tgb._index.mix_stats
    before = dict(st)
    got = routed()
    torch.cuda.synchronize()
    if st["filtered_calls"] == before["filtered_calls"]:
        say(f"   {label}  route not open for this call (the index sends lists of {K.mix_filter_list(k)} keys to "
            f"{tgb._index._route(q.shape[0], tgb._index.sealed_rows, q.shape[1], K.mix_filter_list(k))}): exact call only")
        return "closed", None, None
    share = (st["rows_unproven"] - before["rows_unproven"]) / q.shape[0]
    same = torch.equal(got[1], ref[1]) and torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32))
    del ref, got
    nr, ne = calls_for(routed, window_ms, 3), calls_for(exact, window_ms, 1)
    tr, te = [], []
    for _ in range(reps):                                   # exact, routed, exact, routed, ...
        te.append(window(exact, ne))
        tr.append(window(routed, nr))
    spread = max(max(tr) - min(tr), max(te) - min(te))
    gain = statistics.median(te) - statistics.median(tr)
    verdict = "ROUTE" if gain > spread else ("exact" if -gain > spread else "draw")
    ratio = statistics.median(te) / statistics.median(tr)
    say(f"   {label}  exact  {fmt(te)}  ({ne} calls per window)\n   {' ' * len(label)}  routed {fmt(tr)}  ({nr} calls per window)   "
        f"unproven share {share:.4f}   equal bits: {same}\n   {' ' * len(label)}  exact - routed = {gain:+.3f} ms, spread of the pair "
        f"{spread:.3f} ms, exact / routed = {ratio:.2f}  -> {verdict}")
    return verdict, ratio, share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/topk_mix_filtered.txt")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--skip-grid", action="store_true", help="section 2 (the threshold) only")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K.mix_filter_measured = lambda *shape: True             # the probe times the route wherever the index can take it
    K.KeyIndex.MIX_FILTER_MAX_UNPROVEN = 2.0                # (and never lets a call demote it)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                      # (kept current: a run that is cut short leaves what it measured)
            f.write("\n".join(lines) + "\n")

    say(f"# tools/topk_mix_filtered_probe.py on {torch.cuda.get_device_name(0)}: exact = K.topk_cosine_mix, routed = KeyIndex.topk_mix "
        "(filtered semantic top-k', rerank + proof, read-back, exact repair of unproven rows), both through ToyGraphBase.topk.")
    say(f"# {args.reps} alternating windows per pair behind a warm-up of both; a window is back-to-back calls between two device "
        f"events for >= {args.window_ms:.0f} ms; ms per call, median (min, max); ROUTE / exact: faster by more than the spread of the pair.")
    results = {}
    for N in BANKS:
        for D in WIDTHS:
            g = torch.Generator(device=dev).manual_seed(N + D)
            keys = torch.randn(N, D, device=dev, generator=g)
            tgb = ToyGraphBase(None, 3, D, 3, device=dev)
            tgb.set_resources(keys, keys, torch.zeros(N, 3, device=dev), codes(N, dev, g))
            del keys
            for B in BATCHES:
                q, pq = torch.randn(B, D, device=dev, generator=g), codes(B, dev, g)
                if not args.skip_grid:
                    say(f"\n== {B} queries x {N} keys x {D}")
                    for k in KS:
                        for ws, wm in WEIGHTS:
                            tgb.structure_weight, tgb.semantic_weight = ws, wm
                            results[(B, N, D, k, ws)] = pair(say, f"k = {k:2d} ({ws}, {wm})", tgb, q, pq, k, args.reps, args.window_ms)
                if N == 1 << 20 and D == 256 and B in (4096, 100_000):
                    say(f"\n== forced unproven share, {B} queries x {N} keys x {D}, k = 10, weights (0.001, 0.999)")
                    tgb.structure_weight, tgb.semantic_weight = 0.001, 0.999
                    real = K.topk_mix_rerank
                    for share in SHARES:
                        m = int(round(share * B))

                        def forced(*a, _m=m, **kw):
                            s, i, flags, count = real(*a, **kw)
                            flags[:_m] = 1
                            return s, i, flags, flags.sum(dtype=torch.int32).reshape(1)

                        K.topk_mix_rerank = forced
                        try:
                            results[("share", B, share)] = pair(say, f"share {share:6.4f}", tgb, q, pq, 10, args.reps, args.window_ms)
                        finally:
                            K.topk_mix_rerank = real
                del q, pq
            del tgb
            torch.cuda.empty_cache()
    say("\n== summary")
    won = sorted(key for key, v in results.items() if key[0] != "share" and v[0] == "ROUTE")
    lost = sorted(key for key, v in results.items() if key[0] != "share" and v[0] in ("exact", "draw"))
    say(f"   ROUTE (B, N, D, k, w_struct): {won}")
    say(f"   exact or draw: {lost}")
    ok = [s for s in SHARES if all(results.get(("share", B, s), ("", 0, 0))[0] == "ROUTE" for B in (4096, 100_000))]
    say(f"   shares at which the route wins at both B = 4096 and B = 100 000: {ok}  -> largest: {max(ok) if ok else None}")


if __name__ == "__main__":
    main()
