"""What a tail behind a sealed bank costs, and what an append costs with and without one (profiles/bank_append.txt).

  python tools/bank_append_probe.py [--rows 1000000] [--dim 256] [--k 10] [--out FILE]

Bank: unit rows of a seeded normal draw, as tools/bench_blocks.py builds its synthetic bank; queries: normal draws, four
distinct batches per size.  Times are device events around windows of at least --window seconds after warming every shape;
the tail lengths of one batch size are timed alternately, twice, in this process, and the smaller time is reported.

1. launches of ragraph_topk_cosine_tail_f32 per shape (from its plan: one kernel, plus a memset node when the tail is cut
   into slices);
2. steady state: a KeyIndex.topk call with a tail of T rows against the same call without one;
3. append 40 rows, then query: wall-clock until the next topk call has completed, (a) with the tail, (b) sealing at once
   (what RAGRAPH_BANK_TAIL=0 does), (c) dropping the caches and the index as add_resources did before there was a tail; and
   the calls that ran with a bound pass (no learnt prior) from the append on."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ragraph_amd import _native as N   # noqa: E402
from ragraph_amd import kernels as K   # noqa: E402
from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase   # noqa: E402

TAILS = (0, 40, 512, 4096, 16384, 65536)
BATCHES = (1, 16, 512, 4096, 100000)


def window(fn, seconds):
    """ms per call of fn over a window of at least `seconds` (device events; fn was warmed by the caller)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(3):
        fn()
    b.record()
    b.synchronize()
    n = max(3, int(seconds * 1000.0 / max(a.elapsed_time(b) / 3, 1e-3)) + 1)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    Nr, D, k = args.rows, args.dim, args.k
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device=dev).manual_seed(1)
    rows = K.normalize_rows(torch.nn.functional.normalize(torch.randn(Nr + max(TAILS), D, device=dev, generator=g), dim=-1))
    queries = {B: [torch.randn(B, D, device=dev, generator=g) for _ in range(4)] for B in BATCHES}
    L = N.lib()
    say(f"bank {Nr} x {D}, k = {k}; {torch.cuda.get_device_name(0)}")

    say("\n== 1. launches of the tail entry (kernel + memset node in front of a sliced tail) ==")
    say("     B " + "".join(f"{'T=' + str(T):>12}" for T in TAILS[1:]))
    for B in (1, 16, 512, 100000):
        cells = []
        for T in TAILS[1:]:
            sliced = L.ragraph_topk_cosine_tail_workspace_bytes(B, T, D, k) > 256
            cells.append("1 + memset" if sliced else "1")
        say(f"{B:>6} " + "".join(f"{c:>12}" for c in cells))

    say("\n== 2. steady state: ms per KeyIndex.topk call with a tail of T rows (ratio to T = 0) ==")
    indexes = {}
    for T in TAILS:
        index = K.KeyIndex(rows[:Nr])
        index.TAIL_MAX_ROWS = 1 << 30          # (this sweep is what chooses the limit)
        if T:
            index.extend(rows[:Nr + T])
            assert index.tail_rows == T
        indexes[T] = index
    say("     B " + "".join(f"{'T=' + str(T):>16}" for T in TAILS))
    table = {}
    for B in BATCHES:
        qs = queries[B]
        calls = {}
        for T in TAILS:
            state = {"i": 0}

            def call(index=indexes[T], state=state):
                state["i"] += 1
                return index.topk(qs[state["i"] & 3], k)

            for _ in range(8):                 # warm: copies, duplicate judgement, the learnt prior
                call()
                torch.cuda.synchronize()
            calls[T] = call
        best = {T: float("inf") for T in TAILS}
        for _ in range(2):
            for T in TAILS:
                best[T] = min(best[T], window(calls[T], args.window))
        table[B] = best
        say(f"{B:>6} " + "".join(f"{best[T]:>9.4f} ({best[T] / best[0]:4.2f})" for T in TAILS))
    ok = [T for T in TAILS[1:] if all(table[B][T] <= 1.10 * table[B][0] for B in (4096, 100000))]
    say(f"largest swept T within 1.10 x the T = 0 call at B = 4096 and B = 100000: {max(ok) if ok else 'none'}")
    for B in (1, 16):
        say(f"added latency at B = {B}: " + ", ".join(f"T={T}: {1000 * (table[B][T] - table[B][0]):+.1f} us" for T in TAILS[1:]))
    del indexes

    say("\n== 3. append 40 rows, then query: wall-clock ms until the next topk call has completed (median of 3) ==")
    say("     B      tail  bound-pass calls |  seal at once  bound-pass calls |  caches + index dropped  bound-pass calls")
    for B in (16, 4096, 100000):
        qs = queries[B]
        tgb = ToyGraphBase(None, 3, D, 3, device=dev)
        labels = torch.zeros(Nr, 3, device=dev)
        tgb.set_resources(rows[:Nr], rows[:Nr], labels)
        new = rows[Nr:Nr + 40]
        new_l = torch.zeros(40, 3, device=dev)
        tgb.topk(qs[0], k)
        tgb.add_resources(new, new, new_l)       # (the stores' first reallocation behind adopted tensors: not what is measured)
        times = {"tail": [], "seal": [], "drop": []}
        passes = {"tail": [], "seal": [], "drop": []}
        for _ in range(3):
            for variant in ("tail", "seal", "drop"):
                for i in range(8):               # a warm index before every append
                    tgb.topk(qs[i & 3], k)
                    torch.cuda.synchronize()
                index = tgb._index
                index.seal()
                index.tail_enabled = variant == "tail"
                for i in range(4):
                    tgb.topk(qs[i & 3], k)
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                tgb.add_resources(new, new, new_l)
                if variant == "drop":
                    tgb._keys_normalized = tgb._positions_normalized = tgb._index = tgb._kn_store = None
                tgb.topk(qs[0], k)
                torch.cuda.synchronize()
                times[variant].append(1000 * (time.perf_counter() - t0))
                n_pass = 0 if tgb._index.last_prior is not None else 1
                for i in range(1, 12):
                    tgb.topk(qs[i & 3], k)
                    torch.cuda.synchronize()
                    if tgb._index.last_prior is not None:
                        break
                    n_pass += 1
                passes[variant].append(n_pass)
                tgb._index.tail_enabled = True
        med = lambda v: sorted(v)[len(v) // 2]
        say(f"{B:>6} " + " | ".join(f"{med(times[v]):>9.3f}  {str(passes[v]):>16}" for v in ("tail", "seal", "drop")))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
