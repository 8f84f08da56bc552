"""What retired rows behind a live index cost, and what a removal costs three ways (profiles/bank_remove.txt).

  python tools/bank_remove_probe.py --section steady|kernel|remove [--batches 1,16,...] [--rows 1000000] [--dim 256] [--k 10]
                                    [--out FILE]      (--out appends: one file collects the sections)

Bank: unit rows of a seeded normal draw, as tools/bank_append_probe.py builds it; queries: normal draws, four distinct batches per
size.  Times are device events around windows of at least --window seconds after warming every shape; the cases of one batch size
are timed alternately, twice, in this process, and the smaller time is reported.  Every section is a process of its own, so
that a caller can give each GPU step its own time limit (timeout -k 10 SECONDS python tools/bank_remove_probe.py --section ...).

steady  ms per KeyIndex.topk call with retired_rows in {0, 1, 22, 54} (k = 10: lists of 10, 11, 32 and 64 keys before the
        drop), and for 22 and 54 the ratio to 0 -- always against 0 retired rows in this same process;
kernel  ragraph_topk_drop_rows_f32 alone at B = 100 000, k_in = 32, k_out = k, on the lists of a real search;
remove  remove 40 rows, then query: wall-clock until the next top-k has completed, (a) tombstones (remove_resources, then the
        index's own topk: 40 retired rows cross the class ceiling of k = 10, where ToyGraphBase.topk itself would compact),
        (b) remove_resources + ToyGraphBase.topk, which compacts (compact() + KeyIndex.rebase), (c) set_resources over the
        survivors, gathered by the same K.gather_rows; and the calls that ran with a bound pass (no learnt prior) from there on."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ragraph_amd import kernels as K   # noqa: E402
from ragraph_amd.ragraph_utils.ToyGraphBase import ToyGraphBase   # noqa: E402

RETIRED = (0, 1, 22, 54)
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
    ap.add_argument("--section", choices=("steady", "kernel", "remove"), required=True)
    ap.add_argument("--batches", default=None, help="comma-separated batch sizes (default: the section's own)")
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
    rows = K.normalize_rows(torch.nn.functional.normalize(torch.randn(Nr, D, device=dev, generator=g), dim=-1))
    batches = tuple(int(b) for b in args.batches.split(",")) if args.batches else None
    gone = torch.randperm(Nr, generator=torch.Generator().manual_seed(2))[:max(RETIRED)]   # host ids, the same in every section
    say(f"[{args.section}] bank {Nr} x {D}, k = {k}; {torch.cuda.get_device_name(0)}")

    if args.section == "steady":
        say("== ms per KeyIndex.topk call with r retired rows (ratio to r = 0, same process, cases alternated) ==")
        say("     B " + "".join(f"{'r=' + str(r):>16}" for r in RETIRED))
        indexes = {}
        for r in RETIRED:
            indexes[r] = K.KeyIndex(rows)
            indexes[r].retire(gone[:r])
            assert indexes[r].retired_rows == r
        for B in batches or BATCHES:
            qs = [torch.randn(B, D, device=dev, generator=g) for _ in range(4)]
            calls = {}
            for r in RETIRED:
                state = {"i": 0}

                def call(index=indexes[r], state=state):
                    state["i"] += 1
                    return index.topk(qs[state["i"] & 3], k)

                for _ in range(8):                 # warm: copies, duplicate judgement, the learnt prior of this list length
                    call()
                    torch.cuda.synchronize()
                calls[r] = call
            best = {r: float("inf") for r in RETIRED}
            for _ in range(2):
                for r in RETIRED:
                    best[r] = min(best[r], window(calls[r], args.window))
            say(f"{B:>6} " + "".join(f"{best[r]:>9.4f} ({best[r] / best[0]:4.2f})" for r in RETIRED))

    elif args.section == "kernel":
        B, k_in = (batches or (100000,))[0], 32
        q = torch.randn(B, D, device=dev, generator=g)
        index = K.KeyIndex(rows)
        s, i = index.topk(q, k_in)
        bitmap = K.retire_rows(K.retired_bitmap(Nr, dev), gone[:k_in - k].to(dev), Nr)
        bitmap = K.retire_rows(bitmap, i[::7, 0].contiguous(), Nr)      # every seventh query loses its best hit as well
        for _ in range(3):
            K.topk_drop_rows(s, i, bitmap, Nr, k)
        torch.cuda.synchronize()
        ms = window(lambda: K.topk_drop_rows(s, i, bitmap, Nr, k), args.window)
        moved = 12 * B * (k_in + k) / 1e6
        say(f"== topk_drop_rows alone (its memset of the short_lists word included): B = {B}, k_in = {k_in}, k_out = {k} ==")
        say(f"{1000 * ms:.1f} us per call; model 12 B (k_in + k_out) = {moved:.1f} MB -> {moved / ms / 1e3:.2f} TB/s if every entry were read")

    else:
        say("== remove 40 rows, then query: wall-clock ms until the next top-k has completed (median of 3) ==")
        say("     B  tombstones  bound-pass calls |  compact()  bound-pass calls |  set_resources(survivors)  bound-pass calls")
        labels = torch.zeros(Nr, 3, device=dev)
        ids = gone[:40]
        for B in batches or (16, 4096, 100000):
            qs = [torch.randn(B, D, device=dev, generator=g) for _ in range(4)]
            times = {v: [] for v in ("tomb", "compact", "set")}
            passes = {v: [] for v in ("tomb", "compact", "set")}
            for _ in range(3):
                for variant in ("tomb", "compact", "set"):
                    tgb = ToyGraphBase(None, 3, D, 3, device=dev)
                    tgb.set_resources(rows, rows, labels)
                    for i in range(8):               # a warm index before every removal
                        tgb.topk(qs[i & 3], k)
                        torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if variant == "tomb":
                        tgb.remove_resources(ids)
                        top = tgb._index.topk
                    elif variant == "compact":
                        tgb.remove_resources(ids)
                        top = lambda q, kk: tgb.topk(q, kk)
                    else:
                        live = torch.ones(Nr, dtype=torch.bool, device=dev)
                        live[ids.to(dev)] = False
                        pos = K.mask_positions(live)
                        tgb.set_resources(K.gather_rows(rows, pos), K.gather_rows(rows, pos), K.gather_rows(labels, pos))
                        top = lambda q, kk: tgb.topk(q, kk)
                    top(qs[0], k)
                    torch.cuda.synchronize()
                    times[variant].append(1000 * (time.perf_counter() - t0))
                    if variant == "compact":
                        assert tgb.retired_rows == 0 and tgb.resource_keys.shape[0] == Nr - 40
                    n_pass = 0 if tgb._index.last_prior is not None else 1
                    for i in range(1, 12):
                        top(qs[i & 3], k)
                        torch.cuda.synchronize()
                        if tgb._index.last_prior is not None:
                            break
                        n_pass += 1
                    passes[variant].append(n_pass)
                    del tgb
            med = lambda v: sorted(v)[len(v) // 2]
            say(f"{B:>6} " + " | ".join(f"{med(times[v]):>9.3f}  {str(passes[v]):>16}" for v in ("tomb", "compact", "set")))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
