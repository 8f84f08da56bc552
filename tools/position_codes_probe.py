"""Position codes of large graphs: time per call and number of rounds (profiles/position_codes_global.txt).

One process.  Every timed call ends in a device synchronise (host clock around it: the eager global path reads a word back
between batches of rounds, so its host time is part of the call).  The modes of a shape alternate inside one loop after all of
them are warm; medians, min, max and every value are printed.  Rounds: the smallest R for which a fixed-round call reports
the converged word 1 (its last round is the one that changes nothing).

  python tools/position_codes_probe.py [--reps 9] [--shapes lds,c2,1m,c5,batch]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ragraph_amd import kernels as K          # noqa: E402
from ragraph_amd.graph import CSRGraph        # noqa: E402

DIS_Q, A = 10.0, 10


def random_graph(n, deg, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    rowptr = torch.arange(0, n * deg + 1, deg, device=dev, dtype=torch.int64)
    col = torch.randint(0, n, (n * deg,), device=dev, generator=g).to(torch.int32)
    val = torch.rand(n * deg, device=dev, generator=g) * 2.0 + 0.5
    return CSRGraph(rowptr, col, val, n)


def c2_graph(n, dev):
    from ragraph_amd.data import synthetic_big_graph

    return CSRGraph.from_edge_index_sym_normalized(synthetic_big_graph(n, 10, seed=8, device=dev), n)


def c5_shaped_graph(users, items, per_user, dev):
    """Bipartite, both directions, bi-normalised (D^-1/2 A D^-1/2): every user rates item 0 (the hub row: `users` edges) and
    per_user random other items."""
    g = torch.Generator(device=dev).manual_seed(10)
    u = torch.arange(users, device=dev).repeat_interleave(per_user + 1)
    i = torch.randint(1, items, (users, per_user + 1), device=dev, generator=g)
    i[:, 0] = 0
    i = i.reshape(-1) + users
    src, dst = torch.cat([u, i]), torch.cat([i, u])
    n = users + items
    deg = torch.bincount(src, minlength=n).float()
    val = deg[src].rsqrt() * deg[dst].rsqrt()
    graph, _ = CSRGraph.from_coo(src, dst, val, n)
    return graph


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(modes, reps):
    """modes: {name: callable}.  Warm each, then reps rounds of one call per mode in turn."""
    for fn in modes.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in modes}
    for _ in range(reps):
        for name, fn in modes.items():
            ms[name].append(timed(fn))
    for name, v in ms.items():
        med = statistics.median(v)
        print(f"  [{name:<24}] median {med:9.3f} ms   min {min(v):9.3f}  max {max(v):9.3f}  spread {(max(v) - min(v)) / med * 100:5.1f} %"
              f"   all: {' '.join(f'{x:.3f}' for x in v)}", flush=True)
    return {name: statistics.median(v) for name, v in ms.items()}


def rounds_to_converge(g, anchors):
    def ok(r):
        _, w = K.position_codes_csr(g.rowptr, g.col, g.val, anchors, DIS_Q, rounds=r, return_converged=True)
        return int(w.item()) == 1
    hi = 4
    while not ok(hi):
        hi *= 2
        if hi > g.n:
            return None
    lo = hi // 2 if hi > 4 else 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    return hi


def with_dirty(on, fn):
    def run():
        os.environ["RAGRAPH_POSITION_CODES_DIRTY"] = "1" if on else "0"
        try:
            return fn()
        finally:
            os.environ.pop("RAGRAPH_POSITION_CODES_DIRTY", None)
    return run


def describe(name, g):
    deg = g.rowptr[1:] - g.rowptr[:-1]
    print(f"{name}: n = {g.n}, nnz = {g.nnz}, longest row {int(deg.max())}, A = {A}", flush=True)


def shape(name, g, reps, lds=False, same_bits=True):
    describe(name, g)
    anchors = torch.randint(0, g.n, (A,), generator=torch.Generator().manual_seed(2)).to(g.device)
    call = lambda **kw: K.position_codes_csr(g.rowptr, g.col, g.val, anchors, DIS_Q, **kw)   # noqa: E731
    r = rounds_to_converge(g, anchors)
    print(f"  rounds to the fixpoint (the last one changes nothing): {r}", flush=True)
    modes = {}
    if lds:
        modes["lds kernel"] = lambda: call()
    modes["global, dirty bytes on"] = with_dirty(True, lambda: call(method="global"))
    modes["global, dirty bytes off"] = with_dirty(False, lambda: call(method="global"))
    if r is not None:
        modes[f"global, rounds={r} fixed"] = lambda: call(rounds=r)
    if same_bits:
        ref = call(method="global")
        off = with_dirty(False, lambda: call(method="global"))()
        assert torch.equal(ref, off), "dirty bytes change the result"
        if lds:
            assert torch.equal(ref, call()), "global path differs from the LDS kernel"
        print(f"  same bits in every mode; non-zero codes {float((ref != 0).float().mean()):.3f}", flush=True)
    return alternate(modes, reps), call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="lds,c2,1m,c5,batch")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no ROCm device: this probe measures on the GPU only")
    dev = torch.device("cuda:0")
    shapes = args.shapes.split(",")
    print(f"device: {torch.cuda.get_device_name(0)}; rounds per read-back = {K.POSITION_CODES_ROUNDS_PER_READBACK}; "
          f"reps = {args.reps}", flush=True)
    if "lds" in shapes:
        shape("random deg 10, n = 40000 (LDS kernel's limit)", random_graph(40000, 10, 6, dev), args.reps, lds=True)
    if "c2" in shapes:
        shape("c2 graph (ring + Erdos-Renyi, sym-normalised)", c2_graph(100_000, dev), args.reps)
    if "1m" in shapes:
        shape("random deg 10, n = 1000000", random_graph(1_000_000, 10, 7, dev), args.reps)
    if "c5" in shapes:
        shape("c5-shaped bipartite (3M users x 1M items, hub item)", c5_shaped_graph(3_000_000, 1_000_000, 4, dev),
              max(3, args.reps // 2))
    if "batch" in shapes:
        default = K.POSITION_CODES_ROUNDS_PER_READBACK
        for name, g in (("c2 graph", c2_graph(100_000, dev)), ("random deg 10, n = 1000000", random_graph(1_000_000, 10, 7, dev))):
            describe("read-back batch size, " + name, g)
            anchors = torch.randint(0, g.n, (A,), generator=torch.Generator().manual_seed(2)).to(g.device)

            def eager(batch, g=g, anchors=anchors):
                def run():
                    K.POSITION_CODES_ROUNDS_PER_READBACK = batch
                    try:
                        return K.position_codes_csr(g.rowptr, g.col, g.val, anchors, DIS_Q, method="global")
                    finally:
                        K.POSITION_CODES_ROUNDS_PER_READBACK = default
                return run
            alternate({f"eager, {b:>2} rounds/read-back": eager(b) for b in (4, 8, 16, 32, 64)}, args.reps)


if __name__ == "__main__":
    main()
