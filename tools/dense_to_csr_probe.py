"""What the device dense -> CSR conversion costs and saves (profiles/dense_to_csr.txt is this tool's output).

  1. CSRGraph.from_dense on a device tensor against the torch chain it replaced (nonzero, bincount, cumsum, a fancy-index
     gather, and the has_long_rows read-back the forward then makes), restated here: same process, alternating rounds,
     medians of host-clock times that end in a device synchronise.  Three shapes: a 40-node graph, the Cora-shaped 2708^2
     with ~13 k entries, 4096^2 at 1 % density.
  2. The eager c1-shaped forward (tools/bench_blocks.py config_c1) called with a DENSE adjacency: with the torch chain
     patched in for from_dense against the library's -- the share of the step the conversion is.
  3. The captured replay with the dense adjacency as an INPUT (converted on the device at every replay) against the captured
     replay with a closed-over CSRGraph, c1-shaped and at 40 nodes: the price of converting per replay.

    python tools/dense_to_csr_probe.py [--out FILE] [--rounds 7]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ragraph_amd import kernels as K  # noqa: E402
from ragraph_amd.capture import CapturedForward  # noqa: E402
from ragraph_amd.graph import CSRGraph  # noqa: E402


def torch_from_dense(adj, capacity=None):
    """CSRGraph.from_dense before the library's conversion (torch ops on the device)."""
    a = adj.squeeze(0) if adj.dim() == 3 else adj
    n = a.shape[0]
    nz = torch.nonzero(a, as_tuple=False)
    rows, cols = nz[:, 0], nz[:, 1]
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=a.device)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return CSRGraph(rowptr, cols.to(torch.int32), a[rows, cols].float().contiguous(), n)


def host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def alternate(fns, reps, rounds):
    """Median over `rounds` of the mean ms per call, the candidates taking turns inside every round."""
    for f in fns.values():
        for _ in range(3):
            f()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            times[k].append(host_ms(f, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def dense_adjacency(n, nnz_target, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    a = (torch.rand(n, n, device=dev, generator=g) < nnz_target / (n * n)).float()
    a = ((a + a.t() + torch.eye(n, device=dev)) > 0).float()
    d = a.sum(1).rsqrt()
    return (a * d[:, None] * d[None, :]).contiguous()


def node_model(n, F, D, C, N, k, dev, bag_of_words):
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph import RAGraph

    g = torch.Generator(device=dev).manual_seed(70)
    if bag_of_words:
        X = (torch.rand(n, F, device=dev, generator=g) < 0.0127).float()
        X = X / X.sum(1, keepdim=True).clamp_min(1)
    else:
        X = torch.randn(n, F, device=dev, generator=g)
    m = RAGraph(PrePrompt(F, D, "prelu", 1, 0.3).to(dev), None, F, C, D, device=dev).eval()
    m.toy_graph_base.retrieve_num = k
    m.toy_graph_base.add_resources(torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=g), dim=-1),
                                   torch.randn(N, D, device=dev, generator=g),
                                   torch.nn.functional.one_hot(torch.randint(0, C, (N,), device=dev, generator=g), C).float())
    _ = m.toy_graph_base.keys_normalized
    return m, X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_to_csr_probe: no ROCm device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda t: f"{t[0]:8.4f} ms (min {t[1]:.4f}, max {t[2]:.4f})"
    say(f"# tools/dense_to_csr_probe.py --rounds {args.rounds}: medians over the rounds of the mean ms per call; the candidates")
    say("# alternate inside every round; host clock around calls that end in a device synchronise")
    say()
    say("## 1. CSRGraph.from_dense on a device tensor: the torch chain it replaced / the library's conversion")
    for name, n, nnz, reps in (("40 nodes", 40, 150, 200), ("Cora-shaped 2708^2", 2708, 13000, 100), ("4096^2 at 1 %", 4096, 168000, 50)):
        a = dense_adjacency(n, nnz / 2, dev, n)

        def old():
            g = torch_from_dense(a)
            return g.has_long_rows          # (the forward's second read-back; the new graph knows it at construction)

        def new():
            g = CSRGraph.from_dense(a)
            return g.has_long_rows

        def new_padded():
            g = CSRGraph.from_dense(a, capacity=n * n)
            return g.has_long_rows

        g0, g1 = torch_from_dense(a), CSRGraph.from_dense(a)
        assert torch.equal(g0.rowptr, g1.rowptr) and torch.equal(g0.col, g1.col) and torch.equal(g0.val, g1.val)
        r = alternate({"torch": old, "library": new, "padded": new_padded}, reps, args.rounds)
        say(f"{name:>20} ({g1.nnz} entries): torch chain {fmt(r['torch'])}")
        say(f"{'':>20}  library, eager form (one read-back) {fmt(r['library'])}   x{r['torch'][0] / r['library'][0]:.2f}")
        say(f"{'':>20}  library, capacity n*n (no read-back; enqueue + sync) {fmt(r['padded'])}")
    say()
    say("## 2. eager c1-shaped forward (2708 nodes, F = 1433 bag-of-words, 10k x 128 bank, k = 5) called with a DENSE adjacency")
    n = 2708
    adj = dense_adjacency(n, 5000, dev, 7)
    m, X = node_model(n, 1433, 128, 7, 10_000, 5, dev, True)
    g_fixed = CSRGraph.from_dense(adj)
    _ = g_fixed.row_normalized_values()
    library = CSRGraph.__dict__["from_dense"]

    def with_torch():
        CSRGraph.from_dense = staticmethod(torch_from_dense)
        try:
            return m(X, adj)
        finally:
            CSRGraph.from_dense = library

    with torch.no_grad():
        assert torch.equal(with_torch(), m(X, adj))
        r = alternate({"torch": with_torch, "library": lambda: m(X, adj), "csr": lambda: m(X, g_fixed)}, 50, args.rounds)
    say(f"from_dense = torch chain : {fmt(r['torch'])}")
    say(f"from_dense = library     : {fmt(r['library'])}")
    say(f"a CSRGraph made once     : {fmt(r['csr'])}   (row normalisation cached on the graph too)")
    say(f"the conversion's share of the dense-adjacency step: torch chain {100 * (r['torch'][0] - r['csr'][0]) / r['torch'][0]:.0f} %, "
        f"library {100 * (r['library'][0] - r['csr'][0]) / r['library'][0]:.0f} % (both include the row normalisation a fresh graph repeats)")
    say()
    say("## 3. captured replay: dense adjacency as an INPUT (converted at every replay) / a closed-over CSRGraph")
    for name, mm, XX, aa in (("c1-shaped, 2708 nodes", m, X, adj),) + tuple(
            (f"{nn} nodes, F = 32, 256 x 256 bank", *node_model(nn, 32, 256, 3, 256, 5, dev, False), dense_adjacency(nn, 3 * nn, dev, 11))
            for nn in (40,)):
        gg = CSRGraph.from_dense(aa)
        _ = gg.row_normalized_values()
        f_dense = CapturedForward(lambda x, a: mm(x, a), XX, aa)
        f_csr = CapturedForward(lambda x: mm(x, gg), XX)
        with torch.no_grad():
            want = mm(XX, gg)
        assert torch.equal(f_dense(XX, aa), want) and torch.equal(f_csr(XX), want)
        # (inputs at the static addresses: no copy, the replay alone)
        xs, as_ = f_dense.static_inputs
        r = alternate({"dense": lambda: f_dense(xs, as_), "csr": lambda: f_csr(f_csr.static_inputs[0])}, 200, args.rounds)
        say(f"{name}: dense input {fmt(r['dense'])}")
        say(f"{'':>{len(name)}}  closed-over CSRGraph {fmt(r['csr'])}   difference {r['dense'][0] - r['csr'][0]:+.4f} ms per replay")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
