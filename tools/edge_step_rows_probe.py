#!/usr/bin/env python3
"""The edge flavour's training step with the loss computed at the batch's rows ("batch", RAGraph.forward_rows) against the
whole forward ("all", the code before forward_rows existed) on one GPU (profiles/edge_step_rows.txt).

  finetune: c5's fine-tuning model (tools/bench_blocks.py: config_c5 -- 2.2 M users x 1.8 M items, 44 M directed edges, the
            4 M x 64 bank, k = 10), the step bench_blocks.finetune_edge times: cal_loss + backward + Adam.step, edge dropout
            0.5 with the mask drawn on the device, 2048 BPR triples.
  pretrain: the pre-training step of tools/edge_pretrain_probe.py (phase "pretrain": no gate, no bank, nothing retrieved) at
            its amazon-like or c5 shape, the same two modes.

The two modes alternate inside one process after both are warm: ROUNDS x ("all", "batch"), one event-timed step each; the
medians and every single time are printed, so the spread of the box is on the page.  Then the split of one step per mode,
every phase synchronised (the sum exceeds the unsynchronised step): graph rebuild (COO -> CSR), time softmax, propagation
layers, retrieval (top-k + gather_reduce), the rest of cal_loss, backward, Adam.  Finally the loss of both modes on one
mask and batch (equal as floats) and the largest gradient difference.

Usage:  python tools/edge_step_rows_probe.py finetune [--rounds N]
        python tools/edge_step_rows_probe.py pretrain amazon|c5 [--rounds N]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragraph_amd import autograd as A  # noqa: E402
from ragraph_amd import kernels as K  # noqa: E402

B = 2048
MODES = ("all", "batch")


def c5_finetune_model(dev):
    from ragraph_amd.data import synthetic_bipartite
    from ragraph_amd.RAGraph_edge import RAGraph

    U, I, D, k = 2_200_000, 1_800_000, 64, 10       # (tools/bench_blocks.py: config_c5)
    edges, norm, times = synthetic_bipartite(U, I, edges_per_user=10, seed=10, device=dev)

    class DS:
        num_users, num_items = U, I
    DS.edges, DS.edge_norm, DS.edge_times = edges, norm, times

    class Pre:
        def generate(self):
            g = torch.Generator(device=dev).manual_seed(3)
            return 0.1 * torch.randn(U, D, device=dev, generator=g), 0.1 * torch.randn(I, D, device=dev, generator=g)

    m = RAGraph(DS, Pre(), phase="finetune", use_RAG=True, retrieve_num=k, device=dev)
    g = torch.Generator().manual_seed(76)
    batches = [(torch.randint(0, U, (B,), generator=g), torch.randint(0, I, (B,), generator=g),
                torch.randint(0, I, (B,), generator=g)) for _ in range(4)]
    return m, batches


def pretrain_model(shape, dev):
    import edge_pretrain_probe as P
    from ragraph_amd.RAGraph_edge import RAGraph

    ds = P.build(shape, dev)
    torch.manual_seed(2023)
    m = RAGraph(ds, None, phase="pretrain", device=dev)
    ds.shuffle()
    return m, [ds.get_train_batch(s * B, (s + 1) * B) for s in range(4)]


class Split:
    """Synchronised wall-clock per phase of a forward, through wrappers around the library calls the step makes."""

    def __init__(self, model):
        self.on, self.ms, self.undo = False, {}, []
        for owner, name, key in ((K, "coo_to_csr", "coo_to_csr"), (K, "time_rescale", "softmax"), (K, "segment_softmax", "softmax"),
                                 (A, "spmm_csr", "layers"), (A, "spmm_csr_rows", "layers"), (K, "gather_reduce", "retrieval")):
            self.wrap(owner, name, key)
        if model._index is not None:
            self.wrap(model._index, "topk", "retrieval")

    def wrap(self, owner, name, key):
        real = getattr(owner, name)

        def timed(*a, **kw):
            if not self.on:
                return real(*a, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = real(*a, **kw)
            torch.cuda.synchronize()
            self.ms[key] = self.ms.get(key, 0.0) + (time.perf_counter() - t0) * 1e3
            return out
        setattr(owner, name, timed)
        self.undo.append((owner, name, real))

    def close(self):
        for owner, name, real in self.undo:
            setattr(owner, name, real)


def run(m, batches, rounds):
    m.train()
    m.dropout_rng = "device"
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    state = {"i": 0}

    def step(mode):
        m.loss_rows = mode
        state["i"] += 1
        opt.zero_grad()
        loss, _ = m.cal_loss(batches[state["i"] % len(batches)])
        loss.backward()
        opt.step()

    def timed(mode):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        step(mode)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for mode in MODES * 2:     # warm: code objects, workspaces, the index's copies, the dispatch's statistics
        step(mode)
    ms = {mode: [] for mode in MODES}
    for _ in range(rounds):
        for mode in MODES:
            ms[mode].append(timed(mode))
    for mode in MODES:
        v = ms[mode]
        print(f"step [{mode:5s}] median {statistics.median(v):9.2f} ms   min {min(v):9.2f}  max {max(v):9.2f}   all: "
              + " ".join(f"{x:.2f}" for x in v), flush=True)
    ma, mb = statistics.median(ms["all"]), statistics.median(ms["batch"])
    spread = max((max(v) - min(v)) / statistics.median(v) for v in ms.values())
    print(f"batch / all = {mb / ma:.3f} ({ma / mb:.2f}x); largest (max - min) / median of a mode: {spread * 100:.1f} %", flush=True)

    sp = Split(m)
    try:
        for mode in MODES:
            m.loss_rows = mode
            acc = {}
            for _ in range(2):
                sp.ms = {}
                opt.zero_grad()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sp.on = True
                loss, _ = m.cal_loss(batches[0])
                sp.on = False
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                loss.backward()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                opt.step()
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                parts = dict(sp.ms)
                parts["cal_loss other"] = (t1 - t0) * 1e3 - sum(sp.ms.values())
                parts["backward"], parts["adam"] = (t2 - t1) * 1e3, (t3 - t2) * 1e3
                for k, v in parts.items():
                    acc[k] = acc.get(k, 0.0) + v / 2
            print(f"split [{mode:5s}] ms, synchronised: " + ", ".join(f"{k} {v:.2f}" for k, v in acc.items())
                  + f"; sum {sum(acc.values()):.2f}", flush=True)
    finally:
        sp.close()

    # the same mask and batch through both modes
    out = {}
    m.dropout_rng = "host"
    for mode in MODES:
        m.loss_rows = mode
        m.zero_grad(set_to_none=True)
        torch.manual_seed(8)
        loss, _ = m.cal_loss(batches[1])
        loss.backward()
        out[mode] = (float(loss), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    worst = max(float((out["batch"][1][k] - g).abs().max()) / max(1.0, float(g.abs().max())) for k, g in out["all"][1].items())
    print(f"same mask: loss all {out['all'][0]!r} batch {out['batch'][0]!r} equal {out['all'][0] == out['batch'][0]}; "
          f"largest gradient difference / max(1, |ref|max): {worst:.3e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("finetune", "pretrain"))
    ap.add_argument("shape", nargs="?", default="c5", choices=("amazon", "c5"))
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; {a.what} {a.shape}, B = {B}, device mask, {a.rounds} alternating rounds",
          flush=True)
    t0 = time.perf_counter()
    if a.what == "finetune":
        m, batches = c5_finetune_model(dev)
        with torch.no_grad():
            m.eval().generate()          # (makes the index and its copies, as bench_blocks does before it times a step)
    else:
        m, batches = pretrain_model(a.shape, dev)
    torch.cuda.synchronize()
    print(f"model built in {time.perf_counter() - t0:.1f} s", flush=True)
    run(m, batches, a.rounds)


if __name__ == "__main__":
    main()
