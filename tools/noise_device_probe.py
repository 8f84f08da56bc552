#!/usr/bin/env python3
"""Noisy fine-tuning with the noise drawn on the host generator (noise_rng = "host", the reference's draws and the code before
the device source existed) against the device source (noise_rng = "device") on one GPU (profiles/noise_device.txt, DESIGN
section 4.17).

  edge c5|amazon: the edge flavour's noisy fine-tuning step -- cal_loss + backward + Adam.step with use_noise, loss_rows =
                  "batch", edge dropout 0.5 with the mask drawn on the device, 2048 BPR triples -- at c5's model
                  (tools/edge_step_rows_probe.py: 2.2 M users x 1.8 M items, the 4 M x 64 bank, k = 10) or the amazon-like
                  shape of tools/edge_pretrain_probe.py.  The two modes alternate inside one process after both are warm:
                  ROUNDS x ("host", "device"), one event-timed step each; medians and every single time are printed.  Then
                  the host draw alone ([n, 1] torch.randint on the CPU generator + the copy), synchronised.
  node:           the node flavour's noisy step at the node_528 shape of tools/capture_train_probe.py: eager with the host
                  draws, eager with the device source, and the device source replayed from one HIP graph
                  (capture.CapturedTrainStep -- the host mode cannot be captured); blocks of STEPS steps, the variants
                  alternating per round.

Usage:  python tools/noise_device_probe.py edge c5|amazon [--rounds N]
        python tools/noise_device_probe.py node [--steps 200] [--rounds 4]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B = 2048
MODES = ("host", "device")


def edge_model(shape, dev):
    from ragraph_amd.RAGraph_edge import RAGraph

    D, k = 64, 10
    if shape == "c5":
        from ragraph_amd.data import synthetic_bipartite

        U, I = 2_200_000, 1_800_000                  # (tools/bench_blocks.py: config_c5)
        edges, norm, times = synthetic_bipartite(U, I, edges_per_user=10, seed=10, device=dev)

        class DS:
            num_users, num_items = U, I
        DS.edges, DS.edge_norm, DS.edge_times = edges, norm, times
        ds = DS
    else:
        import edge_pretrain_probe as P

        ds = P.build(shape, dev)
        U, I = ds.num_users, ds.num_items

    class Pre:
        def generate(self):
            g = torch.Generator(device=dev).manual_seed(3)
            return 0.1 * torch.randn(U, D, device=dev, generator=g), 0.1 * torch.randn(I, D, device=dev, generator=g)

    m = RAGraph(ds, Pre(), phase="finetune", use_RAG=True, use_noise=True, retrieve_num=k, device=dev)
    g = torch.Generator().manual_seed(76)
    batches = [(torch.randint(0, U, (B,), generator=g), torch.randint(0, I, (B,), generator=g),
                torch.randint(0, I, (B,), generator=g)) for _ in range(4)]
    return m, batches


def run_edge(shape, rounds, dev):
    t0 = time.perf_counter()
    m, batches = edge_model(shape, dev)
    with torch.no_grad():
        m.eval().generate()          # (makes the index and its copies before a step is timed)
    torch.cuda.synchronize()
    n = m.num_users + m.num_items
    print(f"[{shape}] n = {n} nodes, bank {tuple(m.resource_values.shape)}; model built in {time.perf_counter() - t0:.1f} s",
          flush=True)
    m.train()
    m.dropout_rng = "device"
    assert m.loss_rows == "batch" and m.use_noise
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    state = {"i": 0}

    def step(mode):
        m.noise_rng = mode
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

    for mode in MODES * 2:     # warm: code objects, workspaces, the dispatch's statistics
        step(mode)
    ms = {mode: [] for mode in MODES}
    for _ in range(rounds):
        for mode in MODES:
            ms[mode].append(timed(mode))
    for mode in MODES:
        v = ms[mode]
        print(f"step [{mode:6s}] median {statistics.median(v):9.2f} ms   min {min(v):9.2f}  max {max(v):9.2f}   all: "
              + " ".join(f"{x:.2f}" for x in v), flush=True)
    mh, md = statistics.median(ms["host"]), statistics.median(ms["device"])
    spread = max((max(v) - min(v)) / statistics.median(v) for v in ms.values())
    print(f"device / host = {md / mh:.3f} ({mh / md:.2f}x); largest (max - min) / median of a mode: {spread * 100:.1f} %",
          flush=True)
    draws = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.randint(0, m.resource_values.shape[0], (n, m.noise_retrieve_num)).to(dev)
        torch.cuda.synchronize()
        draws.append((time.perf_counter() - t0) * 1e3)
    print(f"host draw alone ([{n}, 1] torch.randint on the CPU generator + copy), synchronised: median "
          f"{statistics.median(draws):.2f} ms   min {min(draws):.2f}  max {max(draws):.2f}", flush=True)


def node_528(dev, noise_rng):
    """tools/capture_train_probe.py's node_528 with noise_finetune."""
    from ragraph_amd.data import DataLoader, synthetic_tu_dataset
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph import RAGraph
    from ragraph_amd.ragraph_utils import process_tu_dataset

    F_in, C, D, N = 18, 3, 256, 20_000
    ds = synthetic_tu_dataset(num_graphs=16, num_node_attributes=F_in, num_node_labels=C, seed=21)
    feats, adj, _ = process_tu_dataset(next(iter(DataLoader(ds, batch_size=16))), F_in, device=dev)
    _ = adj.row_normalized_values()
    gen = torch.Generator(device=dev).manual_seed(74)
    torch.manual_seed(5)
    model = RAGraph(PrePrompt(F_in, D, "prelu", 1, 0.3).to(dev), None, F_in, C, D, finetune=True, noise_finetune=True, device=dev)
    model.toy_graph_base.add_resources(F.normalize(torch.randn(N, D, device=dev, generator=gen), dim=-1),
                                       torch.randn(N, D, device=dev, generator=gen),
                                       F.one_hot(torch.randint(0, C, (N,), device=dev, generator=gen), C).float())
    model.toy_graph_base.noise_rng = noise_rng
    labels = torch.randint(0, C, (feats.shape[0],), device=dev, generator=torch.Generator(device=dev).manual_seed(75))
    model.train()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3, capturable=True)
    return model, (lambda x, y: F.cross_entropy(model(x, adj), y)), opt, (feats, labels)


def run_node(steps, rounds, dev):
    from ragraph_amd.capture import CapturedTrainStep

    def eager_loop(step, opt, ins):
        def run():
            for _ in range(steps):
                opt.zero_grad()
                step(*ins).backward()
                opt.step()
        return run

    def time_block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    variants = {}
    _, step_h, opt_h, ins = node_528(dev, "host")
    variants["eager_host"] = eager_loop(step_h, opt_h, ins)
    _, step_d, opt_d, _ = node_528(dev, "device")
    variants["eager_device"] = eager_loop(step_d, opt_d, ins)
    _, step_c, opt_c, _ = node_528(dev, "device")
    cap = CapturedTrainStep(step_c, opt_c, *ins)

    def replay():
        for _ in range(steps):
            cap(*ins)
    variants["replay_device"] = replay
    for fn in variants.values():   # warm every variant once
        fn()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(time_block(fn))
    med = {k: round(statistics.median(v), 4) for k, v in times.items()}
    print(json.dumps({"shape": "node_528 noisy", "steps_per_round": steps, "rounds": rounds, "ms_per_step": med,
                      "all_rounds": {k: [round(x, 4) for x in v] for k, v in times.items()},
                      "eager_device_over_eager_host": round(med["eager_device"] / med["eager_host"], 3),
                      "replay_device_over_eager_host": round(med["replay_device"] / med["eager_host"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("edge", "node"))
    ap.add_argument("shape", nargs="?", default="c5", choices=("amazon", "c5"))
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}; {a.what}" + (f" {a.shape}, B = {B}" if a.what == "edge" else ""), flush=True)
    if a.what == "edge":
        run_edge(a.shape, a.rounds or 9, dev)
    else:
        run_node(a.steps, a.rounds or 4, dev)


if __name__ == "__main__":
    main()
