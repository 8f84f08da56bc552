#!/usr/bin/env python3
"""Edge-flavour pre-training costs on one GPU (profiles/edge_pretrain.txt).

  sampler: kernels.edge_neg_sample per call (HIP events, warm, no read-back) at B = 2048 / 4096 and n_negs = 1 / 16,
           against the reference's negative_sampling loop (RAGraph_edge/utils/dataloader.py:142-152) restated below and run
           on the host (one Python thread) over the same histories.
  step:    one pre-training step -- get_train_batch + cal_loss + backward + Adam(lr=1e-3) -- with the edge-dropout mask drawn
           on the host (the reference's torch.rand) or on the device: ms per step over a run of steps (events), the split of
           a step (each phase synchronised), and an epoch (--epoch: every batch of a shuffled epoch, timed).

Shapes: amazon-like (131 707 users x 107 028 items, as the reference's amazon split; its pretrain.txt is not shipped, so the
interactions are synthetic: 1 + Poisson(8.1) per user, Zipf-like item popularity) and c5 (2.2 M users x 1.8 M items, 10
interactions per user before de-duplication: 44 M directed edges).

Usage:  python tools/edge_pretrain_probe.py sampler [amazon|c5]
        python tools/edge_pretrain_probe.py step amazon|c5 host|device [--steps N] [--epoch]
        python tools/edge_pretrain_probe.py step amazon device --only N    (N plain steps after one warm step: for
            rocprofv3 --kernel-trace --stats; two runs with different N give the launches of one step)
"""
from __future__ import annotations

import argparse
import os
import platform
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragraph_amd import kernels as K  # noqa: E402
from ragraph_amd.edge_data import EdgeListData  # noqa: E402
from ragraph_amd.RAGraph_edge import RAGraph  # noqa: E402

SHAPES = {"amazon": (131_707, 107_028), "c5": (2_200_000, 1_800_000)}


def interactions(shape, seed=10):
    U, I = SHAPES[shape]
    rng = np.random.default_rng(seed)
    per = 1 + rng.poisson(8.1, U) if shape == "amazon" else np.full(U, 10)
    u = np.repeat(np.arange(U, dtype=np.int64), per)
    i = np.minimum((rng.pareto(1.1, len(u)) * I / 50).astype(np.int64), I - 1)
    if shape == "c5":                      # as data.synthetic_bipartite: (user, item) pairs de-duplicated
        key = np.unique(u * I + i)
        u, i = key // I, key % I
    t = 1_700_000_000 + rng.integers(0, 720 * 3600, len(u))
    return u, i, t, U, I


def build(shape, dev):
    t0 = time.perf_counter()
    u, i, t, U, I = interactions(shape)
    ds = EdgeListData.from_interactions(u, i, t, num_users=U, num_items=I, device=dev)
    torch.cuda.synchronize()
    print(f"[{shape}] {U} users x {I} items, {ds.num_edges} interactions, {ds.edges.shape[0]} directed edges, history "
          f"{ds.hist_items.numel()} items; built in {time.perf_counter() - t0:.1f} s", flush=True)
    return ds


def ref_negative_sampling(user_item, train_user_set, num_items, n=1):
    """dataloader.py:142-152, as the reference runs it (np.random.randint until the item is not in the user's list)."""
    neg_items = []
    for user, _ in user_item:
        user = int(user)
        for _ in range(n):
            while True:
                neg_item = np.random.randint(low=0, high=num_items, size=1)[0]
                if neg_item not in train_user_set[user]:
                    break
            neg_items.append(neg_item)
    return neg_items


def event_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def sampler(shape, dev):
    ds = build(shape, dev)
    edgelist = ds.edgelist.cpu().numpy().astype(np.int32)      # the reference keeps it as int32 numpy
    print(f"host: {cpu_name()}, os.cpu_count() = {os.cpu_count()}, the loop on one Python thread "
          f"(sched_getaffinity: {len(os.sched_getaffinity(0))} CPUs)", flush=True)
    torch.manual_seed(0)
    ds.shuffle()
    np.random.seed(0)
    for B in (2048, 4096):
        users = ds.edgelist[:B, 0].contiguous()
        seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=dev)
        for n in (1, 16):
            ms = event_ms(lambda: K.edge_neg_sample(ds.hist_rowptr, ds.hist_items, ds.num_items, users, n, seed,
                                                    check_users=False), 200)
            ui = edgelist[:B]
            reps = 5 if n == 1 else 2
            ref_negative_sampling(ui, ds.train_user_dict, ds.num_items, n)
            t0 = time.perf_counter()
            for _ in range(reps):
                ref_negative_sampling(ui, ds.train_user_dict, ds.num_items, n)
            host = (time.perf_counter() - t0) / reps * 1e3
            batch_ms = event_ms(lambda: ds.get_train_batch(0, B, n_negs=n), 200)
            print(f"[{shape}] sampler B={B} n_negs={n}: device {ms * 1e3:.1f} us/call (get_train_batch {batch_ms * 1e3:.1f} us); "
                  f"reference loop on the host {host:.2f} ms/call ({host / ms:.0f}x)", flush=True)


def step_probe(shape, rng, dev, steps, epoch, only=0):
    ds = build(shape, dev)
    torch.manual_seed(2023)
    t0 = time.perf_counter()
    m = RAGraph(ds, None, phase="pretrain", device=dev).train()
    m.dropout_rng = rng
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    torch.cuda.synchronize()
    print(f"[{shape}] pretrain model built in {time.perf_counter() - t0:.1f} s; dropout mask on the {rng}", flush=True)
    B = 2048
    per_epoch = ds.num_edges // B
    ds.shuffle()
    state = {"s": 0}

    def one():
        s = state["s"]
        if s + B > ds.num_edges:
            s = 0
        state["s"] = s + B
        opt.zero_grad()
        loss, _ = m.cal_loss(ds.get_train_batch(s, s + B))
        loss.backward()
        opt.step()

    if only:
        one()
        torch.cuda.synchronize()
        for _ in range(only):
            one()
        torch.cuda.synchronize()
        print(f"[{shape}] {only} steps after one warm step", flush=True)
        return
    ms = event_ms(one, steps, warm=2)
    # the split: every phase synchronised
    split = {"get_train_batch": 0.0, "cal_loss": 0.0, "backward": 0.0, "adam": 0.0}
    for _ in range(steps):
        s = state["s"] if state["s"] + B <= ds.num_edges else 0
        state["s"] = s + B
        torch.cuda.synchronize()
        t = time.perf_counter()
        batch = ds.get_train_batch(s, s + B)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        opt.zero_grad()
        loss, _ = m.cal_loss(batch)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        loss.backward()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        opt.step()
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        for k, v in zip(split, (t1 - t, t2 - t1, t3 - t2, t4 - t3)):
            split[k] += v * 1e3 / steps
    mask_ms = event_ms(m.draw_edge_mask, steps, warm=1)
    parts = ", ".join(f"{k} {v:.2f}" for k, v in split.items())
    print(f"[{shape}] step ({rng} mask): {ms:.2f} ms/step over {steps} steps; split (synchronised) ms: {parts}, of which "
          f"the mask draw alone {mask_ms:.2f}; {per_epoch} steps per epoch of {ds.num_edges} interactions", flush=True)
    if epoch:
        ds.shuffle()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = 0
        while s + B <= ds.num_edges:
            opt.zero_grad()
            loss, _ = m.cal_loss(ds.get_train_batch(s, s + B))
            loss.backward()
            opt.step()
            s += B
            if (s // B) % 2000 == 0:
                print(f"  {s // B} steps, {time.perf_counter() - t0:.1f} s", flush=True)
        torch.cuda.synchronize()
        print(f"[{shape}] one epoch ({rng} mask, shuffle + {per_epoch} steps): {time.perf_counter() - t0:.2f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("sampler", "step"))
    ap.add_argument("shape", nargs="?", default="amazon", choices=tuple(SHAPES))
    ap.add_argument("rng", nargs="?", default="host", choices=("host", "device"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--epoch", action="store_true")
    ap.add_argument("--only", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}", flush=True)
    if a.what == "sampler":
        sampler(a.shape, dev)
    else:
        step_probe(a.shape, a.rng, dev, a.steps, a.epoch, a.only)


if __name__ == "__main__":
    main()
