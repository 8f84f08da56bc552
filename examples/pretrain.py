#!/usr/bin/env python3
"""The reference's RAGraph_node/pretrain.py:64-170 (link-prediction pre-training) on ragraph_amd, on synthetic TU-shaped
data (the reference ships no dataset and no weights, .MISSING_LARGE_BLOBS).  The loop is the reference's, step for step:

    model = PrePrompt(F, 256, 'prelu', 1, 0.3)                                       # pretrain.py:64
    for epoch: seed_everything(seed)                                                 # :69 (same batches every epoch)
               loss = 0
               for step, batch: features, adj = process_tu(batch)                    # :73
                                sample = prompt_pretrain_sample(adj, 100)            # :75
                                optimiser = Adam(model.parameters(), lr=0.001)       # :123 (a new one per batch)
                                loss = loss + model(features, ..., sample=sample)    # :142-148
               loss = loss / step                                                    # :152 (the last step INDEX)
               save the state dict when the loss is a new best, else count; stop at patience 10   # :154-163
               loss.backward(); optimiser.step()                                     # :164-165 (one step per epoch)

Differences: A_hat comes from process_tu_dataset (CSR with self loops; the sampler ignores the diagonal, so it draws from
A as the reference's does), the sample is drawn on the device, and the augmented inputs of DGI / GraphCL -- whose losses
the reference never computes -- are not built.  A single batch divides by 1 instead of 0.

Usage: python examples/pretrain.py [--epochs 1000] [--graphs 120] [--out modelset/model_SYNTH.pkl]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragraph_amd.data import DataLoader, synthetic_tu_dataset  # noqa: E402
from ragraph_amd.preprompt import PrePrompt, prompt_pretrain_sample  # noqa: E402
from ragraph_amd.ragraph_utils import process_tu_dataset, seed_everything  # noqa: E402

PATIENCE = 10      # pretrain.py:47
LR = 0.001         # :48
N_NEG = 100        # :75 (RAGraph_graph/pretrain.py:86: 50)


def pretrain(model, dataset, num_node_attributes, epochs, batch_size=16, seed=39, n_neg=N_NEG, patience=PATIENCE, lr=LR,
             save_path=None, device="cuda", log=print):
    """The reference's epoch loop (see the module docstring).  Returns (the loss of every epoch run, the best state dict)."""
    best, cnt_wait, best_state, history = float("inf"), 0, None, []
    for epoch in range(epochs):
        seed_everything(seed)
        loss, optimiser, step = 0, None, 0
        batches = list(DataLoader(dataset, batch_size=batch_size, shuffle=True))
        if len(dataset) % batch_size and len(batches) > 1:
            batches = batches[:-1]                                      # drop_last=True (:60)
        for step, batch in enumerate(batches):
            features, adj, _ = process_tu_dataset(batch, num_node_attributes, device=device)
            sample = prompt_pretrain_sample(adj, n_neg)
            optimiser = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0)
            model.train()
            optimiser.zero_grad()
            logit = model(features, None, None, None, adj, None, None, False, None, None, None, lbl=None, sample=sample)
            loss = loss + logit
        loss = loss / max(step, 1)
        value = float(loss.detach())
        history.append(value)
        log(f"epoch {epoch}: Loss:[{value:.4f}]")
        if value < best:
            best, cnt_wait = value, 0
            best_state = {k: v.detach().clone() for k, v in model.state_dict().items()}
            if save_path:
                torch.save(best_state, save_path)
        else:
            cnt_wait += 1
        if cnt_wait == patience:
            log("Early stopping!")
            break
        loss.backward()
        optimiser.step()
    return history, best_state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=1000)
    ap.add_argument("--graphs", type=int, default=120)
    ap.add_argument("--seed", type=int, default=39)
    ap.add_argument("--out", default="modelset/model_SYNTH.pkl")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    seed_everything(args.seed)
    F_attr, C = 18, 3  # ENZYMES-shaped: 18 node attributes + 3 one-hot node labels
    dataset = synthetic_tu_dataset(num_graphs=args.graphs, num_node_attributes=F_attr, num_node_labels=C, seed=9,
                                   name="ENZYMES")
    model = PrePrompt(F_attr, 256, "prelu", 1, 0.3).to(dev)
    if os.path.dirname(args.out):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    t0 = time.perf_counter()
    history, _ = pretrain(model, dataset, F_attr, args.epochs, seed=args.seed, save_path=args.out, device=dev)
    torch.cuda.synchronize()
    print(f"{len(history)} epochs in {time.perf_counter() - t0:.2f} s; best loss {min(history):.4f}; wrote {args.out}")


if __name__ == "__main__":
    main()
