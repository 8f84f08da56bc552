#!/usr/bin/env python3
"""The reference's RAGraph_edge/pretrain.py --phase pretrain (with utils/trainer.py Trainer.train) on ragraph_amd:

    data  = EdgeListData(pretrain.txt, pretrain_val.txt)                             # pretrain.py:66
    model = RAGraph(data, phase='pretrain')                                          # :68 (xavier tables, no gate, no bank)
    for epoch: data.shuffle()                                                        # trainer.py:22
               while s + batch_size <= num_edges:                                    # :33
                   loss = model.cal_loss(data.get_train_batch(s, s + batch_size))    # :35-38
                   loss.backward(); Adam(lr=1e-3).step()                             # :39-40
               Metric('recall;ndcg', '20').eval(model, data)                         # :101-102 (the validation file)
               save the state dict on a new best recall, stop after 10 epochs without one   # :103-122

The negatives of every batch come from the device sampler (kernels.edge_neg_sample); the edge-dropout mask is the
reference's CPU draw by default (--dropout_rng device: torch.rand on the device).  Runs on a synthetic planted-community
dataset unless --data_path names a directory with pretrain.txt and pretrain_val.txt (the reference's layout).  The saved
checkpoint loads strictly into RAGraph(..., phase="for_tune"), the pretrained_model of phase="finetune".

Usage: python examples/pretrain_edge.py [--epochs 300] [--data_path DIR] [--out saved/edge_pretrain.pt]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragraph_amd.edge_data import EdgeListData  # noqa: E402
from ragraph_amd.edge_eval import Metric  # noqa: E402
from ragraph_amd.RAGraph_edge import RAGraph  # noqa: E402


def synthetic_files(directory, num_users=3000, num_items=2000, communities=20, per_user=24, n_val=5, noise=0.1, seed=0):
    """pretrain.txt / pretrain_val.txt in the reference's format: users of a community interact mostly with its items, the
    popular ones (Zipf within the community) more often; the validation file holds n_val unseen items of the user's
    community, drawn by the same popularity."""
    rng = np.random.default_rng(seed)
    uc, ic = rng.integers(0, communities, num_users), np.arange(num_items) % communities
    pools = [np.flatnonzero(ic == c) for c in range(communities)]
    train, val = [], []
    for u in range(num_users):
        pool = pools[uc[u]]
        pop = 1.0 / np.arange(1, len(pool) + 1)
        its = rng.choice(pool, size=per_user + n_val, replace=False, p=pop / pop.sum())
        tr = its[:per_user].copy()
        nz = rng.random(per_user) < noise
        tr[nz] = rng.integers(0, num_items, int(nz.sum()))
        times = 1_700_000_000 + rng.integers(0, 7 * 24 * 3600, per_user)
        train.append(f"{u}\t{' '.join(map(str, tr))}\t{' '.join(map(str, times))}")
        val.append(f"{u}\t{' '.join(map(str, its[per_user:]))}")
    paths = os.path.join(directory, "pretrain.txt"), os.path.join(directory, "pretrain_val.txt")
    for p, lines in zip(paths, (train, val)):
        with open(p, "w") as f:
            f.write("\n".join(lines) + "\n")
    return paths


def train(model, data, epochs, batch_size=2048, lr=1e-3, patience=10, save_path=None, log=print):
    """Trainer.train (utils/trainer.py:20-122).  Returns the best recall@20 and its state dict."""
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    metric = Metric("recall;ndcg", "20")
    best, best_state, wait = 0.0, None, 0
    model.eval()
    r0 = metric.eval(model, data)
    log(f"epoch -1: recall@20 {r0['recall'][0]:.4f} ndcg@20 {r0['ndcg'][0]:.4f} (initial tables)")
    for epoch in range(epochs):
        t0 = time.time()
        data.shuffle()
        model.train()
        s, losses = 0, []
        while s + batch_size <= data.num_edges:
            opt.zero_grad()
            loss, _ = model.cal_loss(data.get_train_batch(s, s + batch_size))
            loss.backward()
            opt.step()
            losses.append(loss.detach())
            s += batch_size
        ep_loss = float(torch.stack(losses).mean()) if losses else float("nan")
        t_train = time.time() - t0
        model.eval()
        res = metric.eval(model, data)
        rec = float(res["recall"][0])
        log(f"epoch {epoch}: loss {ep_loss:.5f} ({len(losses)} steps, {t_train:.2f} s) recall@20 {rec:.4f} "
            f"ndcg@20 {res['ndcg'][0]:.4f}")
        if rec > best:
            best, wait = rec, 0
            best_state = {k: v.detach().clone() for k, v in model.state_dict().items()}
            if save_path:
                torch.save(best_state, save_path)
        else:
            wait += 1
            if wait >= patience:
                log(f"early stop: best recall@20 {best:.4f}")
                break
    return best, best_state


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data_path", default=None, help="directory with pretrain.txt and pretrain_val.txt (default: synthetic)")
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--batch_size", type=int, default=2048)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=2023)
    ap.add_argument("--dropout_rng", choices=("host", "device"), default="host")
    ap.add_argument("--out", default="saved/edge_pretrain.pt")
    a = ap.parse_args()
    torch.manual_seed(a.seed)
    np.random.seed(a.seed)
    dev = torch.device("cuda")
    with tempfile.TemporaryDirectory() as tmp:
        tr, va = ((os.path.join(a.data_path, "pretrain.txt"), os.path.join(a.data_path, "pretrain_val.txt"))
                  if a.data_path else synthetic_files(tmp))
        data = EdgeListData(tr, va, device=dev)
    print(f"{data.num_users} users x {data.num_items} items, {data.num_edges} interactions")
    model = RAGraph(data, None, phase="pretrain", device=dev)
    model.dropout_rng = a.dropout_rng
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    best, state = train(model, data, a.epochs, a.batch_size, a.lr, save_path=a.out)
    if state is None:                       # (no epoch beat recall 0: keep the last tables)
        torch.save(model.state_dict(), a.out)
    ft = RAGraph(data, None, phase="for_tune", device=dev)
    ft.load_state_dict(torch.load(a.out), strict=True)
    print(f"best recall@20 {best:.4f}; checkpoint {a.out} loads strictly into phase='for_tune'")


if __name__ == "__main__":
    main()
