#!/usr/bin/env python3
"""The reference's RAGraph_edge/finetune_rag.py on ragraph_amd: staged fine-tuning with the interpolative update.

    pre-train  RAGraph(phase="pretrain") on pretrain.txt / pretrain_val.txt (edge_train.Trainer.train), keep the best tables
    stage s    start from the pre-trained tables or, once --updt-inter stages are saved, from their interpolative update with
               the newest saved models (edge_train.interpolative_update: one kernel call per table); propagate over the
               merge of every file seen so far; fine-tune on file s of [fine_tune, test_1, ...]; test on test_s with every
               earlier file masked out of the ranking (edge_train.run_stages)

Writes a small synthetic dataset in the reference's layout (one line per user: user TAB items TAB unix times; planted
communities, a user's later files hold further items of its community, about a third of the users miss from each later
file) unless --data_path names a directory with pretrain.txt, pretrain_val.txt, fine_tune.txt, test_1.txt, ...

Usage: python examples/finetune_edge.py [--stages 3] [--updt-inter 1] [--lora] [--noise] [--dropout-rng device]
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
from ragraph_amd.edge_train import Trainer, run_stages  # noqa: E402
from ragraph_amd.RAGraph_edge import RAGraph  # noqa: E402


def synthetic_files(directory, stages, num_users=1500, num_items=1000, communities=20, seed=0):
    """pretrain (12 items per user), pretrain_val (3), then fine_tune and test_1..test_stages (4 each, a third of the users
    absent), every file a day later than the one before."""
    rng = np.random.default_rng(seed)
    uc, ic = rng.integers(0, communities, num_users), np.arange(num_items) % communities
    pools = [np.flatnonzero(ic == c) for c in range(communities)]
    names = ["pretrain", "pretrain_val", "fine_tune"] + [f"test_{s}" for s in range(1, stages + 1)]
    sizes = [12, 3] + [4] * (stages + 1)
    lines = {n: [] for n in names}
    for u in range(num_users):
        pool = pools[uc[u]]
        pop = 1.0 / np.arange(1, len(pool) + 1)
        its = rng.choice(pool, size=sum(sizes), replace=False, p=pop / pop.sum())
        off = 0
        for day, (n, k) in enumerate(zip(names, sizes)):
            mine, off = its[off:off + k], off + k
            if day >= 2 and rng.random() < 1 / 3:
                continue
            if n == "pretrain_val":
                lines[n].append(f"{u}\t{' '.join(map(str, mine))}")
            else:
                times = 1_700_000_000 + day * 86400 + rng.integers(0, 86400, k)
                lines[n].append(f"{u}\t{' '.join(map(str, mine))}\t{' '.join(map(str, times))}")
    for n in names:
        with open(os.path.join(directory, n + ".txt"), "w") as f:
            f.write("\n".join(lines[n]) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data_path", default=None)
    ap.add_argument("--stages", type=int, default=3, help="test files test_1 .. test_N (synthetic data: how many to write)")
    ap.add_argument("--updt-inter", type=int, default=1, help="saved stages mixed into the next start (finetune_rag.py --updt_inter)")
    ap.add_argument("--pretrain-epochs", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=5, help="fine-tuning epochs per stage at most")
    ap.add_argument("--batch-size", type=int, default=2048)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--lora", action="store_true", help="use_LoRA: train rank-16 factors next to the tables")
    ap.add_argument("--noise", action="store_true", help="use_noise: noisy fine-tuning")
    ap.add_argument("--dropout-rng", choices=("host", "device"), default="host")
    ap.add_argument("--seed", type=int, default=2023)
    a = ap.parse_args()
    torch.manual_seed(a.seed)
    np.random.seed(a.seed)
    dev = torch.device("cuda")
    with tempfile.TemporaryDirectory() as tmp:
        root = a.data_path or tmp
        if not a.data_path:
            synthetic_files(tmp, a.stages, seed=a.seed)
        f = lambda n: os.path.join(root, n + ".txt")   # noqa: E731
        tests = [f(f"test_{s}") for s in range(1, a.stages + 1)]
        data = EdgeListData(f("pretrain"), f("pretrain_val"), device=dev)
        print(f"{data.num_users} users x {data.num_items} items, {data.num_edges} pre-training interactions, {len(tests)} stages")
        model = RAGraph(data, None, phase="pretrain", device=dev)
        model.dropout_rng = a.dropout_rng
        t0 = time.time()
        pre = Trainer(data, lr=a.lr, batch_size=a.batch_size, num_epochs=a.pretrain_epochs, log=print)
        best = pre.train(model)
        pre_state = pre.best_state if pre.best_state is not None else model.state_dict()
        print(f"pre-training: recall@20 {best['recall'][0]:.4f} ndcg@20 {best['ndcg'][0]:.4f} ({time.time() - t0:.1f} s)")
        stage_t = [time.time()]

        def on_stage(stage, pre_model, ft_model, trainer):
            stage_t.append(time.time())
            bp = trainer.best_perform
            print(f"stage {stage}: {trainer.dataloader.num_edges} interactions, recall@20 {bp['recall'][0]:.4f} "
                  f"ndcg@20 {bp['ndcg'][0]:.4f} ({stage_t[-1] - stage_t[-2]:.2f} s with its datasets and models)")

        out = run_stages(f("pretrain"), f("pretrain_val"), f("fine_tune"), tests, pre_state, updt_inter=a.updt_inter,
                         model_kwargs={"use_LoRA": a.lora, "use_noise": a.noise, "dropout_rng": a.dropout_rng},
                         trainer_kwargs={"lr": a.lr, "batch_size": a.batch_size, "num_epochs": a.epochs}, device=dev,
                         on_stage=on_stage)
    print(f"recalls: {[round(float(r), 4) for r in out['recalls']]}\nndcgs:   {[round(float(x), 4) for x in out['ndcgs']]}\n"
          f"avg. recall: {out['recall_mean']} std. {out['recall_std']}, avg. ndcg: {out['ndcg_mean']} std. {out['ndcg_std']}")


if __name__ == "__main__":
    main()
