#!/usr/bin/env python3
"""Generate tests/golden/g19_edge_pretrain.npz by running the REFERENCE's own edge-flavour pre-training pieces on CPU
(RAGraph_edge: utils/dataloader.py EdgeListData(phase="pretrain"), modules/RAGraph.py RAGraph(phase="pretrain") and
RAGraph(phase="for_tune")).

Uses oracle/make_golden.py's import context unchanged.  The training TSV is small (D = 64, tens of users and items), has
one user on two lines (the last line wins in train_user_dict) and one repeated (user, item) pair.  Recorded:
  * train_txt / test_txt, num_users, num_items, and the reference model's edges / edge_norm / edge_times;
  * init_user / init_item: the xavier tables after torch.manual_seed(SEED_INIT);
  * hist_users / hist_items: train_user_dict flattened (user, item) in dict order, repeats kept as the dict holds them;
  * users / pos / neg: get_train_batch(0, B) after np.random.seed(SEED_BATCH) and shuffle();
  * mask: the edge-dropout mask cal_loss draws after torch.manual_seed(SEED_STEP) (torch.rand on the CPU generator);
  * loss / rec / reg, g_user / g_item (table gradients), user_after / item_after (one Adam(lr=1e-3) step);
  * state_keys: the pretrain model's state-dict keys;
  * ft_user / ft_item: generate() of a for_tune model loaded strictly from that state dict, after
    torch.manual_seed(SEED_GATE).

Usage:  python tools/make_golden_edge_pretrain.py   (writes tests/golden/g19_edge_pretrain.npz)
"""
from __future__ import annotations

import contextlib
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.make_golden import _install_shims, ref_project, save  # noqa: E402

U, I, B = 30, 24, 48
SEED_INIT, SEED_BATCH, SEED_STEP, SEED_GATE = 19, 190, 1919, 91


def _tsv(rng):
    lines = []
    for u in range(U):
        if u == 11:
            continue                                          # a user without interactions
        k = int(rng.integers(2, 8))
        items = rng.choice(I, size=k, replace=False)
        if u == 6:
            items = np.array([3, 17, 3, 9])                   # a repeated (user, item) pair
        times = 1_600_000_000 + rng.integers(0, 30 * 3600, len(items))
        lines.append(f"{u}\t{' '.join(map(str, items))}\t{' '.join(map(str, times))}")
        if u == 4:                                            # user 4 on a second line: train_user_dict keeps this one
            lines.append(f"4\t5 12 20\t{' '.join(str(1_600_000_000 + 3600 * h) for h in (2, 7, 29))}")
    train = "\n".join(lines) + "\n"
    test = "".join(f"{u}\t{' '.join(map(str, rng.choice(I, size=3, replace=False)))}\n" for u in (0, 4, 9, 23, 29))
    return train, test


def main():
    _install_shims()
    rng = np.random.default_rng(1919)
    train_txt, test_txt = _tsv(rng)
    argv = ["x", "--device", "cpu", "--data_path", "dataset/amazon", "--log", "0", "--emb_dropout", "0"]
    with ref_project("RAGraph_edge", argv=argv):
        from modules.RAGraph import RAGraph
        from utils.dataloader import EdgeListData

        with tempfile.TemporaryDirectory() as d:
            tr, te = os.path.join(d, "train.txt"), os.path.join(d, "test.txt")
            open(tr, "w").write(train_txt)
            open(te, "w").write(test_txt)
            with contextlib.redirect_stdout(open(os.devnull, "w")):
                ds = EdgeListData(tr, te, phase="pretrain")
        assert ds.num_users == U and ds.num_items == I, (ds.num_users, ds.num_items)
        assert ds.train_user_dict[4] == [5, 12, 20] and ds.train_user_dict[6] == [3, 17, 3, 9]

        torch.manual_seed(SEED_INIT)
        model = RAGraph(ds, phase="pretrain", use_RAG=False)
        init_user = model.user_embedding.detach().clone()
        init_item = model.item_embedding.detach().clone()

        np.random.seed(SEED_BATCH)
        ds.shuffle()
        users, pos, neg = ds.get_train_batch(0, B)
        for uu, nn_ in zip(users.tolist(), neg.tolist()):
            assert nn_ not in ds.train_user_dict[uu]

        n_e = model.edges.shape[0]
        torch.manual_seed(SEED_STEP)
        mask = (torch.rand(n_e) + 0.5).floor().bool()          # the draw of EdgelistDrop (modules/utils.py:46)
        torch.manual_seed(SEED_STEP)
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        opt.zero_grad()
        loss, parts = model.cal_loss((users, pos, neg))
        loss.backward()
        g_user = model.user_embedding.grad.detach().clone()
        g_item = model.item_embedding.grad.detach().clone()
        opt.step()
        state = model.state_dict()
        state_keys = list(state.keys())

        ft = RAGraph(ds, phase="for_tune", use_RAG=False)
        ft.load_state_dict(state, strict=True)
        ft.eval()
        torch.manual_seed(SEED_GATE)
        ft_user, ft_item = ft.generate()

    hist_users = np.array([u for u, v in ds.train_user_dict.items() for _ in v], dtype=np.int64)
    hist_items = np.array([x for v in ds.train_user_dict.values() for x in v], dtype=np.int64)
    print(f"  {U} users x {I} items, {ds.num_edges} interactions, {n_e} directed edges; loss {float(loss):.6f} "
          f"(rec {parts['rec_loss']:.6f}, reg {parts['reg_loss']:.3e}); {int(mask.sum())} edges kept")
    save("g19_edge_pretrain", train_txt=np.array(train_txt), test_txt=np.array(test_txt), num_users=np.int64(U),
         num_items=np.int64(I), edges=model.edges, edge_norm=model.edge_norm, edge_times=model.edge_times,
         seeds=np.array([SEED_INIT, SEED_BATCH, SEED_STEP, SEED_GATE], dtype=np.int64), init_user=init_user,
         init_item=init_item, hist_users=hist_users, hist_items=hist_items, users=users, pos=pos, neg=neg, mask=mask,
         loss=np.float32(float(loss)), rec=np.float64(parts["rec_loss"]), reg=np.float64(parts["reg_loss"]), g_user=g_user,
         g_item=g_item, user_after=state["user_embedding"], item_after=state["item_embedding"],
         state_keys=np.array(state_keys), ft_user=ft_user, ft_item=ft_item)


if __name__ == "__main__":
    main()
