#!/usr/bin/env python3
"""Generate tests/golden/g20_edge_stages.npz by running the REFERENCE's own staged fine-tuning pieces on the CPU
(RAGraph_edge: utility.py merge_pd, utils/dataloader.py EdgeListData with pre_dataset / phase="finetune" / user_hist_files,
and the interpolative-update lines of finetune_rag.py:70-86, executed from the reference's file).

Uses oracle/make_golden.py's import context unchanged.  The data: 30 users x 24 items in five small TSVs -- pretrain,
pretrain_val, fine_tune, test_1, test_2 -- with users absent from later files, user 11 only in later files (the left join
drops it), (user, item) pairs repeated across files, and lines of one and of several items in every file (so pandas reads
the item column as strings).  Recorded, for the stages s = 1, 2 of finetune_rag.py:61-154:
  * s{s}_merged_txt: the merged frame as TSV; s{s}_pre_*: the merged dataset's edgelist, edge_time, num_users, num_items
    and train_user_dict (dict order) as keys / rowptr / items;
  * s{s}_ft_*: the same of the fine-tuning dataset, and s{s}_ft_hist_*: its user_hist_dict, raw (duplicates kept);
  * weights_{I}: the interpolation weights for interval I = 1, 2, 3, 7;
  * tables [3, 37, 64] (row 0 is zero in every table) and, for S = 2, 3 (interval S - 1, tables[0] the pre-trained one,
    tables[1] the newest saved), mix_S -- the weighted sum before F.normalize -- and out_S, the normalised result.

Usage:  python tools/make_golden_edge_stages.py   (writes tests/golden/g20_edge_stages.npz)
"""
from __future__ import annotations

import contextlib
import os
import sys
import tempfile
import textwrap
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.make_golden import REF, _install_shims, ref_project, save  # noqa: E402

U, I = 30, 24
T0 = 1_600_000_000
NAMES = ("pretrain", "pretrain_val", "fine_tune", "test_1", "test_2")


def _line(u, items, times=None):
    s = f"{u}\t{' '.join(map(str, items))}"
    return s if times is None else s + f"\t{' '.join(map(str, times))}"


def _tsvs(rng):
    """file name -> text.  File f's times lie in day f."""
    def block(users, day, kmin, kmax, fixed=None):
        lines = []
        for u in users:
            k = int(rng.integers(kmin, kmax + 1))
            items = (fixed or {}).get(u)
            if items is None:
                items = rng.choice(I, size=k, replace=False)
            times = T0 + day * 86400 + rng.integers(0, 20 * 3600, len(items))
            lines.append(_line(u, items, times))
        return "\n".join(lines) + "\n"

    pre_users = [u for u in range(U) if u not in (11, 19)]               # 11: only in later files; 19: nowhere
    txt = {"pretrain": block(pre_users, 0, 2, 6, {6: [3, 17, 3, 9], 2: [23]}),
           "pretrain_val": "".join(_line(u, rng.choice(I, size=2, replace=False)) + "\n" for u in (0, 4, 9, 23, 29))}
    # later files, in an order of their own; some users absent, user 11 present, pairs of earlier files repeated
    ft_users = [7, 0, 11, 3, 28, 6, 14, 21, 9, 25, 1, 16]
    txt["fine_tune"] = block(ft_users, 1, 1, 4, {6: [3, 5], 0: [12]})
    t1_users = [5, 6, 0, 11, 29, 13, 3, 22, 8, 17, 26, 10]
    txt["test_1"] = block(t1_users, 2, 1, 4, {6: [17, 20], 5: [1]})
    t2_users = [6, 2, 11, 0, 18, 3, 27, 12, 24]
    txt["test_2"] = block(t2_users, 3, 1, 4, {0: [12, 7], 18: [4]})
    return txt


def _csr(d):
    keys = np.fromiter(d.keys(), dtype=np.int64, count=len(d))
    rowptr = np.zeros(len(d) + 1, dtype=np.int64)
    np.cumsum([len(v) for v in d.values()], out=rowptr[1:])
    items = np.array([x for v in d.values() for x in v], dtype=np.int64)
    return keys, rowptr, items


def _dataset_arrays(prefix, ds, hist=False):
    out = {f"{prefix}_edgelist": np.asarray(ds.edgelist, dtype=np.int64), f"{prefix}_edge_time": np.asarray(ds.edge_time).astype(np.int64),
           f"{prefix}_num_users": np.int64(ds.num_users), f"{prefix}_num_items": np.int64(ds.num_items)}
    assert np.array_equal(out[f"{prefix}_edge_time"], np.asarray(ds.edge_time)), "time steps are whole numbers"
    for name, d in (("train", ds.train_user_dict),) + ((("hist", ds.user_hist_dict),) if hist else ()):
        k, r, i = _csr(d)
        out.update({f"{prefix}_{name}_keys": k, f"{prefix}_{name}_rowptr": r, f"{prefix}_{name}_items": i})
    return out


def _reference_lines(first, last):
    """Lines first..last (1-based, inclusive) of the reference's finetune_rag.py, dedented."""
    with open(os.path.join(REF, "RAGraph_edge", "finetune_rag.py")) as f:
        lines = f.readlines()
    return textwrap.dedent("".join(lines[first - 1:last]))


def _interpolate(tables, upto):
    """Execute finetune_rag.py:70-`upto` on all_state_dict = [{'user_embedding': t} for t in tables] (85: the weighted sum,
    86: with F.normalize)."""
    code = _reference_lines(70, upto)
    assert "pretrain_weight = 0.5" in code and "interpolative_weight" in code and ("torch.stack" in code) == (upto >= 85) \
        and ("F.normalize(state_dict[k], dim=1)" in code) == (upto >= 86), "finetune_rag.py:70-86 is not the interpolative update any more"
    ns = {"torch": torch, "F": torch.nn.functional, "args": types.SimpleNamespace(device="cpu"), "interval": len(tables) - 1,
          "all_state_dict": [{"user_embedding": t, "gating_weight": torch.zeros(2, 2)} for t in tables]}
    exec(compile(code, "finetune_rag.py:70-%d" % upto, "exec"), ns)
    if upto < 85:
        return ns["interpolative_weight"].reshape(-1), None
    assert list(ns["state_dict"]) == ["user_embedding"]
    return ns["interpolative_weight"].reshape(-1), ns["state_dict"]["user_embedding"]


def main():
    _install_shims()
    rng = np.random.default_rng(2020)
    txt = _tsvs(rng)
    out = {f"{n}_txt": np.array(txt[n]) for n in NAMES}
    argv = ["x", "--device", "cpu", "--data_path", "dataset/amazon", "--log", "0", "--emb_dropout", "0"]
    with ref_project("RAGraph_edge", argv=argv):
        import pandas as pd
        from utility import merge_pd
        from utils.dataloader import EdgeListData
        from utils.parse_args import args as ref_args

        with tempfile.TemporaryDirectory() as d, contextlib.redirect_stdout(open(os.devnull, "w")):
            path = {n: os.path.join(d, n + ".txt") for n in NAMES}
            for n in NAMES:
                open(path[n], "w").write(txt[n])
            all_data = [path["pretrain"], path["fine_tune"], path["test_1"], path["test_2"]]
            pretrain_dataset = EdgeListData(path["pretrain"], path["pretrain_val"])
            assert (pretrain_dataset.num_users, pretrain_dataset.num_items) == (U, I)
            for num_stage in (1, 2):                                     # finetune_rag.py:96-154
                test_data_idx = num_stage + 1
                ft_data_idx = test_data_idx - 1
                all_data_pd = [pd.read_csv(p, sep="\t", names=["user", "item", "time"]) for p in all_data]
                merged_pre_pd = merge_pd(all_data_pd[:ft_data_idx + 1])
                out[f"s{num_stage}_merged_txt"] = np.array("".join(
                    f"{int(r.iloc[0])}\t{r.iloc[1]}\t{r.iloc[2]}\n" for _, r in merged_pre_pd.iterrows()))
                pre_dataset = EdgeListData(train_file=merged_pre_pd, test_file=all_data_pd[ft_data_idx], has_time=True,
                                           pre_dataset=pretrain_dataset)
                finetune_dataset = EdgeListData(train_file=all_data[ft_data_idx], test_file=path[f"test_{num_stage}"],
                                                phase="finetune", pre_dataset=pre_dataset, has_time=True,
                                                user_hist_files=all_data[:ft_data_idx])
                out.update(_dataset_arrays(f"s{num_stage}_pre", pre_dataset))
                out.update(_dataset_arrays(f"s{num_stage}_ft", finetune_dataset, hist=True))
                # (a "pretrain"-phase train_user_dict IS the user_hist_dict, dataloader.py:35: users without a line hold [])
                assert pre_dataset.train_user_dict[11] == [] and len(finetune_dataset.user_hist_dict[11]) > 0
        out["hour_interval_pre"] = np.int64(ref_args.hour_interval_pre)
        out["hour_interval_f"] = np.int64(ref_args.hour_interval_f)

    g = torch.Generator().manual_seed(2020)
    tables = torch.randn(3, 37, 64, generator=g)
    tables[:, 0] = 0.0
    out["tables"] = tables
    for interval in (1, 2, 3, 7):
        w, _ = _interpolate([torch.zeros(1, 1)] * (interval + 1), 79)
        out[f"weights_{interval}"] = w
    for S in (2, 3):
        _, out[f"mix_{S}"] = _interpolate(list(tables[:S]), 85)
        _, out[f"out_{S}"] = _interpolate(list(tables[:S]), 86)
    save("g20_edge_stages", **out)


if __name__ == "__main__":
    main()
