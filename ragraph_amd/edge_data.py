"""Edge-list ingestion for the link-prediction flavour -- a vectorised restatement of
RAGraph_edge/utils/dataloader.py:14-124,186-196 and RAGraph_edge/modules/base_model.py:34-52.

File format (the reference's): one line per user, TAB-separated `user \t items (space-sep) \t unix times (space-sep)`.
Produces what RAGraph_edge.RAGraph consumes, directly as device tensors:
  edges [2E,2] int64 (src,dst) over the joint id space (items offset by num_users), both directions, sorted by
  destination then source (the order the reference's transposed scipy product leaves them in), edge_norm [2E] = d^-1/2[src] d^-1/2[dst] on the 0/1 bipartite
  graph, edge_times [2E] = 1 + (t - t_min) // (hour_interval * 3600)  (dataloader.py:94,186-196).
The reference builds these through Python loops over every edge and a dict-of-dicts; here it is numpy on the host
(one-off preprocessing, not on the per-forward path).
"""
from __future__ import annotations

import numpy as np
import torch


def _read_lines(path):
    """The lines of a file in order as [(user, items int64 array, times int64 array)]; a line without a time column gets
    zero times, a line without items is skipped."""
    lines = []
    with open(path, "r") as f:
        for line in f:
            parts = line.rstrip("\n").split("\t")
            if len(parts) < 2 or not parts[1]:
                continue
            it = np.array(parts[1].split(" "), dtype=np.int64)
            tm = np.array(parts[2].split(" "), dtype=np.int64) if (len(parts) > 2 and parts[2]) else np.zeros_like(it)
            lines.append((int(parts[0]), it, tm))
    return lines


def _check_unique_users(frame, what):
    seen = set()
    for line in frame:
        if line[0] in seen:
            raise ValueError(f"{what} names user {line[0]} twice: the reference's pd.merge would multiply its rows "
                             "(utility.py:23), which is not reproduced")
        seen.add(line[0])


def read_frame(path):
    """pd.read_csv(path, sep="\t", names=["user", "item", "time"]) (finetune_rag.py:106-114) without pandas: the file's lines
    in order as a list of (user, items int64 array, times int64 array).  A frame is a table keyed by user: a file that names
    a user twice raises ValueError."""
    frame = _read_lines(path)
    _check_unique_users(frame, str(path))
    return frame


def merge_frames(frames):
    """utility.py:16-35 merge_pd: a left join on the FIRST frame's users, in its order; per user the items and times of the
    later frames are appended in frame order; users absent from the first frame are dropped.  A single frame (not a list)
    is returned as it is (:17-18)."""
    if not isinstance(frames, list) or (frames and isinstance(frames[0], tuple)):
        return frames
    for j, fr in enumerate(frames):
        _check_unique_users(fr, f"frame {j}")
    later = [{u: (it, tm) for u, it, tm in fr} for fr in frames[1:]]
    merged = []
    for u, it, tm in frames[0]:
        more = [d[u] for d in later if u in d]
        merged.append((u, np.concatenate([it] + [m[0] for m in more]), np.concatenate([tm] + [m[1] for m in more])))
    return merged


def _is_frame(x):
    return isinstance(x, (list, tuple))


def _read(source, has_time=True):
    """A file (path) or a frame (dataloader.py:47-93 _read_file / _read_pd) -> flat (users, items, times) in line order and
    the per-user dict, in which a user's LAST line stands (:61,85)."""
    users, items, times = [], [], []
    per_user = {}
    for u, it, tm in (source if _is_frame(source) else _read_lines(source)):
        users.append(np.full(it.shape, u, dtype=np.int64))
        items.append(it)
        times.append(tm if has_time else np.zeros_like(it))
        per_user[u] = it.tolist()
    cat = (lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64))
    return cat(users), cat(items), cat(times), per_user


class EdgeListData:
    """The interactions of one training file.  Besides the graph tensors above, for pre-training (dataloader.py:140-167):
    edgelist [num_edges, 2] int64 (user, item) and edge_time [num_edges] int64 -- every line's pairs in file order, repeats
    included (the reference's self.edgelist / self.edge_time) -- and the training-history CSR hist_rowptr / hist_items of
    train_user_dict (the negative sampler's exclusion sets), all on `device`; shuffle() and get_train_batch()."""

    def __init__(self, train_file, test_file=None, hour_interval=1, has_time=True, num_users=None, num_items=None,
                 device="cuda", phase="pretrain", pre_dataset=None, user_hist_files=()):
        """train_file / test_file: a path or a frame (read_frame, merge_frames), as dataloader.py:95-99.
        pre_dataset: the dataset whose num_users / num_items this one takes (:106-108).
        phase="finetune" (:36-45,126-135): user_hist_dict -- what an evaluation masks out of the ranking -- is a copy of
        train_user_dict extended, in file order, by the items of every line of every file of user_hist_files (duplicates
        kept); train_user_dict itself, the sampler's exclusion sets, is not extended."""
        if phase not in ("pretrain", "finetune"):
            raise ValueError(f"phase: 'pretrain' or 'finetune', not {phase!r}")
        u, i, t, train_user_dict = _read(train_file, has_time)
        self._setup(u, i, t, train_user_dict, _read(test_file, False)[3] if test_file else {}, hour_interval, num_users,
                    num_items, device, phase, pre_dataset, user_hist_files)

    @classmethod
    def from_interactions(cls, users, items, times, test_user_dict=None, hour_interval=1, num_users=None, num_items=None,
                          device="cuda"):
        """The same object from interaction arrays (numpy, file order) instead of a file: each user's history is every item
        it has (as if all of a user's pairs stood on one line)."""
        u, i = np.asarray(users, np.int64), np.asarray(items, np.int64)
        t = np.asarray(times, np.int64)
        order = np.argsort(u, kind="stable")
        us, starts = np.unique(u[order], return_index=True)
        train_user_dict = dict(zip(us.tolist(), (x.tolist() for x in np.split(i[order], starts[1:])))) if u.size else {}
        obj = cls.__new__(cls)
        obj._setup(u, i, t, train_user_dict, dict(test_user_dict or {}), hour_interval, num_users, num_items, device)
        return obj

    def _setup(self, u, i, t, train_user_dict, test_user_dict, hour_interval, num_users, num_items, device,
               phase="pretrain", pre_dataset=None, user_hist_files=()):
        self.phase, self.pre_dataset = phase, pre_dataset
        self.train_user_dict = train_user_dict
        self.test_user_dict = test_user_dict
        if pre_dataset is not None:                                      # dataloader.py:106-108
            num_users, num_items = pre_dataset.num_users, pre_dataset.num_items
        tu = max(self.test_user_dict) + 1 if self.test_user_dict else 0
        ti = max(max(v) for v in self.test_user_dict.values()) + 1 if self.test_user_dict else 0
        self.num_users = int(num_users or max(u.max() + 1, tu))          # dataloader.py:100-101
        self.num_items = int(num_items or max(i.max() + 1, ti))
        self.num_edges = int(u.shape[0])
        step = 1 + (t - t.min()) // int(hour_interval * 3600)            # :94,186-196 (0 is the self-loop padding)
        if phase == "finetune":                                          # :36-45,126-135
            self.user_hist_dict = {uu: list(v) for uu, v in self.train_user_dict.items()}
            for source in user_hist_files:
                for uu, it, _ in (source if _is_frame(source) else _read_lines(source)):
                    self.user_hist_dict.setdefault(uu, []).extend(it.tolist())
            for uu in range(self.num_users):
                self.user_hist_dict.setdefault(uu, [])
        else:
            self.user_hist_dict = {uu: self.train_user_dict.get(uu, []) for uu in range(self.num_users)}
        if torch.device(device).type == "cuda":   # the product path: sorts, degrees and norms on the device (csrc/ingest.hip)
            from . import kernels as K
            self.edges, self.edge_norm, self.edge_times = K.binorm_edges(
                torch.from_numpy(u).to(device), torch.from_numpy(i).to(device), torch.from_numpy(step.astype(np.int64)).to(device),
                self.num_users, self.num_items)
        else:                                      # host tensors (the CPU host-logic test): the numpy restatement below
            edges, norm, times = binorm_edges(self.num_users, self.num_items, u, i, step)
            self.edges = torch.from_numpy(edges).to(device)
            self.edge_norm = torch.from_numpy(norm).to(device)
            self.edge_times = torch.from_numpy(times).to(device)
        # pre-training (dataloader.py:140-167): the interactions in file order, and the history CSR the sampler excludes
        self.edgelist = torch.from_numpy(np.stack([u, i], 1).astype(np.int64)).to(device)
        self.edge_time = torch.from_numpy(step.astype(np.int64)).to(device)
        rowptr, items = flatten_history(self.train_user_dict, self.num_users, self.num_items)
        self.hist_rowptr, self.hist_items = torch.from_numpy(rowptr).to(device), torch.from_numpy(items).to(device)
        if torch.device(device).type == "cuda":   # checked once (one read-back): a later batch needs none
            from . import kernels as K
            K.edge_hist_check(self.hist_rowptr, self.hist_items, self.num_items)

    def shuffle(self):
        """dataloader.py:164-167: one permutation of the interactions (torch.randperm on the generator of their device)."""
        perm = torch.randperm(self.num_edges, device=self.edgelist.device)
        self.edgelist = self.edgelist[perm]
        self.edge_time = self.edge_time[perm]

    def get_train_batch(self, start, end, n_negs=1):
        """dataloader.py:140-162: (users, pos_items, neg_items) of interactions [start, end) (slicing semantics), as device
        int64; neg_items [B * n_negs] triple-major, each uniform over the items outside the user's train_user_dict entry
        (kernels.edge_neg_sample; the seed drawn on the device generator, so torch.manual_seed reproduces a batch).  No
        synchronisation: every user of the edge list is a key of train_user_dict, whose ids were checked when the history
        was built.  There is no CPU sampler (RagraphNativeError)."""
        from . import kernels as K
        ui = self.edgelist[start:end]
        users, pos_items = ui[:, 0].contiguous(), ui[:, 1].contiguous()
        seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=users.device)
        neg_items = K.edge_neg_sample(self.hist_rowptr, self.hist_items, self.num_items, users, n_negs, seed,
                                      check_users=False)
        return users, pos_items, neg_items

    def history_csr(self, users, device="cuda"):
        """CSR of training-history items for `users` (the mask of metrics.py:210-214)."""
        lens = [len(self.user_hist_dict.get(int(x), [])) for x in users]
        rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        cols = (np.concatenate([np.asarray(self.user_hist_dict.get(int(x), []), dtype=np.int64) for x in users])
                if sum(lens) else np.zeros(0, np.int64))
        return torch.from_numpy(rowptr).to(device), torch.from_numpy(cols).to(device)


def flatten_history(train_user_dict, num_users, num_items):
    """train_user_dict -> the negative sampler's exclusion sets as a CSR on the host: (rowptr int64 [num_users + 1], items
    int64), each row u the set of train_user_dict[u] (the dict already holds a user's LAST line, dataloader.py:61) with its
    repeats removed, ascending."""
    lens = np.fromiter((len(v) for v in train_user_dict.values()), dtype=np.int64, count=len(train_user_dict))
    users = np.repeat(np.fromiter(train_user_dict.keys(), dtype=np.int64, count=len(train_user_dict)), lens)
    items = np.fromiter((x for v in train_user_dict.values() for x in v), dtype=np.int64, count=int(lens.sum()))
    if users.size and (users.min() < 0 or users.max() >= num_users or items.min() < 0 or items.max() >= num_items):
        raise ValueError(f"train_user_dict holds ids outside {num_users} users x {num_items} items")
    key = np.unique(users * np.int64(num_items) + items)
    rowptr = np.zeros(num_users + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // num_items, minlength=num_users), out=rowptr[1:])
    return rowptr, (key % num_items).astype(np.int64)


def binorm_edges(num_users, num_items, u, i, step):
    """base_model.py:34-52: symmetric bipartite adjacency, binarised, D^-1/2 A D^-1/2, as a sorted COO edge list; the
    time of a duplicated (user,item) pair is its LAST occurrence (the dict assignment of dataloader.py:112-113)."""
    n = num_users + num_items
    key = u * num_items + i
    order = np.argsort(key, kind="stable")
    ks = key[order]
    last = np.r_[ks[1:] != ks[:-1], True] if ks.size else np.zeros(0, bool)   # last occurrence of each pair
    uu, ii, tt = u[order][last], i[order][last] + num_users, step[order][last]
    src = np.concatenate([uu, ii])
    dst = np.concatenate([ii, uu])
    tim = np.concatenate([tt, tt])
    deg = np.bincount(src, minlength=n).astype(np.float64)
    with np.errstate(divide="ignore"):
        dinv = np.power(deg, -0.5)
    dinv[np.isinf(dinv)] = 0.0
    norm = (dinv[src] * dinv[dst]).astype(np.float32)   # float64 product cast to fp32, as mat.data.astype(np.float32)
    o = np.lexsort((src, dst))   # by destination, then source: the order (A D)^T D .tocoo() leaves the reference
    return np.stack([src[o], dst[o]], 1).astype(np.int64), norm[o], tim[o].astype(np.int64)
