"""Ordered top-k beyond k = 64, host side: the header / binding constants, workspace sizes (k <= 64 unchanged, k > 64
large enough for the score slabs), KeyIndex's large-k route (oracle-backed ops on CPU tensors) and the sharded bank's
k limit (gloo world 2).  No GPU needed."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_define(name):
    with open(os.path.join(ROOT, "include", "ragraph_hip.h")) as f:
        m = re.search(rf"#define\s+{name}\s+(\d+)", f.read())
    assert m, name
    return int(m.group(1))


def test_ordered_max_matches_header():
    from ragraph_amd import _native as N

    assert _header_define("RAGRAPH_TOPK_ORDERED_MAX") == N.TOPK_ORDERED_MAX == 4096
    assert _header_define("RAGRAPH_TOPK_MAX") == N.TOPK_MAX == 64


# ragraph_topk_cosine_workspace_bytes(B, N, D, k) for k <= 64, as the library computed them before large k existed
COSINE_WS_K64 = [
    ((1, 5000, 256, 10), 21248),
    ((64, 20000, 256, 10), 5185536),
    ((16, 1000000, 256, 10), 344064),
    ((1024, 1000000, 256, 32), 17825792),
    ((100, 50000, 100, 20), 20040192),
    ((8, 200000, 64, 40), 6402048),
    ((512, 300000, 128, 64), 614662144),
    ((2, 8388608, 64, 50), 33557760),
    ((4096, 169343, 256, 41), 1077829120),
]


@pytest.mark.parametrize("shape,nbytes", COSINE_WS_K64)
def test_cosine_workspace_unchanged_for_k_up_to_64(shape, nbytes):
    from ragraph_amd import _native as N

    assert N.lib().ragraph_topk_cosine_workspace_bytes(*shape) == nbytes


@pytest.mark.parametrize("B,Nk,k", [(3, 65, 65), (9, 70001, 1000), (2, 300001, 4096), (3, 1 << 20, 128), (1000, 1 << 20, 4096)])
def test_rows_large_workspace(B, Nk, k):
    """Rows of >= 65536 scores keep k candidates per chunk of at most 65536 scores; shorter rows need none."""
    from ragraph_amd import _native as N

    ws = N.lib().ragraph_topk_rows_large_workspace_bytes(B, Nk, k)
    if Nk < 65536:
        assert ws == 0
    else:
        assert ws >= B * -(-Nk // 65536) * k * 8
    assert N.lib().ragraph_topk_rows_large_workspace_bytes(B, Nk, 4097) == 0


@pytest.mark.parametrize("B,Nk,D,k", [(8, 5000, 64, 65), (8, 200000, 100, 512), (64, 1 << 20, 256, 128),
                                      (2, 8 << 20, 64, 256), (1024, 1 << 20, 256, 4096)])
def test_cosine_workspace_large_k_holds_the_slabs(B, Nk, D, k):
    from ragraph_amd import _native as N

    rows = min(B, max(64, (1 << 30) // (4 * Nk)))
    G = -(-Nk // (65535 * 64))
    nc = -(-Nk // G)
    ws = N.lib().ragraph_topk_cosine_workspace_bytes(B, Nk, D, k)
    need = B * D * 4 + rows * nc * 4 + (rows * G * k * 8 if G > 1 else 0)
    assert ws >= need + N.lib().ragraph_topk_rows_large_workspace_bytes(rows, nc, k)


class _Ops:
    """The kernels KeyIndex needs, answered by the CPU oracle; records the topk_cosine calls."""

    calls = []

    @staticmethod
    def padded_dim(D):
        return D if D in (64, 128, 256) else None

    @staticmethod
    def pad_cols(x, width):
        out = x.new_zeros((x.shape[0], width))
        out[:, :x.shape[1]] = x
        return out

    @staticmethod
    def dedup_rows(kn):
        U, largest, uniq, ptr, mem = cref.dedup_rows(kn.numpy())
        return U, largest, torch.from_numpy(uniq), torch.from_numpy(ptr), torch.from_numpy(mem)

    @classmethod
    def topk_cosine(cls, q, kn, k, idx_base=0):
        cls.calls.append((tuple(kn.shape), k, idx_base))
        s, i = cref.topk_cosine(q.numpy(), kn.numpy(), k, idx_base)
        return torch.from_numpy(s), torch.from_numpy(i)

    @staticmethod
    def normalize_rows(x):
        return torch.from_numpy(cref.normalize_rows(x.numpy()))

    @staticmethod
    def gather_reduce(v, l, idx, idx_base=0, v_scale=1.0):
        a, b = cref.gather_reduce(v.numpy(), None if l is None else l.numpy(), idx.numpy(), idx_base, v_scale)
        return torch.from_numpy(a), (None if b is None else torch.from_numpy(b))

    @staticmethod
    def gather_rows(v, idx, idx_base=0):
        return torch.from_numpy(cref.gather_rows(v.numpy(), idx.numpy(), idx_base))

    @staticmethod
    def topk_merge(s, i):
        a, b = cref.topk_merge(s.numpy(), i.numpy())
        return torch.from_numpy(a), torch.from_numpy(b)

    @staticmethod
    def topk_expand_groups(su, iu, ptr, mem, k, idx_base=0, idx_base_u=0):
        s, i = cref.topk_expand_groups(su.numpy(), iu.numpy(), ptr.numpy(), mem.numpy(), k, idx_base, idx_base_u)
        return torch.from_numpy(s), torch.from_numpy(i)


def test_key_index_routes_large_k_to_the_full_bank():
    from ragraph_amd.kernels_index import KeyIndex

    rng = np.random.default_rng(3)
    base = cref.normalize_rows(rng.standard_normal((300, 64), dtype=np.float32))
    kn = base[rng.integers(0, 300, 1200)]                       # duplicate rows: k <= 64 calls search a collapsed bank
    q = rng.standard_normal((5, 64), dtype=np.float32)
    idx = KeyIndex(torch.from_numpy(kn), ops=_Ops)
    _Ops.calls.clear()
    s, i = idx.topk(torch.from_numpy(q), 100, idx_base=7)
    assert _Ops.calls == [((1200, 64), 100, 7)]                 # one call, the full uncollapsed bank
    ws, wi = cref.topk_cosine(q, kn, 100, 7)
    assert np.array_equal(i.numpy(), wi) and np.array_equal(s.numpy(), ws)
    assert idx._queries == 0 and idx.last_prior is None and idx._pending is None


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sharded_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ragraph_amd._native import RagraphNativeError
        from ragraph_amd.sharded import ShardedToyGraphBase, shard_bounds

        N, D, C = 2000, 64, 3
        rng = np.random.default_rng(0)
        keys = cref.normalize_rows(rng.standard_normal((N, D), dtype=np.float32))
        vals = rng.standard_normal((N, D), dtype=np.float32)
        labs = np.eye(C, dtype=np.float32)[rng.integers(0, C, N)]
        q = torch.from_numpy(rng.standard_normal((6, D), dtype=np.float32))
        lo, hi = shard_bounds(N, world, rank)
        tgb = ShardedToyGraphBase(torch.from_numpy(keys[lo:hi]), torch.from_numpy(vals[lo:hi]), torch.from_numpy(labs[lo:hi]),
                                  lo, 10, ops=_Ops)
        msgs = []
        for call in (lambda: tgb.topk(q, 65), lambda: tgb.topk_rows(q, 100)):
            try:
                call()
                msgs.append("")
            except RagraphNativeError as e:
                msgs.append(str(e))
        s, i = tgb.topk(q, 10)            # the group is still in step: no collective was started by the failed calls
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), msgs=np.array(msgs), i=i.numpy())
    finally:
        dist.destroy_process_group()


def test_sharded_large_k_raises_on_every_rank(tmp_path):
    world = 2
    mp.spawn(_sharded_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    rng = np.random.default_rng(0)
    keys = cref.normalize_rows(rng.standard_normal((2000, 64), dtype=np.float32))
    rng.standard_normal((2000, 64), dtype=np.float32)
    rng.integers(0, 3, 2000)
    q = rng.standard_normal((6, 64), dtype=np.float32)
    _, want = cref.topk_cosine(q, keys, 10)
    for r in range(world):
        out = np.load(os.path.join(tmp_path, f"r{r}.npz"))
        assert all("64" in m and "k=" in m for m in out["msgs"]), out["msgs"]
        assert np.array_equal(out["i"], want)
