"""torch.Tensor front end of the C ABI (include/ragraph_hip.h).

PyTorch is plumbing here: it owns HBM allocations and the HIP stream; every number is produced by libragraph_hip.so.
All functions require CUDA(=ROCm) tensors and raise `RagraphNativeError` otherwise -- there is no eager fallback.
"""
from __future__ import annotations

import collections
import ctypes
import os

import torch

from . import _native as N
from ._native import ACT_ELU, ACT_LEAKY, ACT_NONE, ACT_PRELU, ACT_RELU, RagraphNativeError  # noqa: F401
from ._native import LINEAR_GENERIC, LINEAR_NARROW, LINEAR_SMALL, LINEAR_STREAM, LINEAR_TILE  # noqa: F401
from .filter_stats import MAGIC_VALUE as FILTER_STATS_MAGIC, levels as filter_stats_levels, ord2f  # noqa: F401  (the names tools import)

_device_ok = False


def _ready():
    global _device_ok
    if not _device_ok:
        N.require_device()
        _device_ok = True
    return N.lib()


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RagraphNativeError(f"{name}: expected a ROCm device tensor (ragraph_amd has no CPU fallback)")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _idxc(t: torch.Tensor, name: str, dtype=torch.int64) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RagraphNativeError(f"{name}: expected a ROCm device tensor")
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """The current HIP stream of the current device as an integer handle.  (torch.cuda.current_stream().cuda_stream
    builds a Stream object through three Python layers -- 3-4 us, a third of a small forward's host time; the raw
    accessor torch's own compiled graphs use is one C call.)"""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------
def normalize_rows(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """F.normalize(x, p=2, dim=-1) -- SimilarityFunctions.py:8,11."""
    L = _ready()
    x = _f32c(x, "normalize_rows.x")
    x2 = x.reshape(-1, x.shape[-1])
    if out is None:
        out = torch.empty_like(x2)
    N.check(L.ragraph_normalize_rows_f32(x2.data_ptr(), x2.shape[0], x2.shape[1], out.data_ptr(), _stream()),
            "normalize_rows")
    return out.reshape(x.shape)


_ws_cache: dict = {}      # insertion-ordered: least recently used first
_WS_CACHE_MAX = 8


def _workspace(nbytes: int, device) -> torch.Tensor:
    """One grow-only scratch buffer per (device index, current stream OF THAT DEVICE): calls on a stream are ordered, so
    reuse is safe.  The cache is bounded (least recently used entry dropped; torch's allocator keeps a dropped buffer
    alive until the work already enqueued on its stream has used it)."""
    dev = device.index if device.index is not None else torch.cuda.current_device()
    stream = _raw_stream(dev) if _raw_stream is not None else torch.cuda.current_stream(dev).cuda_stream
    key = (dev, stream)
    ws = _ws_cache.pop(key, None)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
    _ws_cache[key] = ws
    while len(_ws_cache) > _WS_CACHE_MAX:
        _ws_cache.pop(next(iter(_ws_cache)))
    return ws


def pack_keys(keys_normalized: torch.Tensor) -> torch.Tensor:
    """Packed copy of the bank (row = [even k | odd k]) for the LDS-DMA ring of the tile kernel; made once per bank
    update and passed to topk_cosine(keys_packed=...)."""
    L = _ready()
    kn = _f32c(keys_normalized, "pack_keys.keys")
    out = torch.empty_like(kn)
    if kn.shape[0] == 0:
        return out
    N.check(L.ragraph_pack_keys_f32(kn.data_ptr(), kn.shape[0], kn.shape[1], out.data_ptr(), _stream()), "pack_keys")
    return out


def packed_keys_help(B: int, D: int, k: int) -> bool:
    """True when topk_cosine(B queries, k) would use a packed bank copy (tile kernel, D = 256, 4-slot ring fits)."""
    return B > 128 and D == 256 and k <= 14


FUSED_WIDTHS = (64, 128, 256)   # row widths the fused / filtered top-k kernels are written for


def padded_dim(D: int):
    """The fused kernels' width that rows of D floats are zero-padded to (None beyond 256: such banks take the score-slab
    path of ragraph_topk_cosine_f32, any D).  Zero columns change no bit of a result: a row norm's lane tree adds +0 terms,
    a score's fmaf chain ends in fmaf(0, 0, acc) = acc (acc is never -0: the chain starts from +0)."""
    for w in FUSED_WIDTHS:
        if D <= w:
            return w
    return None


def pad_cols(x: torch.Tensor, width: int) -> torch.Tensor:
    """[n, D] -> [n, width] with zero columns behind (a copy; no arithmetic)."""
    x = _f32c(x, "pad_cols.x")
    if x.shape[1] == width:
        return x
    out = x.new_zeros((x.shape[0], width))
    out[:, :x.shape[1]] = x
    return out


def topk_cosine(q: torch.Tensor, keys_normalized: torch.Tensor, k: int, idx_base: int = 0,
                keys_packed: torch.Tensor | None = None):
    """Fused normalize(q) @ keys_normalized.T -> top-k.  Returns (scores [B,k] f32, idx [B,k] i64), canonical order.

    SimilarityFunctions.py:6-16 + ToyGraphBase.py:66-67.  `keys_normalized` must come from normalize_rows();
    `keys_packed` (optional) from pack_keys(keys_normalized) -- same bits out, faster key stream for B > 128.
    Any D >= 1: widths other than 64 / 128 / 256 take materialised score slabs (dense kernel + row top-k, same bits);
    KeyIndex pads banks narrower than 256 once and keeps them on the fused kernels.
    1 <= k <= min(N, TOPK_ORDERED_MAX): k > TOPK_MAX always takes exact fp32 score slabs and the ordered large-k selection."""
    L = _ready()
    q = _f32c(q, "topk_cosine.q")
    kn = _f32c(keys_normalized, "topk_cosine.keys")
    kp = 0
    if keys_packed is not None:
        kpt = _f32c(keys_packed, "topk_cosine.keys_packed")
        if kpt.shape != kn.shape:
            raise RagraphNativeError(f"topk_cosine: keys_packed {tuple(kpt.shape)} != keys {tuple(kn.shape)}")
        kp = kpt.data_ptr()
    if q.dim() != 2 or kn.dim() != 2 or q.shape[1] != kn.shape[1]:
        raise RagraphNativeError(f"topk_cosine: bad shapes {tuple(q.shape)} x {tuple(kn.shape)}")
    B, D = q.shape
    Nk = kn.shape[0]
    scores = torch.empty((B, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((B, k), dtype=torch.int64, device=q.device)
    if B == 0:
        return scores, idx
    nbytes = L.ragraph_topk_cosine_workspace_bytes(B, Nk, D, k)
    ws = _workspace(nbytes, q.device)
    N.check(L.ragraph_topk_cosine_bank_f32(q.data_ptr(), B, kn.data_ptr(), kp, Nk, D, k, idx_base, scores.data_ptr(),
                                           idx.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "topk_cosine")
    return scores, idx


def topk_cosine_mix_workspace_bytes(B: int, n_keys: int, D: int, A: int, k: int) -> int:
    """Workspace of topk_cosine_mix (a host computation: no device needed)."""
    return int(N.lib().ragraph_topk_cosine_mix_workspace_bytes(B, n_keys, D, A, k))


def topk_cosine_mix(q: torch.Tensor, keys_normalized: torch.Tensor, pos_q: torch.Tensor, pos_normalized: torch.Tensor,
                    w_struct: float, w_sem: float, k: int, idx_base: int = 0):
    """Top-k of  w_struct * cos(position codes) + w_sem * cos(embeddings)  -- RAGraph_node_fewshot/ragraph_utils/
    ToyGraphBase.py:47-65.  Returns (scores [B,k] f32, idx [B,k] i64), canonical order: the bits of linear x 2 + axpby +
    topk_rows on the materialised matrices, which the fused kernels (D in 64 / 128 / 256, k <= 32, w_sem > 0) never write.

    q [B,D] and pos_q [B,A] raw (normalised inside); keys_normalized [N,D] and pos_normalized [N,A] from normalize_rows();
    1 <= A <= 16, 1 <= k <= min(N, TOPK_ORDERED_MAX).  No synchronisation, no read-back: the call can be captured."""
    L = _ready()
    q = _f32c(q, "topk_cosine_mix.q")
    kn = _f32c(keys_normalized, "topk_cosine_mix.keys")
    pq = _f32c(pos_q, "topk_cosine_mix.pos_q")
    pn = _f32c(pos_normalized, "topk_cosine_mix.pos_normalized")
    if q.dim() != 2 or kn.dim() != 2 or q.shape[1] != kn.shape[1]:
        raise RagraphNativeError(f"topk_cosine_mix: bad shapes {tuple(q.shape)} x {tuple(kn.shape)}")
    if pq.dim() != 2 or pn.dim() != 2 or pq.shape[1] != pn.shape[1] or pq.shape[0] != q.shape[0] or pn.shape[0] != kn.shape[0]:
        raise RagraphNativeError(f"topk_cosine_mix: codes {tuple(pq.shape)} x {tuple(pn.shape)} do not match "
                                 f"{tuple(q.shape)} x {tuple(kn.shape)}")
    B, D = q.shape
    Nk, A = pn.shape
    scores = torch.empty((B, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((B, k), dtype=torch.int64, device=q.device)
    if B == 0:
        return scores, idx
    nbytes = L.ragraph_topk_cosine_mix_workspace_bytes(B, Nk, D, A, k)
    ws = _workspace(nbytes, q.device)
    N.check(L.ragraph_topk_cosine_mix_f32(q.data_ptr(), B, kn.data_ptr(), Nk, D, pq.data_ptr(), pn.data_ptr(), A,
                                          float(w_struct), float(w_sem), k, idx_base, scores.data_ptr(), idx.data_ptr(),
                                          ws.data_ptr(), ws.numel(), _stream()), "topk_cosine_mix")
    return scores, idx


MIX_FILTER_MAX_K = 64      # mix_filter_list(k) <= TOPK_FILTER_MAX: the longest list the filtered entries finish


def mix_filter_list(k: int) -> int:
    """k', the semantic candidates KeyIndex.topk_mix asks the filter for when the mixed top-k is wanted."""
    return min(128, max(32, 2 * k))


def mix_filter_helps(B: int, n_keys: int, D: int, k: int) -> bool:
    """True where the mixed top-k through the filter (KeyIndex.topk_mix: filtered semantic top-k', topk_mix_rerank, one 4-byte
    read-back, exact repair of the unproven rows) is the faster way to the bits of topk_cosine_mix.  Host arithmetic only;
    RAGRAPH_MIX_FILTER=0 (read per call) and RAGRAPH_EXACT_FP32=1 switch the route off."""
    if os.environ.get("RAGRAPH_MIX_FILTER", "1") == "0" or os.environ.get("RAGRAPH_EXACT_FP32") == "1":
        return False
    if D not in (64, 128, 256) or not 1 <= k <= MIX_FILTER_MAX_K:
        return False
    return mix_filter_measured(B, n_keys, D, k)


def mix_filter_measured(B: int, n_keys: int, D: int, k: int) -> bool:
    """The measured part of mix_filter_helps: the shapes where tools/topk_mix_filtered_probe.py measured the route faster than the
    exact fused call by more than the spread of the pair (profiles/topk_mix_filtered.txt).  What was not measured stays out."""
    # MI355X, ms per call, exact vs routed at the few-shot weights (0.001, 0.999), where no row is unproven (k = 10 / 20 / 40):
    #   100 000 x 1M x 256: 393 vs 20.5 / 403 vs 21.3 / 1649 vs 26.0;   4096 x 1M x 256: 18.0 vs 1.09 / 19.7 vs 1.13 / 67.4 vs 1.43;
    #   256 x 1M x 256: 1.86 vs 0.22 / 3.05 vs 0.23 / 4.22 vs 0.29;   100 000 x 1M x 128: 207 vs 11.8 / 215 vs 12.2 / 1309 vs 14.8;
    #   65 536 keys, D = 128 and 256, 256 / 4096 / 100 000 queries: ROUTE at every k.
    # The rule does not know the weights: where they leave most rows unproven -- (0.05, 0.95) at k >= 20 and (0.3, 0.7) everywhere on
    # that data -- the routed call costs the exact call plus 2 - 8 %, and the demotion (KeyIndex.MIX_FILTER_MAX_UNPROVEN) ends it
    # after one call.  16 queries: k = 10 goes to the single-launch kernel (no filtered route), k = 20 lost or drew at 65 536 keys
    # and won at 1M; nothing between 16 and 256 queries was measured.  D = 64 and banks below 65 536 keys: not measured.
    # Memory keeps the rule narrower than the clock would: the mixed call promises to stay far below a B x N score matrix (growth
    # below B * N / 2 bytes), and the filtered call brings the bank's bf16 copy (2 N D bytes) and its own workspace -- 1.1 GB at
    # 5000 x 200 000 x 256, more than twice that promise.  Kept: the measured classes whose matrix dwarfs both, banks of >= 1M keys
    # from 4096 queries; the smaller shapes that won on time stay on the exact call until the route's footprint is dealt with.
    return n_keys >= (1 << 20) and D in (128, 256) and B >= 4096


def topk_mix_rerank(sem_scores: torch.Tensor, idx: torch.Tensor, pos_q: torch.Tensor, pos_normalized: torch.Tensor,
                    w_struct: float, w_sem: float, k: int, idx_base: int = 0):
    """The canonical top-k of  w_struct * cos(position codes) + w_sem * s_sem  over the keys of canonical semantic lists
    (sem_scores, idx) [B, k'], k < k' <= 128 -- the operations of topk_cosine_mix on those keys -- and the proof that no key
    outside a list can enter or tie (ragraph_topk_mix_rerank_f32; w_sem > 0).  Returns (scores [B,k], idx [B,k], unproven_flags
    [B] int32, unproven_count [1] int32): a row whose flag is 0 holds the bits of topk_cosine_mix; a row whose flag is 1 does NOT
    and must be recomputed by it.  pos_q [B,A] raw (normalised inside), pos_normalized [N,A]; idx carries idx_base.
    No synchronisation, no read-back."""
    L = _ready()
    s = _f32c(sem_scores, "topk_mix_rerank.sem_scores")
    i = _idxc(idx, "topk_mix_rerank.idx")
    pq = _f32c(pos_q, "topk_mix_rerank.pos_q")
    pn = _f32c(pos_normalized, "topk_mix_rerank.pos_normalized")
    if s.dim() != 2 or s.shape != i.shape:
        raise RagraphNativeError(f"topk_mix_rerank: lists {tuple(s.shape)} / {tuple(i.shape)}")
    if pq.dim() != 2 or pn.dim() != 2 or pq.shape[1] != pn.shape[1] or pq.shape[0] != s.shape[0]:
        raise RagraphNativeError(f"topk_mix_rerank: codes {tuple(pq.shape)} x {tuple(pn.shape)} do not match lists {tuple(s.shape)}")
    B, kl = s.shape
    Nk, A = pn.shape
    out_s = torch.empty((B, k), dtype=torch.float32, device=s.device)
    out_i = torch.empty((B, k), dtype=torch.int64, device=s.device)
    flags = torch.empty(B, dtype=torch.int32, device=s.device)
    count = torch.zeros(1, dtype=torch.int32, device=s.device)
    if B == 0:
        return out_s, out_i, flags, count
    # (the normalised query codes: B * A floats of this call's own, exactly sized -- not the shared grow-only scratch)
    ws = torch.empty(L.ragraph_topk_mix_rerank_workspace_bytes(B, A), dtype=torch.uint8, device=s.device)
    N.check(L.ragraph_topk_mix_rerank_f32(s.data_ptr(), i.data_ptr(), B, kl, pq.data_ptr(), pn.data_ptr(), Nk, A, float(w_struct),
                                          float(w_sem), k, idx_base, out_s.data_ptr(), out_i.data_ptr(), flags.data_ptr(),
                                          count.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "topk_mix_rerank")
    return out_s, out_i, flags, count


def scatter_topk_rows_(scores: torch.Tensor, idx: torch.Tensor, pos: torch.Tensor, rows_s: torch.Tensor, rows_i: torch.Tensor):
    """scores[pos[m]] = rows_s[m], idx[pos[m]] = rows_i[m] in place (lists [B,k] f32 / i64, rows [M,k], pos [M] int64):
    ragraph_topk_rows_scatter_f32.  Returns (scores, idx)."""
    L = _ready()
    if not (scores.is_cuda and scores.is_contiguous() and scores.dtype == torch.float32 and idx.is_cuda and idx.is_contiguous()
            and idx.dtype == torch.int64 and scores.dim() == 2 and scores.shape == idx.shape):
        raise RagraphNativeError("scatter_topk_rows_: the lists must be contiguous [B,k] f32 / i64 ROCm device tensors")
    rs, ri, pos = _f32c(rows_s, "scatter_topk_rows_.rows"), _idxc(rows_i, "scatter_topk_rows_.rows"), _idxc(pos, "scatter_topk_rows_.pos")
    M = pos.numel()
    if rs.shape != (M, scores.shape[1]) or ri.shape != rs.shape:
        raise RagraphNativeError(f"scatter_topk_rows_: rows {tuple(rs.shape)} / {tuple(ri.shape)} for {M} positions of {tuple(scores.shape)}")
    if M:
        N.check(L.ragraph_topk_rows_scatter_f32(rs.data_ptr(), ri.data_ptr(), pos.data_ptr(), M, scores.shape[1], scores.shape[0],
                                                scores.data_ptr(), idx.data_ptr(), _stream()), "scatter_topk_rows_")
    return scores, idx


def keys_to_bf16(keys_normalized: torch.Tensor) -> torch.Tensor:
    """bf16 copy of the bank for topk_cosine_filtered, in MFMA fragment order (csrc/filter_common.h): rows zero-padded to
    a multiple of 256 + one row holding the largest rounding error; int16 storage, 2 D bytes per key."""
    L = _ready()
    kn = _f32c(keys_normalized, "keys_to_bf16.keys")
    rows = L.ragraph_keys_bf16_rows(kn.shape[0])
    out = torch.empty((rows, kn.shape[1]), dtype=torch.int16, device=kn.device)
    if kn.shape[0]:
        N.check(L.ragraph_keys_to_bf16(kn.data_ptr(), kn.shape[0], kn.shape[1], out.data_ptr(), _stream()), "keys_to_bf16")
    return out


def bank_copy_errors(keys_bf16: torch.Tensor, n_keys: int):
    """(max |dk| of the bf16 copy, max |dk| of the int8 copy, int8 scale) read from the copies' tail rows -- ONE
    synchronisation, for the owner of a bank version (KeyIndex) to judge once whether int8 levels suit this bank."""
    npad = -(-n_keys // 256) * 256
    t16 = keys_bf16[npad, :2].contiguous().view(torch.float32).cpu()
    t8 = keys_bf16[npad + 1 + npad // 2, :4].contiguous().view(torch.float32).cpu()
    return float(t16[0]) ** 0.5, float(t8[0]) ** 0.5, float(t8[1])


def int8_copy_classes(keys_bf16: torch.Tensor, n_keys: int) -> dict:
    """The int8 copy's two classes of granules (csrc/filter_common.h "TWO SCALES"; one synchronisation): NORMAL granules --
    32 KiB of int8 rows whose largest |k_i| is at most `cut` -- are quantised with `scale`, the HEAVY rest with
    `scale_heavy` = the bank's largest |k_i| / 127; each class has its own measured max |dk| and hence its own bound."""
    npad = -(-n_keys // 256) * 256
    row = keys_bf16[npad + 1 + npad // 2, :16].contiguous()
    f, i = row.view(torch.float32).cpu(), row.view(torch.int32).cpu()
    return {"err": float(f[0]) ** 0.5, "scale": float(f[1]), "max_abs": float(f[2]), "err_heavy": float(f[3]) ** 0.5,
            "scale_heavy": float(f[4]), "cut": float(f[5]), "heavy_granules": int(i[6]), "granules": int(i[7])}


def filtered_i8_levels(B: int, n_keys: int, D: int, k: int) -> int:
    """How many trailing levels of a filtered call of this shape run on the int8 copy (under this thread's current cap)."""
    return N.lib().ragraph_topk_cosine_filtered_i8_levels(B, n_keys, D, k)


def sharded_speculates(B: int, plan_n: int, D: int, k: int, n_shards: int) -> bool:
    """Would a sharded filtered call of this shape skip its bound pass and exchange 0 under a speculative prior?  (The same
    answer on every rank: computed from the shared plan.)"""
    return bool(N.lib().ragraph_topk_cosine_filtered_sharded_speculates(B, plan_n, D, k, n_shards))


def verify_merged_prior(merged_scores: torch.Tensor, prior, stats=None, overflow=None) -> torch.Tensor:
    """The owner's verdict on the merged lists of a sharded call (ragraph_verify_merged_prior_f32): a [5] float32 device
    tensor [missed rows, -(lowest proven k-th best), highest, candidates per query of this shard, overflowed lists]."""
    L = _ready()
    ms = _f32c(merged_scores, "verify_merged_prior.scores")
    R, k = ms.shape
    out = torch.empty(5, dtype=torch.float32, device=ms.device)
    N.check(L.ragraph_verify_merged_prior_f32(ms.data_ptr() if R else None, R, k, 0.0 if prior is None else float(prior),
                                              0 if prior is None else 1, stats.data_ptr() if stats is not None else None,
                                              overflow.data_ptr() if overflow is not None else None, out.data_ptr(), _stream()),
            "verify_merged_prior")
    return out


def set_filter_prior(theta_prior) -> float:
    """A speculative first bound for this thread's following filtered calls (None / NaN: none); returns the old one.
    ragraph_topk_cosine_filtered_set_prior: exact for any value -- queries it is too high for take the exact scan."""
    return N.lib().ragraph_topk_cosine_filtered_set_prior(float("nan") if theta_prior is None else float(theta_prior))


def set_filter_tight_prior(theta_tight) -> float:
    """A TIGHT speculative bound for this thread's following filtered calls (None / NaN: none); returns the old one.
    ragraph_topk_cosine_filtered_set_tight_prior: honoured by single-bank calls of more than 256 queries that also run under a
    prior below it -- one level from theta = tight, the queries it was too high for repaired on the device from
    max(prior, their k-th best found).  Exact for any value."""
    return N.lib().ragraph_topk_cosine_filtered_set_tight_prior(float("nan") if theta_tight is None else float(theta_tight))


def set_max_i8_levels(n: int) -> int:
    """Cap the int8 levels of this thread's following filtered calls (-1: the library's rule); returns the old cap."""
    return N.lib().ragraph_topk_cosine_filtered_max_i8_levels(int(n))


def expected_i8_candidates(B: int, n_keys: int, D: int, k: int) -> float:
    """Candidates per query the schedule's cost model expects from the int8 levels of a filtered call of this shape (under
    this thread's int8 cap): ~3.9 k (level end / previous end) per level."""
    L = N.lib()
    plan = (ctypes.c_int64 * 7)()
    if L.ragraph_topk_cosine_filtered_plan(B, n_keys, D, k, plan) <= 0:
        return 0.0
    nlev = int(plan[2])
    n_i8 = L.ragraph_topk_cosine_filtered_i8_levels(B, n_keys, D, k)
    ends = [max(int(plan[0]), 1)] + [int(plan[3 + l]) for l in range(nlev)]
    return sum(3.9 * k * ends[l + 1] / ends[l] for l in range(nlev) if l >= nlev - n_i8)


def filter_helps(B: int, n_keys: int, D: int, k: int) -> bool:
    """True when the bf16-filtered exact top-k is the faster way to the same bits.  Measured on MI355X (ms, filtered vs
    fp32 kernels, D = 256, k = 10): see DESIGN.md section 4.0 (batch-size table).  Small score matrices stay on the
    fp32 slab / tile kernels."""
    if os.environ.get("RAGRAPH_EXACT_FP32") == "1":
        return False
    if D not in (64, 128, 256) or k > 32:
        return False
    # Measured on MI355X after the round-2 kernels (ms, filtered vs the fp32 dispatch; tools/quick_topk_bench.py):
    #   N >= 65536: filtered at every batch size (1 x 65536 x 256: 0.036 vs 0.055; 64 x 65536: 0.048 vs 0.080; D = 64,
    #     16 x 65536: 0.036 vs 0.056);
    #   32768 <= N < 65536: from 128 queries (128 x 32768 x 256: 0.046 vs 0.076; 64 x 32768: 0.068 vs 0.058);
    #   8192 <= N < 32768: D >= 128 from 512 queries (512 x 10000 x 128: 0.049 vs 0.056; 1024 x 10000 x 256: 0.075 vs
    #     0.114; 256 x 10000 x 128: 0.048 vs 0.042); D = 64 from 2048 (N >= 16384: 1024 x 16384: 0.089 vs 0.085) or 8192
    #     queries (2708 x 10000 x 64: 0.155 vs 0.138; 8192 x 10000: 0.284 vs 0.418).
    if n_keys >= 65536:
        return B >= FILTER_MIN_B
    if n_keys >= 32768:
        return B >= 128
    if n_keys < 8192:
        return False
    if D >= 128:
        return B >= 512
    return B >= (2048 if n_keys >= 16384 else 8192)


FILTER_MIN_B = int(os.environ.get("RAGRAPH_FILTER_MIN_B", "1"))  # banks of >= 64 k keys: filtered from this many queries


def filter_wide_helps(B: int, n_keys: int, D: int, k: int) -> bool:
    """filter_helps for lists of 33 .. 64 keys (topk_cosine_filtered at its list width of 64): True where the filtered call is
    the faster way to the bits of topk_cosine, whose fp32 score slabs are all such a k had before.  Host arithmetic only."""
    if os.environ.get("RAGRAPH_EXACT_FP32") == "1":
        return False
    if D not in (64, 128, 256) or not 32 < k <= 64:
        return False
    # filter_helps' rule at k = 32, class by class, kept where tools/filter_wide_probe.py measured the wide call faster than the
    # slabs by more than the spread of the pair (MI355X, ms, slab vs wide at k = 33 / 41 / 64; profiles/filter_wide.txt):
    #   N >= 65536, every batch size: 100 000 x 1M x 256: 1131 vs 34.2 / 1140 vs 37.8 / 1170 vs 49.5 (k = 32 filtered: 33.6);
    #     4096 x 1M x 256: 46 vs 1.7 / 47 vs 1.8 / 48 vs 2.3;  256 x 1M: 2.42 vs 0.25 / 2.37 vs 0.28 / 2.44 vs 0.33;
    #     1 / 16 / 64 x 1M at k = 64: 0.77 vs 0.31 / 0.82 vs 0.26 / 0.89 vs 0.32;  4096 x 4M x 64: 160 vs 1.6 / 162 vs 1.7 / 168 vs 2.0;
    #     4096 x 200 000 x 128: 5.0 vs 0.46 / 5.1 vs 0.52 / 5.3 vs 0.62;  600 x 70 000 x 256: 0.49 vs 0.15 / 0.50 vs 0.18 / 0.57 vs 0.23;
    #     256 x 70 000 x 256: 0.25 vs 0.13 / 0.27 vs 0.14 / 0.33 vs 0.21;  16 x 70 000 x 64: 1.59 / 1.38 / 1.22 times faster;
    #   32768 <= N < 65536, from 128 queries: 128 x 40 000 x 256: 1.58 / 1.65 / 1.26 times faster; 2100 x 40 000: 2.39 / 2.08 / 1.99
    #     (64 x 40 000, outside the rule: 1.55 / 1.40 times faster but 0.79 at k = 64: stays out);
    #   8192 <= N < 32768: only banks of 20 000 keys up to k = 41 won -- 700 x 20 000 x 128: 1.56 / 1.55 times faster, k = 64: 0.86;
    #     2048 x 20 000 x 64: 1.09 / 1.05, k = 64: a draw -- and 10 000 keys did not: 1024 x 10 000 x 256: 1.00 / 0.89 / 0.88;
    #     8192 x 10 000 x 64: 1.00 / 0.98 / 0.97.  Nothing was measured between 10 000 and 20 000 keys or between k = 41 and 64:
    #     those stay on the slabs.
    if n_keys >= 32768:
        return filter_helps(B, n_keys, D, 32)
    if n_keys < 20000 or k > 41:
        return False
    return B >= (512 if D >= 128 else 2048)


def filter_wide128_helps(B: int, n_keys: int, D: int, k: int) -> bool:
    """filter_helps for lists of 65 .. 128 keys (topk_cosine_filtered at its list width of 128): True where the filtered call is
    the faster way to the bits of topk_cosine, whose fp32 score slabs are all such a k had before.  Host arithmetic only."""
    if os.environ.get("RAGRAPH_EXACT_FP32") == "1":
        return False
    if D not in (64, 128, 256) or not 64 < k <= 128:
        return False
    # Kept where tools/filter_wide128_probe.py measured the wide128 call faster than the slabs by more than the spread of the pair
    # (MI355X, ms per call, slab vs wide128 at k = 65 / 96 / 128; profiles/filter_wide128.txt); what was not measured stays out:
    #   N >= 1M, D >= 128, every batch size: 100 000 x 1M x 256: 1131 vs 50.0 / 1146 vs 62.4 / 1163 vs 67.4;
    #     4096 x 1M x 256: 46.9 vs 2.3 / 47.5 vs 2.5 / 48.2 vs 3.0;  256 x 1M: 6.7 - 8.7 times faster;  1 / 16 / 64 x 1M at
    #     k = 128: 1.30 / 1.46 / 2.00 times faster (k = 65: 2.24 / 2.33 / 2.84);
    #   65536 <= N < 1M, D >= 128, from 256 queries: 4096 x 200 000 x 128: 9.6 / 7.8 / 6.8 times faster; 600 x 70 000 x 256:
    #     2.37 / 1.96 / 1.71;  256 x 70 000 x 256: 1.37 / 1.20 / 1.11 (fewer queries on such a bank were not measured);
    #   D = 64: 4096 x 4M x 64: 72 / 65 / 55 times faster -- but 16 x 70 000 x 64: 0.59 / 0.58 / 0.33, and nothing between
    #     was measured: only banks of >= 4M keys from 4096 queries;
    #   32768 <= N < 65536: 2100 x 40 000 x 256: 1.16 / 1.37 / 1.11 times faster, 128 and 64 x 40 000 x 256: 0.84 - 0.51:
    #     D = 256 from 2048 queries;
    #   N < 32768: every shape lost (700 x 20 000 x 128: 0.91 / 0.57 / 0.53; 1024 x 10 000 x 256: 0.76 / 0.62 / 0.57;
    #     8192 x 10 000 x 64: 0.99 / 0.78 / 0.66; 2048 x 20 000 x 64 won by 1.05 at k = 65 alone).
    if n_keys >= 65536:
        if D == 64:
            return B >= 4096 and n_keys >= 4_000_000
        return B >= (1 if n_keys >= 1_000_000 else 256)
    if n_keys >= 32768:
        return D == 256 and B >= 2048
    return False


_EXCHANGE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int)

# Candidate statistics of a filtered call (filter_stats.py): topk_cosine_filtered(..., return_stats=True) hands the caller a
# view of THAT call's words (valid until the next filtered call on the same stream reuses the workspace); there is no
# module-level "last call" state -- another thread, stream or index would overwrite it.
FILTER_STATS = True   # (KeyIndex: this ops object supports return_stats)


def topk_cosine_filtered(q: torch.Tensor, keys_normalized: torch.Tensor, keys_bf16: torch.Tensor, k: int,
                         idx_base: int = 0, keys_packed: torch.Tensor | None = None, exchange=None, plan_n: int = 0,
                         return_stats: bool = False):
    """Exact top-k (same bits as topk_cosine) through the bf16 MFMA filter.  Returns (scores, idx, overflow): `overflow`
    is a 1-element int32 DEVICE tensor counting the queries whose candidate list overflowed (none on ordinary banks;
    all-zero queries are answered without a scan and never counted);
    the call itself recomputed those rows with an exact fp32 scan on the device, so the result is complete and nothing
    is read back: the call is asynchronous and HIP-graph capturable.  (`int(overflow)` synchronises.)
    return_stats=True: a fourth result, a [32] int32 device view of THIS call's candidate statistics (filter_stats_levels).

    Row-sharded banks: `exchange(phase, theta, scores)` is called between the phases of the call
    (ragraph_topk_cosine_filtered_sharded_f32) with theta [B] = this shard's lower bound of every query's final k-th
    best score and scores [B,k] = its running top-k; it sharpens theta in place across the shards.  `plan_n` = the
    largest shard's size (the same schedule, hence the same collectives, on every rank).  At phase 0 `scores` holds k
    lower bounds of distinct keys' exact scores (the bound pass's group maxima minus eps, or an exact level 0's top-k):
    an exchange that pools them across the shards announces the shard count as `exchange.n_shards` (default 1), and
    every shard then scans 1 / n_shards of the first sample.  The result is then the shard's list of what can still be
    in the global top-k (padded with -inf / INT64_MAX), to be merged by topk_merge."""
    L = _ready()
    q = _f32c(q, "topk_cosine_filtered.q")
    kn = _f32c(keys_normalized, "topk_cosine_filtered.keys")
    B, D = q.shape
    Nk = kn.shape[0]
    if keys_bf16.dtype != torch.int16 or not keys_bf16.is_contiguous() or keys_bf16.shape[1] != D or \
            keys_bf16.shape[0] != L.ragraph_keys_bf16_rows(Nk):
        raise RagraphNativeError("topk_cosine_filtered: keys_bf16 must come from keys_to_bf16(keys_normalized)")
    kp = 0
    if keys_packed is not None:
        kpt = _f32c(keys_packed, "topk_cosine_filtered.keys_packed")
        if kpt.shape != kn.shape:
            raise RagraphNativeError("topk_cosine_filtered: keys_packed shape mismatch")
        kp = kpt.data_ptr()
    scores = torch.empty((B, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((B, k), dtype=torch.int64, device=q.device)
    overflow = torch.empty(1, dtype=torch.int32, device=q.device)
    if exchange is None:   # (every k up to TOPK_FILTER_MAX: the entry picks its list width)
        nbytes = L.ragraph_topk_cosine_filtered_workspace_bytes(B, max(plan_n, Nk), D, k)
    else:  # (the sharded schedule -- planned for (plan_n, n_shards) -- can need another level-0 scratch; k <= 32: the entry refuses more)
        nbytes = L.ragraph_topk_cosine_filtered_sharded_workspace_bytes(B, max(plan_n, Nk), D, k,
                                                                        int(getattr(exchange, "n_shards", 1)))
    if nbytes == 0:
        raise RagraphNativeError(f"topk_cosine_filtered: unsupported shape B={B} N={Nk} D={D} k={k}")
    ws = _workspace(nbytes, q.device)
    off = L.ragraph_topk_cosine_filtered_stats_offset(ws.numel())
    stats = ws[off:off + 128].view(torch.int32)   # (32 words; valid until the next filtered call on this stream)
    if exchange is None:
        N.check(L.ragraph_topk_cosine_filtered_f32(q.data_ptr(), B, kn.data_ptr(), kp, keys_bf16.data_ptr(), Nk, D, k, idx_base,
                                                   scores.data_ptr(), idx.data_ptr(), overflow.data_ptr(), None, ws.data_ptr(),
                                                   ws.numel(), _stream()),
                "topk_cosine_filtered")
        return (scores, idx, overflow, stats) if return_stats else (scores, idx, overflow)
    theta = torch.empty(B, dtype=torch.float32, device=q.device)
    errors = []

    def _cb(_ctx, phase):  # runs on this thread, between the call's launches
        try:
            exchange(int(phase), theta, scores)
        except BaseException as e:  # (an exception must not unwind through the C frames)
            errors.append(e)

    cb = _EXCHANGE_FN(_cb)
    rc = L.ragraph_topk_cosine_filtered_sharded_f32(q.data_ptr(), B, kn.data_ptr(), kp, keys_bf16.data_ptr(), Nk, D, k,
                                                    idx_base, scores.data_ptr(), idx.data_ptr(), overflow.data_ptr(), None,
                                                    ws.data_ptr(), ws.numel(), _stream(), max(plan_n, Nk),
                                                    theta.data_ptr(), cb, None, int(getattr(exchange, "n_shards", 1)))
    if errors:
        raise errors[0]
    N.check(rc, "topk_cosine_filtered(sharded)")
    return (scores, idx, overflow, stats) if return_stats else (scores, idx, overflow)


def fused_helps(B: int, n_keys: int, D: int, k: int) -> bool:
    """True when the single-launch small-bank kernel (csrc/topk_fused.hip) is the fastest way to the exact top-k.  Its time
    is nearly flat in the batch size (38 - 95 us: a chain of per-workgroup phases, every tile streaming the L2-resident
    bf16 copy), while the score-slab / fp32 paths that small banks otherwise take grow with B.  Measured on MI355X
    (us, this kernel vs the dispatch without it; tools/quick_fused_bench.py, profiles/r3_fused_sweep.txt):
      8192 x 2000 x 64: 38 vs 136;  8192 x 5000 x 128: 76 vs 210;  8192 x 5000 x 256: 135 vs 290;  2708 x 5000 x 64: 69 vs 89;
      2708 x 20000 x 64: 83 vs 120;  1024 x 20000 x 64: 68 vs 92;  2708 x 5000 x 256: 96 vs 140;
      not: 1024 x 5000 x 128: 63 vs 52;  256 x 2000 x 64: 38 vs 25;  and banks of >= 8192 keys at D >= 128, where the
      multi-launch filtered path is as fast (2708 x 10000 x 128 -- BASELINE config 1 -- 89 vs 87; 8192 x 10000 x 128: 105 vs 107)."""
    if os.environ.get("RAGRAPH_EXACT_FP32") == "1" or os.environ.get("RAGRAPH_TOPK_FUSED", "1") == "0":
        return False
    if D not in (64, 128, 256) or k > 16 or n_keys < 128 * k:
        return False
    if 2 * n_keys * D > FUSED_MAX_COPY_BYTES or (D >= 128 and n_keys >= 8192):
        return False
    return B * n_keys >= FUSED_MIN_SCORES


FUSED_MAX_COPY_BYTES = int(os.environ.get("RAGRAPH_FUSED_MAX_COPY", str(3 << 20)))
FUSED_MIN_SCORES = int(os.environ.get("RAGRAPH_FUSED_MIN_SCORES", "12000000"))


_fused_tickets: dict = {}


def _tickets(n: int, device) -> torch.Tensor:
    """The fused kernel's per-tile tickets: zero before the first call, left zero by every call; one buffer per
    (device, stream) -- calls on a stream are ordered."""
    dev = device.index if device.index is not None else torch.cuda.current_device()
    key = (dev, _raw_stream(dev) if _raw_stream is not None else torch.cuda.current_stream(dev).cuda_stream)
    t = _fused_tickets.get(key)
    if t is None or t.numel() < n:
        t = torch.zeros(max(n, 1024), dtype=torch.int32, device=device)
        _fused_tickets[key] = t
    return t


def topk_cosine_fused(q: torch.Tensor, keys_normalized: torch.Tensor, keys_bf16: torch.Tensor, k: int, idx_base: int = 0):
    """Exact top-k (same bits as topk_cosine) in ONE launch: small banks (ragraph_topk_cosine_fused_f32)."""
    L = _ready()
    q = _f32c(q, "topk_cosine_fused.q")
    kn = _f32c(keys_normalized, "topk_cosine_fused.keys")
    B, D = q.shape
    Nk = kn.shape[0]
    if keys_bf16.dtype != torch.int16 or not keys_bf16.is_contiguous() or keys_bf16.shape[1] != D or \
            keys_bf16.shape[0] != L.ragraph_keys_bf16_rows(Nk):
        raise RagraphNativeError("topk_cosine_fused: keys_bf16 must come from keys_to_bf16(keys_normalized)")
    scores = torch.empty((B, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((B, k), dtype=torch.int64, device=q.device)
    if B:
        nbytes = L.ragraph_topk_cosine_fused_workspace_bytes(B, Nk, D, k)
        if nbytes == 0:
            raise RagraphNativeError(f"topk_cosine_fused: unsupported shape B={B} N={Nk} D={D} k={k}")
        ws = _workspace(nbytes, q.device)
        N.check(L.ragraph_topk_cosine_fused_f32(q.data_ptr(), B, kn.data_ptr(), keys_bf16.data_ptr(), Nk, D, k, idx_base,
                                                scores.data_ptr(), idx.data_ptr(), _tickets((B + 31) // 32, q.device).data_ptr(),
                                                ws.data_ptr(), ws.numel(), _stream()), "topk_cosine_fused")
    return scores, idx


SMALL_MAX_B = 16   # (the kernel takes up to 32; measured against the four-launch call on the 1M x 256 bank, ms: 1 query 0.067 vs
                   # 0.093, 8: 0.073 vs 0.097, 16: 0.087 vs 0.094, 24: 0.104 vs 0.100, 32: 0.113 vs 0.096 -- profiles/r4_small_ab.txt)


def small_helps(B: int, n_keys: int, D: int, k: int) -> bool:
    """True when the single-launch kernel for a handful of queries against a large bank (csrc/topk_small.hip) is the way
    to the exact top-k: up to 16 queries, banks the filtered path takes at any batch size (>= 65536 keys).  Measured on
    MI355X, 1M x 256 bank, k = 10 (ms per call, this kernel vs the four-launch filtered call): DESIGN.md section 4.0c."""
    if os.environ.get("RAGRAPH_EXACT_FP32") == "1" or os.environ.get("RAGRAPH_TOPK_SMALL", "1") == "0":
        return False
    return 1 <= B <= SMALL_MAX_B and D in (64, 128, 256) and k <= 32 and 65536 <= n_keys < 2 ** 31


_small_state: dict = {}   # insertion-ordered: least recently used first
_small_state_pinned: set = set()   # keys whose buffer a captured HIP graph replays against
_SMALL_STATE_MAX = 8


def _small_state_buf(device, create: bool = True):
    """The single-launch kernel's state words: zero before the first call, left zero by every call; one buffer per
    (device, stream) -- calls on a stream are ordered.  Never ALLOCATED while a HIP graph is being captured (the buffer
    would come from the capture's private pool and be reused by later eager calls on a recycled stream handle): returns
    None then, and the caller takes another path (small_helps_now).  The cache is bounded like the workspace cache -- except that a
    buffer handed out DURING a capture stays for good: the graph replays against its address, and the kernel both reads it as
    zeros and zeroes it on exit."""
    dev = device.index if device.index is not None else torch.cuda.current_device()
    key = (dev, _raw_stream(dev) if _raw_stream is not None else torch.cuda.current_stream(dev).cuda_stream)
    t = _small_state.pop(key, None)
    if t is None:
        if not create or torch.cuda.is_current_stream_capturing():
            return None
        t = torch.zeros(N.lib().ragraph_topk_cosine_small_state_bytes() // 4, dtype=torch.int32, device=device)
    _small_state[key] = t
    if torch.cuda.is_current_stream_capturing():
        _small_state_pinned.add(key)   # a captured graph holds the RAW address: this buffer is never evicted (a few KB)
    for old_key in [k_ for k_ in _small_state if k_ not in _small_state_pinned][:-_SMALL_STATE_MAX]:
        _small_state.pop(old_key)      # least recently used first; pinned entries do not count against the bound
    return t


def small_state_ready(device) -> bool:
    """May the single-launch kernel run on the current stream right now?  (Always outside a capture; inside one only when
    the stream's state buffer already exists -- e.g. from the warm-up runs every capture is preceded by.)"""
    return _small_state_buf(device) is not None


def topk_cosine_small(q: torch.Tensor, keys_normalized: torch.Tensor, keys_bf16: torch.Tensor, k: int, idx_base: int = 0,
                      return_stats: bool = False):
    """Exact top-k (same bits as topk_cosine) of up to 32 queries in ONE launch (ragraph_topk_cosine_small_f32).  Returns
    (scores, idx, overflow): overflow = 1-element int32 device tensor, the queries answered by an exact scan.  Under this
    thread's speculative first bound (set_filter_prior) the launch has no bound phase and a second, normally empty launch
    scans for the queries the prior was too high for.  return_stats=True: + a [32] int32 view of the call's statistics words
    (filter_stats.py: SPECULATIVE, SPEC_FAILED, KTH_LO / KTH_HI -- smallest / largest k-th best score, through ord2f)."""
    L = _ready()
    q = _f32c(q, "topk_cosine_small.q")
    kn = _f32c(keys_normalized, "topk_cosine_small.keys")
    B, D = q.shape
    Nk = kn.shape[0]
    if keys_bf16.dtype != torch.int16 or not keys_bf16.is_contiguous() or keys_bf16.shape[1] != D or \
            keys_bf16.shape[0] != L.ragraph_keys_bf16_rows(Nk):
        raise RagraphNativeError("topk_cosine_small: keys_bf16 must come from keys_to_bf16(keys_normalized)")
    scores = torch.empty((B, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((B, k), dtype=torch.int64, device=q.device)
    overflow = torch.empty(1, dtype=torch.int32, device=q.device)
    nbytes = L.ragraph_topk_cosine_small_workspace_bytes(B, D, k)
    if nbytes == 0:
        raise RagraphNativeError(f"topk_cosine_small: unsupported shape B={B} N={Nk} D={D} k={k}")
    ws = _workspace(nbytes, q.device)
    state = _small_state_buf(q.device)
    if state is None:
        raise RagraphNativeError("topk_cosine_small: no state buffer for this stream yet and a HIP graph is being captured "
                                 "(run the call once on this stream before capturing, or take topk_cosine_filtered)")
    rc = L.ragraph_topk_cosine_small_f32(q.data_ptr(), B, kn.data_ptr(), keys_bf16.data_ptr(), Nk, D, k, idx_base,
                                         scores.data_ptr(), idx.data_ptr(), overflow.data_ptr(), state.data_ptr(), ws.data_ptr(),
                                         ws.numel(), _stream())
    if rc != 0:   # (a launch that did not happen leaves the words as they were; after any error: zero them again)
        state.zero_()
    N.check(rc, "topk_cosine_small")
    if return_stats:
        return scores, idx, overflow, ws[nbytes - 128:nbytes].view(torch.int32)   # (the workspace's last 128 bytes)
    return scores, idx, overflow


def theta_sharpen(gathered: torch.Tensor, theta: torch.Tensor, k: int) -> torch.Tensor:
    """In place: theta[b] = max(theta[b], k-th largest of gathered[:, b, :]) -- the per-level exchange of a filtered
    retrieval over a row-sharded bank (gathered = all_gather of every shard's best m exact scores, [G, B, m])."""
    L = _ready()
    g = _f32c(gathered, "theta_sharpen.gathered")
    G, B, m = g.shape
    if theta.dtype != torch.float32 or not theta.is_contiguous() or theta.numel() != B:
        raise RagraphNativeError("theta_sharpen: theta must be a contiguous fp32 [B] tensor")
    N.check(L.ragraph_theta_sharpen_f32(g.data_ptr(), G, B, m, k, theta.data_ptr(), _stream()), "theta_sharpen")
    return theta


from .kernels_index import KeyIndex  # noqa: E402,F401  (bank copies + dispatch to the fastest exact top-k)


def topk_merge(scores: torch.Tensor, idx: torch.Tensor):
    """[G,B,k] per-shard lists -> canonical [B,k]."""
    L = _ready()
    scores = _f32c(scores, "topk_merge.scores")
    idx = _idxc(idx, "topk_merge.idx")
    G, B, k = scores.shape
    out_s = torch.empty((B, k), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((B, k), dtype=torch.int64, device=scores.device)
    N.check(L.ragraph_topk_merge_f32(scores.data_ptr(), idx.data_ptr(), G, B, k, out_s.data_ptr(), out_i.data_ptr(),
                                     _stream()), "topk_merge")
    return out_s, out_i


TOPK_TAIL_MAX = N.TOPK_TAIL_MAX   # rows one topk_cosine_tail call takes (RAGRAPH_TOPK_TAIL_MAX)


def topk_cosine_tail(q: torch.Tensor, keys_tail: torch.Tensor, seed_scores: torch.Tensor, seed_idx: torch.Tensor,
                     idx_base_tail: int):
    """The canonical top-k of a finished list and more keys: `seed_scores` / `seed_idx` [B, k] is the canonical list of a
    search over other rows (all indices below idx_base_tail; its end may be -inf / INT64_MAX padding), `keys_tail` [T, D] rows
    from normalize_rows() appended behind them (row j carries index idx_base_tail + j), `q` the RAW queries of the seed's
    search.  Returns (scores, idx) [B, k]: the bits of one search over all rows (ragraph_topk_cosine_tail_f32: one launch, a
    memset node in front of it when a long tail under few queries is cut into slices).  D in {64, 128, 256}, k <= TOPK_MAX,
    1 <= T <= TOPK_TAIL_MAX; T < k is fine."""
    L = _ready()
    q = _f32c(q, "topk_cosine_tail.q")
    kt = _f32c(keys_tail, "topk_cosine_tail.keys_tail")
    ss = _f32c(seed_scores, "topk_cosine_tail.seed_scores")
    si = _idxc(seed_idx, "topk_cosine_tail.seed_idx")
    if q.dim() != 2 or kt.dim() != 2 or q.shape[1] != kt.shape[1]:
        raise RagraphNativeError(f"topk_cosine_tail: bad shapes {tuple(q.shape)} x {tuple(kt.shape)}")
    if ss.dim() != 2 or ss.shape != si.shape or ss.shape[0] != q.shape[0]:
        raise RagraphNativeError(f"topk_cosine_tail: seed {tuple(ss.shape)} / {tuple(si.shape)} for {q.shape[0]} queries")
    B, D = q.shape
    T, k = kt.shape[0], ss.shape[1]
    scores = torch.empty((B, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((B, k), dtype=torch.int64, device=q.device)
    if B == 0:
        return scores, idx
    # (+ 4096: the statistics words of a filtered call sit in the LAST bytes of the shared workspace and are read back after the fact)
    ws = _workspace(L.ragraph_topk_cosine_tail_workspace_bytes(B, T, D, k) + 4096, q.device)
    N.check(L.ragraph_topk_cosine_tail_f32(q.data_ptr(), B, kt.data_ptr(), T, D, k, idx_base_tail, ss.data_ptr(), si.data_ptr(),
                                           scores.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel() - 4096, _stream()),
            "topk_cosine_tail")
    return scores, idx


TOPK_ORDERED_MAX = N.TOPK_ORDERED_MAX   # the longest ordered list (RAGRAPH_TOPK_ORDERED_MAX)


def retired_bitmap(n_rows: int, device) -> torch.Tensor:
    """A zeroed bitmap over n_rows physical rows (int32 storage of 32-bit words: bit r & 31 of word r >> 5)."""
    return torch.zeros(max(-(-n_rows // 32), 1), dtype=torch.int32, device=device)


def retire_rows(bitmap: torch.Tensor, rows: torch.Tensor, n_rows: int) -> torch.Tensor:
    """Set the bits of the physical rows `rows` (int64 ids; duplicates and bits already set are fine, an id outside
    [0, n_rows) sets nothing) in `bitmap`, in place (ragraph_rows_retire_u32).  No synchronisation."""
    L = _ready()
    rows = _idxc(rows, "retire_rows.rows").reshape(-1)
    if not isinstance(bitmap, torch.Tensor) or not bitmap.is_cuda or bitmap.dtype != torch.int32 or not bitmap.is_contiguous() \
            or bitmap.numel() * 32 < n_rows:
        raise RagraphNativeError(f"retire_rows: the bitmap must be a contiguous int32 ROCm device tensor of at least {-(-n_rows // 32)} words")
    N.check(L.ragraph_rows_retire_u32(rows.data_ptr() if rows.numel() else None, rows.numel(), n_rows, bitmap.data_ptr(), _stream()),
            "retire_rows")
    return bitmap


def topk_drop_rows(scores: torch.Tensor, idx: torch.Tensor, bitmap: torch.Tensor, n_rows: int, k_out: int, idx_base: int = 0):
    """Canonical lists [B, k_in] without their retired rows: per list the entries whose row idx - idx_base has its bit clear in
    `bitmap` (retired_bitmap / retire_rows), in order, the first k_out of them -- the canonical top-k_out of the live rows when
    the lists are the canonical top-k_in of all n_rows rows and at most k_in - k_out rows are retired.  Returns (scores, idx)
    [B, k_out] and `short_lists`, a device int32 word: the lists that held fewer than k_out live entries (padded with -inf /
    INT64_MAX).  One launch behind the word's memset (ragraph_topk_drop_rows_f32); no synchronisation, capturable."""
    L = _ready()
    s = _f32c(scores, "topk_drop_rows.scores")
    i = _idxc(idx, "topk_drop_rows.idx")
    if s.dim() != 2 or s.shape != i.shape:
        raise RagraphNativeError(f"topk_drop_rows: lists {tuple(s.shape)} / {tuple(i.shape)}")
    if not isinstance(bitmap, torch.Tensor) or not bitmap.is_cuda or bitmap.dtype != torch.int32 or not bitmap.is_contiguous() \
            or bitmap.numel() * 32 < n_rows:
        raise RagraphNativeError(f"topk_drop_rows: the bitmap must be a contiguous int32 ROCm device tensor of at least {-(-n_rows // 32)} words")
    B, k_in = s.shape
    out_s = torch.empty((B, k_out), dtype=torch.float32, device=s.device)
    out_i = torch.empty((B, k_out), dtype=torch.int64, device=s.device)
    short = torch.zeros(1, dtype=torch.int32, device=s.device)
    if B == 0:
        return out_s, out_i, short
    N.check(L.ragraph_topk_drop_rows_f32(s.data_ptr(), i.data_ptr(), B, k_in, idx_base, bitmap.data_ptr(), n_rows, k_out,
                                         out_s.data_ptr(), out_i.data_ptr(), short.data_ptr(), _stream()), "topk_drop_rows")
    return out_s, out_i, short


def dedup_rows(keys_normalized: torch.Tensor):
    """Groups of bit-identical bank rows (ragraph_dedup_rows_f32; the reference's bank recipe stores most rows several
    hundred thousand times over, ToyGraphBase.py:91-119 + Augmentation.py:9-20).  Returns (U, largest group, uniq_row [U]
    int64 = every group's lowest row, ascending; group_ptr [U+1] int32; members [N] int32 = the groups' rows, ascending).
    Reads the two counts back: ONE synchronisation, for the owner of a bank version (KeyIndex)."""
    L = _ready()
    kn = _f32c(keys_normalized, "dedup_rows.keys")
    Nk, D = kn.shape
    dev = kn.device
    stats = torch.empty(2, dtype=torch.int64, device=dev)
    uniq_row = torch.empty(Nk, dtype=torch.int64, device=dev)
    group_ptr = torch.empty(Nk + 1, dtype=torch.int32, device=dev)
    members = torch.empty(Nk, dtype=torch.int32, device=dev)
    nbytes = L.ragraph_dedup_rows_workspace_bytes(Nk)
    if nbytes == 0:
        raise RagraphNativeError(f"dedup_rows: unsupported bank of {Nk} rows")
    ws = _workspace(nbytes, dev)
    N.check(L.ragraph_dedup_rows_f32(kn.data_ptr(), Nk, D, stats.data_ptr(), uniq_row.data_ptr(), group_ptr.data_ptr(),
                                     members.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "dedup_rows")
    U, largest = (int(x) for x in stats.tolist())
    return U, largest, uniq_row[:U], group_ptr[:U + 1], members


def topk_expand_groups(scores_u: torch.Tensor, idx_u: torch.Tensor, group_ptr: torch.Tensor, members: torch.Tensor, k: int,
                       idx_base: int = 0, idx_base_u: int = 0):
    """Canonical top-k of a bank from the canonical top-ku of its unique rows (dedup_rows): [B,ku] -> [B,k], same bits
    as the search over every row (ragraph_topk_expand_groups_f32)."""
    L = _ready()
    su = _f32c(scores_u, "topk_expand_groups.scores")
    iu = _idxc(idx_u, "topk_expand_groups.idx")
    B, ku = su.shape
    out_s = torch.empty((B, k), dtype=torch.float32, device=su.device)
    out_i = torch.empty((B, k), dtype=torch.int64, device=su.device)
    N.check(L.ragraph_topk_expand_groups_f32(su.data_ptr(), iu.data_ptr(), ku, idx_base_u, group_ptr.data_ptr(),
                                             members.data_ptr(), group_ptr.numel() - 1, B, k, idx_base, out_s.data_ptr(),
                                             out_i.data_ptr(), _stream()), "topk_expand_groups")
    return out_s, out_i


def gather_rows(v: torch.Tensor, idx: torch.Tensor, idx_base: int = 0) -> torch.Tensor:
    """v[idx] -- ToyGraphBase.py:70-71.  Rows outside [idx_base, idx_base+N) come back as zeros."""
    L = _ready()
    v = _f32c(v, "gather_rows.v")
    idx = _idxc(idx, "gather_rows.idx")
    out = torch.empty(tuple(idx.shape) + (v.shape[1],), dtype=torch.float32, device=v.device)
    if idx.numel() == 0:      # (an empty tensor has no address to hand over)
        return out
    N.check(L.ragraph_gather_rows_f32(v.data_ptr(), v.shape[0], v.shape[1], idx.data_ptr(), idx.numel(), idx_base,
                                      out.data_ptr(), _stream()), "gather_rows")
    return out


def gather_reduce(v: torch.Tensor, labels: torch.Tensor | None, idx: torch.Tensor, idx_base: int = 0,
                  v_scale: float = 1.0):
    """(v_scale * sum_k v[idx], mean_k labels[idx]) -- RAGraph.py:48-49; edge modules/RAGraph.py:321 (v_scale=1/k)."""
    L = _ready()
    v = _f32c(v, "gather_reduce.v")
    idx = _idxc(idx, "gather_reduce.idx")
    B, k = idx.shape
    sum_v = torch.empty((B, v.shape[1]), dtype=torch.float32, device=v.device)
    mean_l = None
    C = 0
    if labels is not None:
        labels = _f32c(labels, "gather_reduce.labels")
        C = labels.shape[1]
        mean_l = torch.empty((B, C), dtype=torch.float32, device=v.device)
    N.check(L.ragraph_gather_reduce_f32(v.data_ptr(), v.shape[1], _ptr(labels), C, v.shape[0], idx.data_ptr(), B, k,
                                        idx_base, float(v_scale), sum_v.data_ptr(), _ptr(mean_l), _stream()),
            "gather_reduce")
    return sum_v, mean_l


def gather_reduce_mix(v: torch.Tensor, labels: torch.Tensor | None, idx: torch.Tensor, a: torch.Tensor, wa: float, wb: float,
                      idx_base: int = 0, v_scale: float = 1.0):
    """(a * wa + (v_scale * sum_k v[idx]) * wb, mean_k labels[idx]) -- RAGraph.py:48-49 + :53 in one launch: the bits of
    gather_reduce followed by axpby(a, wa, sum, wb), without the sum in memory."""
    L = _ready()
    v = _f32c(v, "gather_reduce_mix.v")
    idx = _idxc(idx, "gather_reduce_mix.idx")
    a = _f32c(a, "gather_reduce_mix.a")
    B, k = idx.shape
    if tuple(a.shape) != (B, v.shape[1]):
        raise RagraphNativeError(f"gather_reduce_mix: a is {tuple(a.shape)}, the reduction [{B}, {v.shape[1]}]")
    out = torch.empty((B, v.shape[1]), dtype=torch.float32, device=v.device)
    mean_l = None
    C = 0
    if labels is not None:
        labels = _f32c(labels, "gather_reduce_mix.labels")
        C = labels.shape[1]
        mean_l = torch.empty((B, C), dtype=torch.float32, device=v.device)
    N.check(L.ragraph_gather_reduce_mix_f32(v.data_ptr(), v.shape[1], _ptr(labels), C, v.shape[0], idx.data_ptr(), B, k, idx_base,
                                            float(v_scale), a.data_ptr(), float(wa), float(wb), out.data_ptr(), _ptr(mean_l),
                                            _stream()), "gather_reduce_mix")
    return out, mean_l


def linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, act: int = ACT_NONE,
           alpha: float = 0.0) -> torch.Tensor:
    """act(x @ weight.T + bias) -- layers/gcn.py:32, TaskDecoder.py:15-16."""
    L = _ready()
    x = _f32c(x, "linear.x")
    w = _f32c(weight, "linear.weight")
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    if w.dim() != 2 or w.shape[1] != x2.shape[1]:
        raise RagraphNativeError(f"linear: bad shapes {tuple(x.shape)} x {tuple(w.shape)}")
    b = None if bias is None else _f32c(bias, "linear.bias")
    y = torch.empty((x2.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
    if x2.shape[0] > 0:
        N.check(L.ragraph_linear_f32(x2.data_ptr(), x2.shape[0], x2.shape[1], w.data_ptr(), w.shape[0], _ptr(b), act,
                                     float(alpha), y.data_ptr(), _stream()), "linear")
    return y.reshape(tuple(lead) + (w.shape[0],))


LINEAR_VARIANTS = {LINEAR_GENERIC: "generic", LINEAR_SMALL: "small", LINEAR_TILE: "tile", LINEAR_STREAM: "stream",
                   LINEAR_NARROW: "narrow"}
LinearPlan = collections.namedtuple("LinearPlan", "variant grid_x grid_y steps")


def linear_plan(M: int, K: int, N_: int, x_aligned: bool = True, w_aligned: bool = True) -> LinearPlan:
    """The kernel `linear` runs for x [M, K] against weight [N_, K], and its launch (ragraph_linear_plan: host arithmetic, no
    device needed; the dispatcher takes its decision from the same function).  variant: one of LINEAR_* (names in
    LINEAR_VARIANTS); grid_x, grid_y; steps: the stages per workgroup of the streaming kernel, else the 32-wide K chunks.
    x_aligned / w_aligned: whether the operand starts on a 16-byte boundary (data_ptr() % 16 == 0)."""
    plan = (ctypes.c_int64 * 4)()
    N.check(N.lib().ragraph_linear_plan(M, K, N_, int(bool(x_aligned)), int(bool(w_aligned)), plan), "linear_plan")
    return LinearPlan(*(int(v) for v in plan))


def linear_tn(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a^T @ b for tall row-major operands: a [n, M], b [n, N] -> [M, N] (ragraph_linear_tn_f32: the weight gradient of a
    dense layer without transposed copies, the rows cut into ranges summed in order -- deterministic)."""
    L = _ready()
    a, b = _f32c(a, "linear_tn.a"), _f32c(b, "linear_tn.b")
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0]:
        raise RagraphNativeError(f"linear_tn: bad shapes {tuple(a.shape)} / {tuple(b.shape)}")
    n, M, Nn = a.shape[0], a.shape[1], b.shape[1]
    out = torch.empty((M, Nn), dtype=torch.float32, device=a.device)
    if n == 0:
        return out.zero_()
    ws = _workspace(L.ragraph_linear_tn_workspace_bytes(n, M, Nn), a.device)
    N.check(L.ragraph_linear_tn_f32(a.data_ptr(), b.data_ptr(), n, M, Nn, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
            "linear_tn")
    return out


def column_sums(x: torch.Tensor) -> torch.Tensor:
    """Sum over the rows of x [n, D] -> [D] (a bias gradient): ranges of COLSUM_ROWS rows summed sequentially by one lane
    group each (ragraph_segment_reduce_f32), then the range sums in order -- deterministic, and chip-wide where one segment
    of 100 000 rows was one workgroup's 7.5-ms chain."""
    x = _f32c(x, "column_sums.x")
    n = x.shape[0]
    if n <= COLSUM_SINGLE_MAX:   # (a batch of a few hundred nodes: one launch beats ranges + their pointer bookkeeping)
        return segment_reduce(x, _whole_segment(n, x.device)).reshape(-1)
    ptr = torch.arange(0, n + COLSUM_ROWS, COLSUM_ROWS, dtype=torch.int64, device=x.device).clamp_(max=n)
    part = segment_reduce(x, ptr)
    return segment_reduce(part, _whole_segment(part.shape[0], x.device)).reshape(-1)


_whole_seg: dict = {}


def _whole_segment(n: int, device) -> torch.Tensor:
    """The segment pointer [0, n] on `device`, made once per (device, n) and kept for the life of the process: a host list
    copied to the device is a synchronising copy, which a HIP graph capture (ragraph_amd.capture.CapturedTrainStep) does
    not allow, and a captured graph keeps reading the entry's address -- so entries are never dropped (16 bytes each, one
    per distinct row count).  Read-only."""
    key = (torch.device(device), n)
    t = _whole_seg.get(key)
    if t is None:
        t = _whole_seg[key] = torch.tensor([0, n], dtype=torch.int64, device=device)
    return t


COLSUM_ROWS = 256
COLSUM_SINGLE_MAX = 2048
LINEAR_TN_MIN_ROWS = 2048   # below: gY^T X through the dense kernel on transposed copies (tiny copies, no range sums)

ROW_BLOCK = 4096  # rows / segments longer than this are summed in blocks (csrc/sparse.hip, oracle ORACLE_ROW_BLOCK)


def _csr_args(who: str, rowptr, col, val, x):
    """The CSR operands of an SpMM wrapper in the dtypes the library takes, with n, D and nnz."""
    rowptr = _idxc(rowptr, f"{who}.rowptr")
    col = _idxc(col, f"{who}.col", torch.int32)
    val = _f32c(val, f"{who}.val")
    x = _f32c(x, f"{who}.x")
    return rowptr, col, val, x, rowptr.numel() - 1, x.shape[1], col.numel()


def _hub_workspace(long_rows: bool, nnz: int, D: int, device):
    """(pointer, bytes) of the hub-row workspace of the full product (D = 0: of the softmax); (None, 0) without long rows --
    the `_ws` entries then leave a hub row to its own lanes, which is all the entries without a workspace do."""
    if not long_rows:
        return None, 0
    ws = _workspace(_ready().ragraph_sparse_workspace_bytes(nnz, D), device)
    return ws.data_ptr(), ws.numel()


def spmm_csr(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, x: torch.Tensor,
             bias: torch.Tensor | None = None, act: int = ACT_NONE, alpha: float = 0.0, beta: float = 0.0,
             y_in: torch.Tensor | None = None, long_rows: bool = False) -> torch.Tensor:
    """act(A @ x + bias) + beta*y_in for CSR A -- layers/gcn.py:36-40, Propagation.py:22-25, edge _agg.
    `long_rows`: the graph has rows of more than ROW_BLOCK edges (CSRGraph.has_long_rows): their blocks are spread over
    the chip through a workspace -- same bits, three more launches."""
    L = _ready()
    rowptr, col, val, x, n, D, nnz = _csr_args("spmm_csr", rowptr, col, val, x)
    b = None if bias is None else _f32c(bias, "spmm_csr.bias")
    yi = None if y_in is None else _f32c(y_in, "spmm_csr.y_in")
    y = torch.empty((n, D), dtype=torch.float32, device=x.device)
    ws, ws_bytes = _hub_workspace(long_rows, nnz, D, x.device)
    N.check(L.ragraph_spmm_csr_ws_f32(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), n, x.data_ptr(), D, _ptr(b), act,
                                      float(alpha), float(beta), _ptr(yi), y.data_ptr(), nnz if long_rows else 0, ws,
                                      ws_bytes, _stream()), "spmm_csr")
    return y


def spmm_csr_rows(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, x: torch.Tensor, rows: torch.Tensor,
                  long_rows: bool = False) -> torch.Tensor:
    """(A @ x)[rows] without the other rows (ragraph_spmm_csr_rows_f32) -- the last propagation layer of the edge flavour's
    training step at the batch's rows, modules/RAGraph.py:232-240,327,343-345.  rows: int64 ids, any order, repeats allowed;
    returns [R, D], bit-identical to spmm_csr(...)[rows].  `long_rows`: as spmm_csr (the blocks of requested hub rows are
    spread over the chip through a workspace)."""
    L = _ready()
    rowptr, col, val, x, n, D, nnz = _csr_args("spmm_csr_rows", rowptr, col, val, x)
    rows = _idxc(rows, "spmm_csr_rows.rows").reshape(-1)
    R = rows.numel()
    y = torch.empty((R, D), dtype=torch.float32, device=x.device)
    ws = None
    if long_rows:
        nbytes = L.ragraph_spmm_csr_rows_workspace_bytes(nnz, R, D)
        if nbytes == 0:
            raise RagraphNativeError(f"spmm_csr_rows: unsupported sizes (nnz={nnz}, R={R}, D={D})")
        ws = _workspace(nbytes, x.device)
    N.check(L.ragraph_spmm_csr_rows_f32(rowptr.data_ptr(), _ptr(col) if nnz else None, _ptr(val) if nnz else None, n,
                                        x.data_ptr(), D, rows.data_ptr() if R else None, R, y.data_ptr(), nnz, _ptr(ws),
                                        0 if ws is None else ws.numel(), _stream()), "spmm_csr_rows")
    return y


def csr_rows_edges(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, rows: torch.Tensor):
    """The edges of the rows `rows` of a CSR matrix as COO (col int64 [E], r int64 [E] = the POSITION in `rows`, val [E]):
    ascending r, CSR order inside a row (ragraph_csr_rows_offsets_i64 on the library's own prefix sums, then
    ragraph_csr_rows_edges_f32) -- what the backward of spmm_csr_rows multiplies by.  Reads the edge count back (one
    synchronisation: it sizes the result)."""
    L = _ready()
    rowptr = _idxc(rowptr, "csr_rows_edges.rowptr")
    col = _idxc(col, "csr_rows_edges.col", torch.int32)
    val = _f32c(val, "csr_rows_edges.val")
    rows = _idxc(rows, "csr_rows_edges.rows").reshape(-1)
    n, R, dev = rowptr.numel() - 1, rows.numel(), rowptr.device
    off = torch.empty(R + 1, dtype=torch.int64, device=dev)
    ws = _workspace(L.ragraph_csr_rows_offsets_workspace_bytes(R), dev)
    N.check(L.ragraph_csr_rows_offsets_i64(rowptr.data_ptr(), n, rows.data_ptr() if R else None, R, off.data_ptr(), ws.data_ptr(),
                                           ws.numel(), _stream()), "csr_rows_offsets")
    E = int(off[R].item())
    if E < 0:
        raise RagraphNativeError("csr_rows_edges: the requested rows hold 2^31 edges or more")
    oc = torch.empty(E, dtype=torch.int64, device=dev)
    orr = torch.empty(E, dtype=torch.int64, device=dev)
    ov = torch.empty(E, dtype=torch.float32, device=dev)
    N.check(L.ragraph_csr_rows_edges_f32(rowptr.data_ptr(), _ptr(col), _ptr(val), rows.data_ptr() if R else None, R, off.data_ptr(),
                                         E, _ptr(oc), _ptr(orr), _ptr(ov), _stream()), "csr_rows_edges")
    return oc, orr, ov


def spmm_csr_panels(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, x: torch.Tensor, x_panels: bool, y_panels: bool,
                    act: int = ACT_NONE, alpha: float = 0.0) -> torch.Tensor:
    """act(A @ x) with x and / or the result PANEL-major ([D/32][n][32] floats, stored as an [n, D]-sized tensor) --
    the hops of a k-hop propagation between which the features never need to be row-major (ragraph_spmm_csr_panels_f32:
    an XCD gathers from one panel; same bits as spmm_csr in every layout)."""
    L = _ready()
    rowptr, col, val, x, n, D, _ = _csr_args("spmm_csr_panels", rowptr, col, val, x)
    y = torch.empty((n, D), dtype=torch.float32, device=x.device)
    N.check(L.ragraph_spmm_csr_panels_f32(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), n, x.data_ptr(), x.shape[0], int(x_panels),
                                          D, act, float(alpha), y.data_ptr(), int(y_panels), _stream()), "spmm_csr_panels")
    return y


def spmm_linear(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, x: torch.Tensor, weight: torch.Tensor,
                bias: torch.Tensor | None = None, act: int = ACT_NONE, alpha: float = 0.0) -> torch.Tensor:
    """act((A @ x) @ weight^T + bias) in ONE launch (ragraph_spmm_linear_f32: the aggregate-first GCN layer; x of 64 or 128
    columns): the bits of spmm_csr followed by linear, without the aggregated table in HBM."""
    L = _ready()
    rowptr, col, val, x, m, _, _ = _csr_args("spmm_linear", rowptr, col, val, x)
    w = _f32c(weight, "spmm_linear.weight")
    b = _f32c(bias, "spmm_linear.bias") if bias is not None else None
    n_out = w.shape[0]
    if w.shape[1] != x.shape[1]:
        raise ValueError(f"spmm_linear: weight [{w.shape[0]}, {w.shape[1]}] does not take x of {x.shape[1]} columns")
    y = torch.empty((m, n_out), dtype=torch.float32, device=x.device)
    if m:
        N.check(L.ragraph_spmm_linear_f32(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), m, x.data_ptr(), x.shape[1], w.data_ptr(),
                                          n_out, b.data_ptr() if b is not None else None, act, float(alpha), y.data_ptr(), _stream()),
                 "spmm_linear")
    return y


def spmm_linear_helps(n_rows: int, f_in: int, f_out: int) -> bool:
    """The aggregate-first layer in one launch: widths the fused kernel takes, enough rows to fill the chip, one block of output
    columns (every 256-column block would aggregate its rows again).  RAGRAPH_SPMM_LINEAR=0: the two launches (A/B)."""
    return f_in in (64, 128) and f_out <= 256 and n_rows >= 4096 and os.environ.get("RAGRAPH_SPMM_LINEAR", "1") != "0"


def spmm_csr_tiled(plan, val2: torch.Tensor, x: torch.Tensor, n: int, x_panels: bool, y_panels: bool, act: int = ACT_NONE,
                   alpha: float = 0.0) -> torch.Tensor:
    """act(A @ x) over a TILED graph (ragraph_spmm_csr_tiled_f32; plan = CSRGraph.tile_plan(...), val2 = the edge values in
    plan order): the layouts of spmm_csr_panels, the same bits, the X traffic of a hop cut to (passes) x the table."""
    L = _ready()
    x = _f32c(x, "spmm_csr_tiled.x")
    D = x.shape[1]
    y = torch.empty((n, D), dtype=torch.float32, device=x.device)
    N.check(L.ragraph_spmm_csr_tiled_f32(plan.wp.data_ptr(), plan.col3.data_ptr(), val2.data_ptr(), plan.row3.data_ptr(), plan.RG,
                                         plan.C, n, x.data_ptr(), x.shape[0], int(x_panels), D, act, float(alpha),
                                         y.data_ptr(), int(y_panels), _stream()), "spmm_csr_tiled")
    return y


def tiles_help(n: int, D: int) -> bool:
    """A hop over a table much larger than the eight L2s on the graph-tiled kernel -- OPT-IN (RAGRAPH_SPMM_TILED=1: D a multiple
    of 256; =2: also D = 64 / 128).  Measured on c2's graph (tools/gnn_probe.py, us per hop, tiled / panel kernel): row-major in
    119 / 134, panel-major in 114 / 118, the GNN forward alone 0.534 / 0.545 ms; on a uniformly random graph 125 / 135
    (tools/microbench/spmm_tiled_bench.hip).  Not the default because inside the full c2 step the hops run on a side stream UNDER
    the retrieval, and a tiled workgroup holds a CU's whole LDS for the length of the launch: the filter kernel's workgroup for
    that CU starts late -- 20.54 - 20.59 ms per step on the panel kernels, 20.55 - 20.69 tiled (A/B on one box,
    profiles/r6_spmm_tiled.txt)."""
    mode = os.environ.get("RAGRAPH_SPMM_TILED", "0")
    if mode == "0" or n * D * 4 < (32 << 20):
        return False
    return (D % 256 == 0 and D <= 2048) or (mode == "2" and D in (64, 128))


def panels_help(n: int, D: int, k: int) -> bool:
    """A k-hop propagation whose intermediate features are worth keeping panel-major: at least two hops over a table much
    larger than the eight L2s (c2: 100 000 x 256 -- 102 MB; a table that fits the L2s gains nothing), D = 256 (one panel per XCD)."""
    return k >= 2 and D == 256 and n * D * 4 >= (64 << 20) and os.environ.get("RAGRAPH_SPMM_PANELS", "1") != "0"


def slices_help(n: int, D: int) -> bool:
    """A plain aggregation act(A @ x) of a NARROW row-major table much larger than the L2s (c2's encoder input: 100 000 x 128,
    51 MB) on the XCD-sliced kernel -- every XCD gathers its 128-byte slice of each neighbour row: 73.6 -> 66.8 us
    (tools/gnn_probe.py).  Not at D = 256: row-major slices 1 KiB apart fall on an eighth of an L2's channels (136 us, the
    row kernel's time; the panel-major layout between the hops is what helps there)."""
    return D == 128 and n * D * 4 >= (32 << 20) and os.environ.get("RAGRAPH_SPMM_ROW_SLICES", "1") != "0"


def csr_row_normalize(rowptr: torch.Tensor, val: torch.Tensor) -> torch.Tensor:
    """val / rowsum -- Propagation.py:15-16."""
    L = _ready()
    rowptr = _idxc(rowptr, "csr_row_normalize.rowptr")
    val = _f32c(val, "csr_row_normalize.val")
    out = torch.empty_like(val)
    N.check(L.ragraph_csr_row_normalize_f32(rowptr.data_ptr(), val.data_ptr(), rowptr.numel() - 1, out.data_ptr(),
                                            _stream()), "csr_row_normalize")
    return out


def segment_softmax(rowptr: torch.Tensor, x: torch.Tensor, long_rows: bool = False) -> torch.Tensor:
    """scatter_softmax over CSR rows -- RAGraph_edge/modules/RAGraph.py:261 (`long_rows`: see spmm_csr)."""
    L = _ready()
    rowptr = _idxc(rowptr, "segment_softmax.rowptr")
    x = _f32c(x, "segment_softmax.x")
    out = torch.zeros_like(x)
    ws, ws_bytes = _hub_workspace(long_rows, x.numel(), 0, x.device)
    N.check(L.ragraph_segment_softmax_ws_f32(rowptr.data_ptr(), x.data_ptr(), rowptr.numel() - 1,
                                             x.numel() if long_rows else 0, out.data_ptr(), ws, ws_bytes, _stream()),
            "segment_softmax")
    return out


def axpby(a: torch.Tensor, wa: float, b: torch.Tensor, wb: float) -> torch.Tensor:
    """a*wa + b*wb (uncontracted) -- RAGraph.py:53."""
    L = _ready()
    a = _f32c(a, "axpby.a")
    b = _f32c(b, "axpby.b")
    if a.shape != b.shape:
        raise RagraphNativeError(f"axpby: shapes differ {tuple(a.shape)} vs {tuple(b.shape)}")
    out = torch.empty_like(a)
    N.check(L.ragraph_axpby_f32(a.data_ptr(), float(wa), b.data_ptr(), float(wb), a.numel(), out.data_ptr(),
                                _stream()), "axpby")
    return out


def interp_normalize(tables, weights, out: torch.Tensor | None = None) -> torch.Tensor:
    """F.normalize(sum_s tables[s] * weights[s], dim=1) in one pass -- RAGraph_edge/finetune_rag.py:63-86 (the interpolative
    update).  tables: 1 to INTERP_MAX_TABLES fp32 [n, D] device tensors of one shape on one device; weights: as many floats (a
    sequence or a host tensor).  The bits of the axpby chain followed by normalize_rows; `out` must not be one of the tables."""
    L = _ready()
    tables = list(tables)
    if not 1 <= len(tables) <= N.INTERP_MAX_TABLES:
        raise RagraphNativeError(f"interp_normalize: {len(tables)} tables, not 1 to {N.INTERP_MAX_TABLES}")
    for s, t in enumerate(tables):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
            raise RagraphNativeError(f"interp_normalize: table {s} must be an fp32 [n, D] ROCm device tensor")
        if t.shape != tables[0].shape or t.device != tables[0].device:
            raise RagraphNativeError(f"interp_normalize: table {s} is {tuple(t.shape)} on {t.device}, table 0 "
                                     f"{tuple(tables[0].shape)} on {tables[0].device}")
    tables = [t.contiguous() for t in tables]
    w = [float(x) for x in (weights.tolist() if isinstance(weights, torch.Tensor) else weights)]
    if len(w) != len(tables):
        raise RagraphNativeError(f"interp_normalize: {len(w)} weights for {len(tables)} tables")
    n, D = tables[0].shape
    if D < 1:
        raise RagraphNativeError("interp_normalize: tables have no columns")
    if out is None:
        out = torch.empty_like(tables[0])
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != tables[0].shape
          or out.device != tables[0].device or not out.is_contiguous()):
        raise RagraphNativeError("interp_normalize: out must be a contiguous fp32 tensor of the tables' shape and device")
    if n == 0:
        return out
    ptrs = (ctypes.c_void_p * len(tables))(*[t.data_ptr() for t in tables])
    ws = (ctypes.c_float * len(w))(*w)
    N.check(L.ragraph_interp_normalize_f32(ptrs, ws, len(tables), n, D, out.data_ptr(), _stream()), "interp_normalize")
    return out


def softmax_mix(logits: torch.Tensor, rag_label: torch.Tensor | None, lam: float = 0.0,
                log_mode: bool = False) -> torch.Tensor:
    """softmax(logits)*(1-lam) + rag_label*lam -- RAGraph.py:55-57."""
    L = _ready()
    logits = _f32c(logits, "softmax_mix.logits")
    lg = logits.reshape(-1, logits.shape[-1])
    rl = None if rag_label is None else _f32c(rag_label, "softmax_mix.rag_label").reshape(lg.shape)
    out = torch.empty_like(lg)
    N.check(L.ragraph_softmax_mix_f32(lg.data_ptr(), _ptr(rl), lg.shape[0], lg.shape[1], float(lam), int(log_mode),
                                      out.data_ptr(), _stream()), "softmax_mix")
    return out.reshape(logits.shape)


FUSE_DECODE_MAX_ROWS = 8192   # beyond: fc1 is faster on the MFMA tile kernel than in the fused launch's scalar chains
FUSE_DECODE_LDS = 64 * 1024


def fuse_decode_fits(n: int, D: int, H: int, C: int) -> bool:
    """Does ragraph_fuse_decode_f32 take this shape (and is it the faster form)?"""
    return 0 < n <= FUSE_DECODE_MAX_ROWS and 4 * 4 * ((D + 3) // 4 * 4 + (H + 3) // 4 * 4 + C) <= FUSE_DECODE_LDS


def fuse_decode(query: torch.Tensor, rag: torch.Tensor, wq: float, wr: float, W1: torch.Tensor, b1: torch.Tensor | None,
                slope: float, W2: torch.Tensor, b2: torch.Tensor | None, rag_label: torch.Tensor | None,
                lam: float) -> torch.Tensor:
    """K5 + K6 in one launch -- RAGraph_node/RAGraph.py:53-57 + TaskDecoder.py:14-17:
    softmax(fc2(LeakyReLU(fc1(query*wq + rag*wr)))) * (1-lam) + rag_label*lam.  Same bits as axpby -> linear(LEAKY) ->
    linear -> softmax_mix."""
    L = _ready()
    query, rag = _f32c(query, "fuse_decode.query"), _f32c(rag, "fuse_decode.rag")
    W1, W2 = _f32c(W1, "fuse_decode.W1"), _f32c(W2, "fuse_decode.W2")
    b1 = None if b1 is None else _f32c(b1, "fuse_decode.b1")
    b2 = None if b2 is None else _f32c(b2, "fuse_decode.b2")
    n, D = query.shape
    H, C = W1.shape[0], W2.shape[0]
    if rag.shape != query.shape or W1.shape[1] != D or W2.shape[1] != H:
        raise ValueError(f"fuse_decode: shapes query {tuple(query.shape)} rag {tuple(rag.shape)} W1 {tuple(W1.shape)} "
                         f"W2 {tuple(W2.shape)}")
    rl = None if rag_label is None else _f32c(rag_label, "fuse_decode.rag_label").reshape(n, C)
    out = torch.empty((n, C), dtype=torch.float32, device=query.device)
    N.check(L.ragraph_fuse_decode_f32(query.data_ptr(), rag.data_ptr(), n, D, float(wq), float(wr), W1.data_ptr(),
                                      _ptr(b1), H, float(slope), W2.data_ptr(), _ptr(b2), C, _ptr(rl), float(lam),
                                      out.data_ptr(), _stream()), "fuse_decode")
    return out


def segment_reduce(x: torch.Tensor, seg_ptr: torch.Tensor, w: torch.Tensor | None = None,
                   mean_mode: bool = False) -> torch.Tensor:
    """Per-segment sum (or mean) of rows, optionally of w*x -- RAGraph_graph/RAGraph.py:50,63; downprompt.py:98-112."""
    L = _ready()
    x = _f32c(x, "segment_reduce.x")
    seg_ptr = _idxc(seg_ptr, "segment_reduce.seg_ptr")
    wv = None if w is None else _f32c(w, "segment_reduce.w").reshape(-1)
    G = seg_ptr.numel() - 1
    out = torch.empty((G, x.shape[1]), dtype=torch.float32, device=x.device)
    N.check(L.ragraph_segment_reduce_f32(x.data_ptr(), x.shape[1], seg_ptr.data_ptr(), G, _ptr(wv), int(mean_mode),
                                         out.data_ptr(), _stream()), "segment_reduce")
    return out


def proto_cosine(emb: torch.Tensor, proto: torch.Tensor, mode: int = 0) -> torch.Tensor:
    """cosine(emb_g, proto_c) (+softmax / log_softmax) -- downprompt.py:41-56."""
    L = _ready()
    emb = _f32c(emb, "proto_cosine.emb")
    proto = _f32c(proto, "proto_cosine.proto")
    G, D = emb.shape
    C = proto.shape[0]
    out = torch.empty((G, C), dtype=torch.float32, device=emb.device)
    N.check(L.ragraph_proto_cosine_f32(emb.data_ptr(), G, D, proto.data_ptr(), C, mode, out.data_ptr(), _stream()),
            "proto_cosine")
    return out


def proto_cosine_grad(emb: torch.Tensor, proto: torch.Tensor, mode: int, out: torch.Tensor, gout: torch.Tensor):
    """Gradient of proto_cosine with respect to `emb` (prototypes constant)."""
    L = _ready()
    emb, proto = _f32c(emb, "proto_cosine_grad.emb"), _f32c(proto, "proto_cosine_grad.proto")
    out, gout = _f32c(out, "proto_cosine_grad.out"), _f32c(gout, "proto_cosine_grad.gout")
    G, D = emb.shape
    gemb = torch.empty_like(emb)
    N.check(L.ragraph_proto_cosine_grad_f32(emb.data_ptr(), G, D, proto.data_ptr(), proto.shape[0], mode, out.data_ptr(),
                                            gout.data_ptr(), gemb.data_ptr(), _stream()), "proto_cosine_grad")
    return gemb


def proto_cosine_grad_proto(emb: torch.Tensor, proto: torch.Tensor, mode: int, out: torch.Tensor, gout: torch.Tensor):
    """Gradient of proto_cosine with respect to the PROTOTYPES [C, D] (a training step that keeps them in the graph:
    RAGraph_node/downprompt.py:24-25); sums in a fixed order."""
    L = _ready()
    emb, proto = _f32c(emb, "proto_cosine_grad_proto.emb"), _f32c(proto, "proto_cosine_grad_proto.proto")
    out, gout = _f32c(out, "proto_cosine_grad_proto.out"), _f32c(gout, "proto_cosine_grad_proto.gout")
    G, D = emb.shape
    C = proto.shape[0]
    nbytes = int(L.ragraph_proto_cosine_grad_proto_workspace_bytes(G, C, D))
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=emb.device)
    gproto = torch.empty_like(proto)
    N.check(L.ragraph_proto_cosine_grad_proto_f32(emb.data_ptr(), G, D, proto.data_ptr(), C, mode, out.data_ptr(), gout.data_ptr(),
                                                  gproto.data_ptr(), ws.data_ptr(), nbytes, _stream()), "proto_cosine_grad_proto")
    return gproto


def axpby_dev(a: torch.Tensor, b: torch.Tensor, w: torch.Tensor, ia: int, ib: int) -> torch.Tensor:
    """a * w[ia] + b * w[ib], the weights read on the device (an index < 0: weight 0) -- RAGraph_node/downprompt.py:113."""
    L = _ready()
    a, b = _f32c(a, "axpby_dev.a"), _f32c(b, "axpby_dev.b")
    w = _f32c(w, "axpby_dev.w").reshape(-1)
    if a.shape != b.shape or max(ia, ib) >= w.numel():
        raise RagraphNativeError(f"axpby_dev: shapes {tuple(a.shape)} / {tuple(b.shape)}, weights {w.numel()}")
    out = torch.empty_like(a)
    N.check(L.ragraph_axpby_dev_f32(a.data_ptr(), b.data_ptr(), w.data_ptr(), int(ia), int(ib), a.numel(), out.data_ptr(),
                                    _stream()), "axpby_dev")
    return out


def topk_rows(scores: torch.Tensor, k: int):
    """torch.topk(scores, k) over a materialised [B,N] matrix, canonical tie order -- few-shot retrieve
    (RAGraph_node_fewshot/.../ToyGraphBase.py:64), edge evaluation (RAGraph_edge/utils/metrics.py:116).
    1 <= k <= min(N, TOPK_ORDERED_MAX): k <= TOPK_MAX takes the wave-list kernel, larger k the ordered large-k kernel
    (ragraph_topk_rows_large_f32; NaN is never selected, rows short of k other scores pad with -inf / INT64_MAX)."""
    L = _ready()
    s = _f32c(scores, "topk_rows.scores")
    if s.dim() != 2:
        raise RagraphNativeError(f"topk_rows: expected [B,N], got {tuple(s.shape)}")
    B, Nn = s.shape
    out_s = torch.empty((B, k), dtype=torch.float32, device=s.device)
    out_i = torch.empty((B, k), dtype=torch.int64, device=s.device)
    if k > N.TOPK_MAX:
        ws = _workspace(L.ragraph_topk_rows_large_workspace_bytes(B, Nn, k), s.device)
        N.check(L.ragraph_topk_rows_large_f32(s.data_ptr(), B, Nn, Nn, k, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(),
                                              ws.numel(), _stream()), "topk_rows")
        return out_s, out_i
    N.check(L.ragraph_topk_rows_f32(s.data_ptr(), B, Nn, Nn, k, out_s.data_ptr(), out_i.data_ptr(), _stream()),
            "topk_rows")
    return out_s, out_i


def topk_select_rows(scores: torch.Tensor, k: int):
    """The canonical top-k SET of every row for any k <= N: (kth [B], idx [B,k] in ascending index order) -- the edge
    flavour's vanilla-phase retrieval (RAGraph_edge/modules/RAGraph.py:57,73,308-321), which only averages the winners."""
    L = _ready()
    s = _f32c(scores, "topk_select_rows.scores")
    if s.dim() != 2:
        raise RagraphNativeError(f"topk_select_rows: expected [B,N], got {tuple(s.shape)}")
    B, Nn = s.shape
    kth = torch.empty(B, dtype=torch.float32, device=s.device)
    idx = torch.empty((B, k), dtype=torch.int64, device=s.device)
    if Nn >= 65536 and B <= 65535:  # long rows: every pass of the selection spread over (chunk, row) workgroups
        ws = _workspace(L.ragraph_topk_select_rows_workspace_bytes(B, Nn), s.device)
        N.check(L.ragraph_topk_select_rows_ws_f32(s.data_ptr(), B, Nn, Nn, k, kth.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                                                  ws.numel(), _stream()), "topk_select_rows")
        return kth, idx
    N.check(L.ragraph_topk_select_rows_f32(s.data_ptr(), B, Nn, Nn, k, kth.data_ptr(), idx.data_ptr(), _stream()),
            "topk_select_rows")
    return kth, idx


def retrieve_mean_large_k(q: torch.Tensor, keys_normalized: torch.Tensor, values: torch.Tensor, k: int,
                          slab_bytes: int = 1 << 30) -> torch.Tensor:
    """mean_k V[top-k(q)] for k beyond the fused kernels' lists (k > 64): score slabs by the dense kernel (the same
    fmaf chains as every other path), topk_select_rows, and the winners' sum in ascending index order times 1/k.
    RAGraph_edge/modules/RAGraph.py:298-324 with retrieve_num = 50 ... 100000.
    Up to ROW_BLOCK winners the sum is gather_reduce's sequential chain.  Beyond (retrieve_num = 100000: one lane group
    walking 100 k rows one after the other took 87 ms per 64 queries) the winners of a query are a CSR row of ones and the
    sum is the SpMM's hub-row path: blocks of ROW_BLOCK consecutive winners, each its own chain, spread over the chip,
    the block sums added in order -- the blocked order of oracle_spmm_csr, deterministic."""
    q = _f32c(q, "retrieve_mean_large_k.q")
    kn = _f32c(keys_normalized, "retrieve_mean_large_k.keys")
    values = _f32c(values, "retrieve_mean_large_k.values")
    B, Nk = q.shape[0], kn.shape[0]
    qn = normalize_rows(q)
    rows = max(1, min(B, slab_bytes // (4 * Nk)))
    out = torch.empty((B, values.shape[1]), dtype=torch.float32, device=q.device)
    ones = rowptr = None
    for b0 in range(0, B, rows):
        S = linear(qn[b0:b0 + rows], kn)
        _, idx = topk_select_rows(S, k)
        nb = idx.shape[0]
        if k <= ROW_BLOCK:
            out[b0:b0 + nb], _ = gather_reduce(values, None, idx, v_scale=1.0 / k)
            continue
        if ones is None or ones.numel() != nb * k:
            ones = torch.ones(nb * k, dtype=torch.float32, device=q.device)
            rowptr = torch.arange(0, (nb + 1) * k, k, dtype=torch.int64, device=q.device)
        total = spmm_csr(rowptr, idx.reshape(-1).to(torch.int32), ones, values, long_rows=True)
        out[b0:b0 + nb] = axpby(total, 1.0 / k, total, 0.0)
    return out


def scatter_fill_(scores: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, value: float) -> torch.Tensor:
    """In place: scores[b, col[rowptr[b]:rowptr[b+1]]] = value -- metrics.py:210-214 (_mask_history_pos)."""
    L = _ready()
    if not (scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous() and scores.dim() == 2):
        raise RagraphNativeError("scatter_fill_: scores must be a contiguous fp32 [B,N] device tensor")
    rowptr = _idxc(rowptr, "scatter_fill_.rowptr")
    col = _idxc(col, "scatter_fill_.col")
    B, Nn = scores.shape
    if col.numel() == 0:   # nothing listed (every row empty, or no rows): an empty tensor has no address to pass
        return scores
    N.check(L.ragraph_scatter_fill_f32(scores.data_ptr(), B, Nn, Nn, rowptr.data_ptr(), col.data_ptr(), float(value),
                                       _stream()), "scatter_fill")
    return scores


def floyd_warshall(adj_dense: torch.Tensor) -> torch.Tensor:
    """All-pairs shortest paths with the adjacency VALUES as edge lengths -- PositionAwareEncoder.py:27-48."""
    L = _ready()
    a = _f32c(adj_dense, "floyd_warshall.adj")
    if a.dim() != 2 or a.shape[0] != a.shape[1]:
        raise RagraphNativeError(f"floyd_warshall: adj must be a square [n, n] matrix, got {tuple(a.shape)}")
    n = a.shape[0]
    d = torch.empty_like(a)
    N.check(L.ragraph_floyd_warshall_f32(a.data_ptr(), n, d.data_ptr(), _stream()), "floyd_warshall")
    return d


def position_code(dist: torch.Tensor, anchors: torch.Tensor, dis_q: float = 10.0) -> torch.Tensor:
    """1/(d+1) if d < dis_q else 0 to each anchor -- PositionAwareEncoder.py:6-24."""
    L = _ready()
    d = _f32c(dist, "position_code.dist")
    anchors = _idxc(anchors, "position_code.anchors")
    if d.dim() != 2 or d.shape[0] != d.shape[1]:
        raise RagraphNativeError(f"position_code: dist must be a square [n, n] matrix, got {tuple(d.shape)}")
    if anchors.dim() != 1 or anchors.numel() == 0:
        raise RagraphNativeError(f"position_code: anchors must be a non-empty [A] vector, got {tuple(anchors.shape)}")
    out = torch.empty((d.shape[0], anchors.numel()), dtype=torch.float32, device=d.device)
    N.check(L.ragraph_position_code_f32(d.data_ptr(), d.shape[0], anchors.data_ptr(), anchors.numel(), float(dis_q),
                                        out.data_ptr(), _stream()), "position_code")
    return out


# Rounds the eager global path enqueues between two read-backs of the converged word (profiles/position_codes_global.txt).
POSITION_CODES_ROUNDS_PER_READBACK = 16


def position_codes_csr(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, anchors: torch.Tensor,
                       dis_q: float = 10.0, return_dist: bool = False, rounds: int | None = None,
                       method: str | None = None, return_converged: bool = False):
    """Position-aware codes [n, A] from the CSR of the query batch: shortest-path distances to the A anchors only, no
    n x n matrix -- PositionAwareEncoder.py:6-24 as the few-shot retrieve uses it on every forward
    (RAGraph_node_fewshot/ragraph_utils/ToyGraphBase.py:49-50).

    `method=None`: n <= 40000 with `rounds=None` takes the LDS kernel (one workgroup per anchor, one launch); anything else
    the global path (distance vectors in global memory, rows over the whole chip, one launch per round; any n < 2^31).
    `method="global"` forces the global path.  Both give the same bits.
    Global path, `rounds=None`: eager -- batches of rounds, one read-back of the converged word per batch, until converged
    or n rounds in total; cannot be captured.  `rounds=R`: one call, exactly R rounds, no read-back (capturable); the codes
    are final when the device int32 word `return_converged=True` adds to the result is 1, lower bounds otherwise (the LDS
    kernel has no such word: None).  Negative weights have no fixpoint on a negative cycle: both paths stop after n rounds."""
    if method not in (None, "global"):
        raise ValueError(f"position_codes_csr: method={method!r} (None or 'global')")
    if rounds is not None and (isinstance(rounds, bool) or int(rounds) != rounds or rounds < 1):
        raise ValueError(f"position_codes_csr: rounds={rounds!r} (None or an integer >= 1)")
    L = _ready()
    rowptr = _idxc(rowptr, "position_codes_csr.rowptr")
    col = _idxc(col, "position_codes_csr.col", torch.int32)
    val = _f32c(val, "position_codes_csr.val")
    anchors = _idxc(anchors, "position_codes_csr.anchors").reshape(-1)
    n, A = rowptr.numel() - 1, anchors.numel()
    codes = torch.empty((n, A), dtype=torch.float32, device=val.device)
    dist = torch.empty((n, A), dtype=torch.float32, device=val.device) if return_dist else None
    if method is None and rounds is None and n <= N.POSITION_CODES_LDS_MAX:
        N.check(L.ragraph_position_codes_csr_f32(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), n, anchors.data_ptr(), A,
                                                 float(dis_q), codes.data_ptr(), _ptr(dist), _stream()), "position_codes_csr")
        converged = None
    else:
        if rounds is None and torch.cuda.is_current_stream_capturing():
            raise RagraphNativeError("position_codes_csr: the global path reads the converged word back between batches of "
                                     "rounds; a captured call must pass `rounds` (a fixed number of rounds, no read-back)")
        nbytes = L.ragraph_position_codes_csr_global_workspace_bytes(n, A)
        if nbytes == 0:
            raise RagraphNativeError(f"position_codes_csr: n={n}, A={A} not supported (1 <= n < 2^31, A >= 1)")
        ws = _workspace(nbytes, val.device)
        converged = torch.empty(1, dtype=torch.int32, device=val.device)

        def call(r, resume):
            N.check(L.ragraph_position_codes_csr_global_f32(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), n,
                                                            anchors.data_ptr(), A, float(dis_q), codes.data_ptr(), _ptr(dist),
                                                            int(r), int(resume), converged.data_ptr(), ws.data_ptr(),
                                                            ws.numel(), _stream()), "position_codes_csr(global)")
        if rounds is not None:
            call(rounds, 0)
        else:
            done = 0
            while True:
                r = max(1, min(POSITION_CODES_ROUNDS_PER_READBACK, n - done))
                call(r, done > 0)
                done += r
                if done >= n or int(converged.item()) != 0:
                    break
    out = (codes, dist) if return_dist else (codes,)
    if return_converged:
        out = out + (converged,)
    return out if len(out) > 1 else out[0]


def sigmoid_gate(x: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """x * sigmoid(z) -- the embedding gate of RAGraph_edge/modules/RAGraph.py:168."""
    L = _ready()
    x = _f32c(x, "sigmoid_gate.x")
    z = _f32c(z, "sigmoid_gate.z")
    out = torch.empty_like(x)
    N.check(L.ragraph_sigmoid_gate_f32(x.data_ptr(), z.data_ptr(), x.numel(), out.data_ptr(), _stream()), "sigmoid_gate")
    return out


def time_rescale(t: torch.Tensor, t_min: float, t_max: float) -> torch.Tensor:
    """(t - t_min) / (t_max - t_min) on int64 time steps -- RAGraph_edge/modules/RAGraph.py:254-257."""
    L = _ready()
    t = _idxc(t, "time_rescale.t")
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    N.check(L.ragraph_time_rescale_f32(t.data_ptr(), t.numel(), float(t_min), float(t_max), out.data_ptr(), _stream()),
            "time_rescale")
    return out


# ---- toy-bank construction --------------------------------------------------------------
def csr_row_sums(rowptr: torch.Tensor, val: torch.Tensor) -> torch.Tensor:
    """Row sums of a CSR matrix (torch.sum(adj, dim=1); dim=0 on the transposed CSR) -- InverseSampling.py:25,53."""
    L = _ready()
    rowptr = _idxc(rowptr, "csr_row_sums.rowptr")
    val = _f32c(val, "csr_row_sums.val")
    out = torch.empty(rowptr.numel() - 1, dtype=torch.float32, device=val.device)
    N.check(L.ragraph_csr_row_sums_f32(rowptr.data_ptr(), val.data_ptr(), out.numel(), out.data_ptr(), _stream()),
            "csr_row_sums")
    return out


def pagerank(rowptr_t: torch.Tensor, col_t: torch.Tensor, val_t: torch.Tensor, out_deg: torch.Tensor,
             graph_ptr: torch.Tensor, d: float = 0.85, eps: float = 1e-6, max_iter: int = 128):
    """InverseSampling.pagerank_algorithm for a batch of graphs (segments of one block-diagonal transposed CSR), all
    power iterations enqueued without a host round trip.  Returns (p [n], iters [G] int32)."""
    L = _ready()
    rowptr_t = _idxc(rowptr_t, "pagerank.rowptr")
    col_t = _idxc(col_t, "pagerank.col", torch.int32)
    val_t = _f32c(val_t, "pagerank.val")
    out_deg = _f32c(out_deg, "pagerank.out_deg")
    graph_ptr = _idxc(graph_ptr, "pagerank.graph_ptr")
    n, G = out_deg.numel(), graph_ptr.numel() - 1
    if rowptr_t.numel() - 1 != n:
        raise RagraphNativeError(f"pagerank: out_deg has {n} entries, rowptr_t describes {rowptr_t.numel() - 1} rows")
    sizes = graph_ptr[1:] - graph_ptr[:-1]
    graph_of = torch.repeat_interleave(torch.arange(G, device=out_deg.device, dtype=torch.int32), sizes)
    p = torch.empty(n, dtype=torch.float32, device=out_deg.device)
    iters = torch.empty(G, dtype=torch.int32, device=out_deg.device)
    ws = _workspace(L.ragraph_pagerank_workspace_bytes(n, G), out_deg.device)
    N.check(L.ragraph_pagerank_f32(rowptr_t.data_ptr(), col_t.data_ptr(), val_t.data_ptr(), out_deg.data_ptr(),
                                   graph_ptr.data_ptr(), graph_of.data_ptr(), G, n, float(d), float(eps), int(max_iter),
                                   p.data_ptr(), iters.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "pagerank")
    return p, iters


def sample_prob(pagerank_p: torch.Tensor, col_sum: torch.Tensor, graph_ptr: torch.Tensor, alpha: float = 0.5,
                eps: float = 1e-6) -> torch.Tensor:
    """InverseSampling.compute_sample_prob (:6-19): inverse-importance sampling probabilities per graph."""
    L = _ready()
    pr = _f32c(pagerank_p, "sample_prob.pagerank")
    cs = _f32c(col_sum, "sample_prob.col_sum")
    graph_ptr = _idxc(graph_ptr, "sample_prob.graph_ptr")
    out = torch.empty_like(pr)
    N.check(L.ragraph_sample_prob_f32(pr.data_ptr(), cs.data_ptr(), graph_ptr.data_ptr(), graph_ptr.numel() - 1, float(alpha),
                                      float(eps), out.data_ptr(), _stream()), "sample_prob")
    return out


def position_codes_batch(adj: torch.Tensor, anchors: torch.Tensor, dis_q: float = 10.0, return_dist: bool = False):
    """PositionAwareEncoder.encode_position_aware_code for G graphs of n <= 64 nodes: adj [G,n,n], anchors [G,A] ->
    codes [G,n,A] (and the all-pairs distances [G,n,n])."""
    L = _ready()
    a = _f32c(adj, "position_codes_batch.adj")
    anchors = _idxc(anchors, "position_codes_batch.anchors")
    if a.dim() != 3 or a.shape[1] != a.shape[2]:
        raise RagraphNativeError(f"position_codes_batch: adj must be [G, n, n], got {tuple(a.shape)}")
    if anchors.dim() != 2 or anchors.shape[0] != a.shape[0]:
        raise RagraphNativeError(f"position_codes_batch: anchors must be [G, A] with G = {a.shape[0]}, got "
                                 f"{tuple(anchors.shape)}")
    G, n, _ = a.shape
    A = anchors.shape[1]
    codes = torch.empty((G, n, A), dtype=torch.float32, device=a.device)
    dist = torch.empty_like(a) if return_dist else None
    N.check(L.ragraph_position_codes_batch_f32(a.data_ptr(), G, n, anchors.data_ptr(), A, float(dis_q), _ptr(dist),
                                               codes.data_ptr(), _stream()), "position_codes_batch")
    return (codes, dist) if return_dist else codes


# ---- graph ingestion --------------------------------------------------------------------
def csr_sym_normalized_from_edges(edge_index: torch.Tensor, n: int):
    """D^-1/2 (A + I) D^-1/2 as CSR from an edge list [2,E] -- ragraph_utils/utility.py:19-26,45-66.  Returns (rowptr
    int64 [n+1], col int32 [nnz], val fp32 [nnz]).  Reads the entry count back (one synchronisation: ingestion is a
    per-graph step, not part of the captured forward)."""
    L = _ready()
    ei = _idxc(edge_index, "csr_sym_normalized.edge_index")
    E = ei.shape[1]
    dev = ei.device
    rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    col = torch.empty(E + n, dtype=torch.int32, device=dev)
    val = torch.empty(E + n, dtype=torch.float32, device=dev)
    nnz = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _workspace(L.ragraph_ingest_workspace_bytes(E + n, n), dev)
    N.check(L.ragraph_csr_sym_normalized_f32(ei[0].data_ptr() if E else None, ei[1].data_ptr() if E else None, E, n,
                                             rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), nnz.data_ptr(), ws.data_ptr(),
                                             ws.numel(), _stream()), "csr_sym_normalized")
    m = int(nnz.item())
    return rowptr, col[:m].contiguous(), val[:m].contiguous()


def coo_to_csr(rows: torch.Tensor, cols: torch.Tensor, n: int, sort_cols: bool = False):
    """COO -> CSR, stable (ragraph_coo_to_csr_i64): returns (rowptr int64 [n+1], col int32 [E] in CSR order, perm int64 [E] =
    the input position of every CSR slot).  No read-back, no other library: the per-step graph rebuilds of the edge flavour,
    the transposed patterns of training and the gather backward come through here."""
    L = _ready()
    r, c = _idxc(rows, "coo_to_csr.rows"), _idxc(cols, "coo_to_csr.cols")
    E = r.numel()
    if c.numel() != E:
        raise RagraphNativeError("coo_to_csr: rows and cols differ in length")
    dev = r.device
    rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    perm = torch.empty(E, dtype=torch.int64, device=dev)
    col = torch.empty(E, dtype=torch.int32, device=dev)
    ws = _workspace(L.ragraph_coo_to_csr_workspace_bytes(E, n), dev)
    N.check(L.ragraph_coo_to_csr_i64(r.data_ptr() if E else None, c.data_ptr() if E else None, E, n, 1 if sort_cols else 0,
                                     rowptr.data_ptr(), perm.data_ptr() if E else None, col.data_ptr() if E else None,
                                     ws.data_ptr(), ws.numel(), _stream()), "coo_to_csr")
    return rowptr, col, perm


def dense_to_csr(a: torch.Tensor, capacity: int | None = None, max_entries: int | None = None):
    """Dense fp32 [rows, cols] (or a [1, rows, cols] view; unit column stride, any row stride) -> CSR of the entries that
    compare unequal to 0 (ragraph_dense_to_csr_f32: torch.nonzero's rule and order -- row-major, columns ascending; the
    values keep their bits).
    capacity=None: the eager form -- a count-only call, ONE 8-byte read-back of the entry count, exact-size buffers, the
    fill.  Returns (rowptr int64 [rows+1], col int32 [nnz], val fp32 [nnz]); with `max_entries`, None -- and no fill -- when
    the matrix holds more entries than that (a density test costs the count pass alone).
    capacity=int: no read-back at all (capturable).  Returns (rowptr, col [capacity], val [capacity], status int64 [2] on
    the device): rowptr holds the true prefix counts whatever the capacity, status[0] the true entry count, status[1] = 1
    iff it exceeds `capacity` (the entries behind the capacity are then missing: the caller owns that check).  The slots
    of col / val behind rowptr[rows] are never written."""
    L = _ready()
    if not isinstance(a, torch.Tensor) or not a.is_cuda:
        raise RagraphNativeError("dense_to_csr.a: expected a ROCm device tensor (ragraph_amd has no CPU fallback)")
    if a.dtype != torch.float32:
        raise RagraphNativeError(f"dense_to_csr.a: expected float32, got {a.dtype}")
    if a.dim() == 3 and a.shape[0] == 1:
        a = a[0]
    if a.dim() != 2:
        raise RagraphNativeError(f"dense_to_csr.a: expected [rows, cols] or [1, rows, cols], got {tuple(a.shape)}")
    rows, cols = a.shape
    if (cols > 1 and a.stride(1) != 1) or (rows > 1 and a.stride(0) < cols):   # (a transposed or expanded view: one copy)
        a = a.contiguous()
    lda = a.stride(0) if rows > 1 else cols
    dev = a.device
    nbytes = L.ragraph_dense_to_csr_workspace_bytes(rows, cols)
    if nbytes == 0:
        raise RagraphNativeError(f"dense_to_csr: {rows} x {cols} not supported (rows * cols must be below 2^31)")
    # (the row counts and the scan's scratch: 4 (rows + 1) bytes and a little of this call's own, exactly sized -- not the
    # shared grow-only scratch)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rowptr = torch.empty(rows + 1, dtype=torch.int64, device=dev)
    status = torch.empty(2, dtype=torch.int64, device=dev)
    ap = a.data_ptr() if rows and cols else None

    def call(cap, col, val):
        N.check(L.ragraph_dense_to_csr_f32(ap, rows, cols, lda, cap, rowptr.data_ptr(), _ptr(col), _ptr(val),
                                           status.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "dense_to_csr")

    if capacity is not None:
        cap = int(capacity)
        if cap < 0:
            raise RagraphNativeError(f"dense_to_csr: capacity={cap}")
        # (at least one slot is allocated, so that the pointers are valid; the library is told the caller's capacity)
        col = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)[:cap]
        val = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)[:cap]
        call(cap, col if cap else None, val if cap else None)
        return rowptr, col, val, status
    call(0, None, None)
    nnz = int(status[0])                    # the one read-back (torch.nonzero has its own)
    if max_entries is not None and nnz > max_entries:
        return None
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev)
    if nnz:
        call(nnz, col, val)
    return rowptr, col, val


def csr_row_ids(rowptr: torch.Tensor, nnz: int) -> torch.Tensor:
    """rows[e] = the row of CSR slot e (ragraph_csr_row_ids_i64)."""
    L = _ready()
    rp = _idxc(rowptr, "csr_row_ids.rowptr")
    rows = torch.empty(nnz, dtype=torch.int64, device=rp.device)
    N.check(L.ragraph_csr_row_ids_i64(rp.data_ptr(), rp.numel() - 1, nnz, rows.data_ptr() if nnz else None, _stream()),
            "csr_row_ids")
    return rows


def mask_positions(mask: torch.Tensor) -> torch.Tensor:
    """Positions of the set elements of a bool / uint8 mask, ascending (ragraph_mask_positions_i64) -- x[mask] as
    x[mask_positions(mask)] without another library's select.  Reads the count back (one synchronisation, as boolean
    indexing does)."""
    L = _ready()
    if not mask.is_cuda or mask.dtype not in (torch.bool, torch.uint8):
        raise RagraphNativeError("mask_positions: expected a bool / uint8 ROCm device tensor")
    m = mask.contiguous().view(torch.uint8).reshape(-1)
    E = m.numel()
    pos = torch.empty(E, dtype=torch.int64, device=m.device)
    count = torch.empty(1, dtype=torch.int64, device=m.device)
    ws = _workspace(L.ragraph_mask_positions_workspace_bytes(E), m.device)
    N.check(L.ragraph_mask_positions_i64(m.data_ptr() if E else None, E, pos.data_ptr() if E else None, count.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _stream()), "mask_positions")
    return pos[:int(count.item())]


def binorm_edges(users: torch.Tensor, items: torch.Tensor, step: torch.Tensor, num_users: int, num_items: int):
    """Bi-normalised bipartite adjacency as a (dst, src)-sorted edge list with per-edge time steps --
    RAGraph_edge/modules/base_model.py:34-52 + utils/dataloader.py:94,108-113.  Returns (edges [M,2] int64, norm [M],
    times [M] int64)."""
    L = _ready()
    u, i, t = (_idxc(x, "binorm_edges") for x in (users, items, step))
    E = u.numel()
    dev = u.device
    edges = torch.empty((2 * E, 2), dtype=torch.int64, device=dev)
    norm = torch.empty(2 * E, dtype=torch.float32, device=dev)
    times = torch.empty(2 * E, dtype=torch.int64, device=dev)
    ne = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _workspace(L.ragraph_ingest_workspace_bytes(2 * E, num_users + num_items), dev)
    N.check(L.ragraph_binorm_edges_f32(u.data_ptr(), i.data_ptr(), t.data_ptr(), E, num_users, num_items, edges.data_ptr(),
                                       norm.data_ptr(), times.data_ptr(), ne.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
            "binorm_edges")
    m = int(ne.item())
    return edges[:m].contiguous(), norm[:m].contiguous(), times[:m].contiguous()


# ---- element-wise derivatives of the fused epilogues (fine-tuning backward) -------------------------------------------
def act_grad(y: torch.Tensor, gy: torch.Tensor, act: int, alpha: float = 0.0, want_alpha_terms: bool = False):
    """gz = gy * act'(z) through the output y; with want_alpha_terms also gy * z on z < 0 (PReLU slope gradient terms)."""
    L = _ready()
    y, gy = _f32c(y, "act_grad.y"), _f32c(gy, "act_grad.gy")
    gz = torch.empty_like(y)
    t = torch.empty_like(y) if want_alpha_terms else None
    N.check(L.ragraph_act_grad_f32(y.data_ptr(), gy.data_ptr(), y.numel(), act, float(alpha), gz.data_ptr(), _ptr(t), _stream()),
            "act_grad")
    return (gz, t) if want_alpha_terms else gz


def spmm_csr_prelu_dev(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, x: torch.Tensor, bias: torch.Tensor | None,
                       alpha: torch.Tensor, want_z: bool = False, long_rows: bool = False):
    """PReLU(A @ x + bias) with the slope read on the DEVICE from alpha[0] (a trained nn.PReLU weight: no host read, so a
    captured HIP graph follows the slope as the optimizer moves it).  want_z: also the pre-activation A @ x + bias ->
    (y, z).  Bit-identical to spmm_csr(..., act=ACT_PRELU, alpha=float(alpha[0])) (and z to act=ACT_NONE)."""
    L = _ready()
    rowptr, col, val, x, n, D, nnz = _csr_args("spmm_csr_prelu_dev", rowptr, col, val, x)
    a = _f32c(alpha, "spmm_csr_prelu_dev.alpha")
    if a.numel() != 1:
        raise ValueError(f"spmm_csr_prelu_dev: one slope expected (nn.PReLU(num_parameters=1)), got {a.numel()}")
    b = None if bias is None else _f32c(bias, "spmm_csr_prelu_dev.bias")
    y = torch.empty((n, D), dtype=torch.float32, device=x.device)
    z = torch.empty((n, D), dtype=torch.float32, device=x.device) if want_z else None
    ws, ws_bytes = _hub_workspace(long_rows, nnz, D, x.device)
    N.check(L.ragraph_spmm_csr_prelu_dev_f32(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), n, x.data_ptr(), D, _ptr(b),
                                             a.data_ptr(), y.data_ptr(), _ptr(z), nnz if long_rows else 0, ws, ws_bytes,
                                             _stream()), "spmm_csr_prelu_dev")
    return (y, z) if want_z else y


def act_grad_prelu_dev(z: torch.Tensor, gy: torch.Tensor, alpha: torch.Tensor, want_alpha_terms: bool = False):
    """gz = gy * PReLU'(z) from the PRE-activation z, slope read on the device; with want_alpha_terms also gy * min(z, 0)
    (the slope's gradient terms).  The bits of the host-scalar training path for the slope's sign (include/ragraph_hip.h)."""
    L = _ready()
    z, gy = _f32c(z, "act_grad_prelu_dev.z"), _f32c(gy, "act_grad_prelu_dev.gy")
    a = _f32c(alpha, "act_grad_prelu_dev.alpha")
    if gy.shape != z.shape:
        raise ValueError(f"act_grad_prelu_dev: gy {tuple(gy.shape)} vs z {tuple(z.shape)}")
    gz = torch.empty_like(z)
    t = torch.empty_like(z) if want_alpha_terms else None
    N.check(L.ragraph_act_grad_prelu_dev_f32(z.data_ptr(), gy.data_ptr(), z.numel(), a.data_ptr(), gz.data_ptr(), _ptr(t),
                                             _stream()), "act_grad_prelu_dev")
    return (gz, t) if want_alpha_terms else gz


def sigmoid_gate_grad(x: torch.Tensor, z: torch.Tensor, g: torch.Tensor):
    L = _ready()
    x, z, g = _f32c(x, "sigmoid_gate_grad.x"), _f32c(z, "sigmoid_gate_grad.z"), _f32c(g, "sigmoid_gate_grad.g")
    gx, gz = torch.empty_like(x), torch.empty_like(x)
    N.check(L.ragraph_sigmoid_gate_grad_f32(x.data_ptr(), z.data_ptr(), g.data_ptr(), x.numel(), gx.data_ptr(), gz.data_ptr(),
                                            _stream()), "sigmoid_gate_grad")
    return gx, gz


def softmax_grad(p: torch.Tensor, go: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    L = _ready()
    p, go = _f32c(p, "softmax_grad.p"), _f32c(go, "softmax_grad.go")
    p2 = p.reshape(-1, p.shape[-1])
    out = torch.empty_like(p2)
    N.check(L.ragraph_softmax_grad_f32(p2.data_ptr(), go.reshape(p2.shape).data_ptr(), p2.shape[0], p2.shape[1], float(scale),
                                       out.data_ptr(), _stream()), "softmax_grad")
    return out.reshape(p.shape)


def mul_cols(x: torch.Tensor, w: torch.Tensor, act: int = ACT_NONE, alpha: float = 0.0) -> torch.Tensor:
    """act(x[r,:] * w) -- downstreamprompt.forward: plain in the graph flavour (RAGraph_graph/downprompt.py:164-168), ELU
    in the node flavour (RAGraph_node/downprompt.py:118-130)."""
    L = _ready()
    x = _f32c(x, "mul_cols.x")
    w = _f32c(w, "mul_cols.w").reshape(-1)
    if w.numel() != x.shape[-1]:
        raise RagraphNativeError(f"mul_cols: weight of {w.numel()} values for rows of {x.shape[-1]}")
    x2 = x.reshape(-1, x.shape[-1])
    out = torch.empty_like(x2)
    N.check(L.ragraph_mul_cols_act_f32(x2.data_ptr(), w.data_ptr(), x2.shape[0], x2.shape[1], int(act), float(alpha),
                                       out.data_ptr(), _stream()), "mul_cols")
    return out.reshape(x.shape)


def mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a * b elementwise (same shape)."""
    L = _ready()
    a, b = _f32c(a, "mul.a"), _f32c(b, "mul.b")
    if a.shape != b.shape:
        raise RagraphNativeError(f"mul: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    out = torch.empty_like(a)
    N.check(L.ragraph_mul_f32(a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(), _stream()), "mul")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# f4: edge (link-prediction) evaluation -- RAGraph_edge/utils/metrics.py:83-141
def topk_dot_masked_workspace_bytes(B: int, n_items: int, D: int, k: int, nnz: int) -> int:
    """Scratch bytes of one topk_dot_masked call (no [B, n_items] slab on the fused kernels)."""
    return int(N.lib().ragraph_topk_dot_masked_workspace_bytes(B, n_items, D, k, nnz))


def topk_dot_masked(user_emb: torch.Tensor, item_emb: torch.Tensor, k: int, hist_rowptr: torch.Tensor,
                    hist_items: torch.Tensor, users: torch.Tensor | None = None, mask_value: float = -1e8):
    """(scores [B,k] f32, idx [B,k] i64): rating = user_emb[users] @ item_emb.T, the items of query b's history
    hist_items[hist_rowptr[b]:hist_rowptr[b+1]] SCORED as mask_value (metrics.py:210-214), canonical top-k (metrics.py:116).
    users=None: query b = row b.  Histories may be unsorted and hold duplicates; an id out of range raises."""
    L = _ready()
    ue = _f32c(user_emb, "topk_dot_masked.user_emb")
    ie = _f32c(item_emb, "topk_dot_masked.item_emb")
    rp = _idxc(hist_rowptr, "topk_dot_masked.hist_rowptr")
    hi = _idxc(hist_items, "topk_dot_masked.hist_items")
    us = None if users is None else _idxc(users, "topk_dot_masked.users")
    if ue.dim() != 2 or ie.dim() != 2 or ue.shape[1] != ie.shape[1]:
        raise RagraphNativeError(f"topk_dot_masked: bad shapes {tuple(ue.shape)} x {tuple(ie.shape)}")
    if k > N.TOPK_MAX:
        raise RagraphNativeError(f"topk_dot_masked: k={k} exceeds the kernels' limit of {N.TOPK_MAX}")
    B = ue.shape[0] if us is None else us.numel()
    Ni, D = ie.shape
    if rp.numel() != B + 1:
        raise RagraphNativeError(f"topk_dot_masked: hist_rowptr has {rp.numel()} entries, expected {B + 1}")
    scores = torch.empty((B, k), dtype=torch.float32, device=ue.device)
    idx = torch.empty((B, k), dtype=torch.int64, device=ue.device)
    if B == 0:
        return scores, idx
    nnz = hi.numel()
    ws = _workspace(L.ragraph_topk_dot_masked_workspace_bytes(B, Ni, D, k, nnz), ue.device)
    N.check(L.ragraph_topk_dot_masked_f32(ue.data_ptr(), ue.shape[0], _ptr(us), B, ie.data_ptr(), Ni, D, k, rp.data_ptr(),
                                          hi.data_ptr() if nnz else None, nnz, float(mask_value), scores.data_ptr(),
                                          idx.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "topk_dot_masked")
    return scores, idx


RANK_METRICS = ("recall", "ndcg", "precision")   # the rows of rank_metrics' result


def rank_metrics(idx: torch.Tensor, gt_rowptr: torch.Tensor, gt_items: torch.Tensor, ks, batch: int = 512):
    """metrics.py:12-46 + 60-80 + 131-133 on the device: [3, len(ks)] float64 numpy array (rows recall, ndcg, precision)
    of the ranked lists idx [U, kmax] against the ground-truth CSR; sums in batches of `batch` users, added batch by batch
    (the reference's order).  One read-back of 3 x len(ks) doubles."""
    L = _ready()
    ix = _idxc(idx, "rank_metrics.idx")
    rp = _idxc(gt_rowptr, "rank_metrics.gt_rowptr")
    gi = _idxc(gt_items, "rank_metrics.gt_items")
    if ix.dim() != 2:
        raise RagraphNativeError(f"rank_metrics: idx must be [U, kmax], got {tuple(ix.shape)}")
    U, kmax = ix.shape
    if rp.numel() != U + 1:
        raise RagraphNativeError(f"rank_metrics: gt_rowptr has {rp.numel()} entries, expected {U + 1}")
    ks = [int(k) for k in ks]
    karr = (ctypes.c_int * len(ks))(*ks)
    out = torch.empty(3 * len(ks), dtype=torch.float64, device=ix.device)
    ws = _workspace(L.ragraph_rank_metrics_workspace_bytes(U, len(ks), batch), ix.device)
    N.check(L.ragraph_rank_metrics_f64(ix.data_ptr(), U, kmax, rp.data_ptr(), gi.data_ptr() if gi.numel() else None, karr,
                                       len(ks), batch, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "rank_metrics")
    return out.cpu().numpy().reshape(3, len(ks))


# ---- link-prediction pre-training (csrc/pretrain.hip) -----------------------------------------------------------------
LP_NEG_MAX = 4096   # negatives per row the sampler and the compare loss take


def lp_sample(rowptr: torch.Tensor, col: torch.Tensor, n_neg: int, seed: torch.Tensor) -> torch.Tensor:
    """prompt_pretrain_sample (preprompt.py:106-126) over a CSR pattern with strictly ascending columns (a diagonal entry is
    ignored): int64 [n, 1 + n_neg], column 0 a neighbour (or i when isolated), then n_neg distinct non-neighbours.  `seed` is
    a one-element int64 device tensor (read on the device).  A row with neighbours and fewer than n_neg non-neighbours
    raises ValueError, as the reference fails on it; any other bad pattern raises RagraphNativeError."""
    L = _ready()
    rp = _idxc(rowptr, "lp_sample.rowptr")
    c = _idxc(col, "lp_sample.col", torch.int32)
    sd = _idxc(seed, "lp_sample.seed")
    n = rp.numel() - 1
    out = torch.empty((n, 1 + n_neg), dtype=torch.int64, device=rp.device)
    ws = _workspace(L.ragraph_lp_workspace_bytes(), rp.device)
    rc = L.ragraph_lp_sample_i64(rp.data_ptr(), c.data_ptr() if c.numel() else None, n, c.numel(), int(n_neg), sd.data_ptr(),
                                 out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    if rc == N.EINVAL and "non-neighbours" in N.last_error():
        raise ValueError(N.last_error())
    N.check(rc, "lp_sample")
    return out


def lp_compare_loss_fwd(h: torch.Tensor, t: torch.Tensor, temperature: float):
    """compareloss (preprompt.py:80-103) forward: (loss [1], L [n], coef [n, S], csim [n, S], hhat [n, D], nrm [n]) -- coef the
    backward's dL_i/dsim, csim = coef * sim, hhat = h / max(||h||, 1e-8) and nrm = ||h|| (what the backward needs)."""
    L = _ready()
    h = _f32c(h, "lp_compare_loss.h")
    t = _idxc(t, "lp_compare_loss.tuples")
    n, D = h.shape
    if t.dim() != 2 or t.shape[0] != n:
        raise RagraphNativeError(f"lp_compare_loss: tuples must be [{n}, 1 + n_neg], got {tuple(t.shape)}")
    S = t.shape[1]
    dev = h.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    Li = torch.empty(n, dtype=torch.float32, device=dev)
    coef = torch.empty((n, S), dtype=torch.float32, device=dev)
    csim = torch.empty((n, S), dtype=torch.float32, device=dev)
    hhat = torch.empty((n, D), dtype=torch.float32, device=dev)
    nrm = torch.empty(n, dtype=torch.float32, device=dev)
    ws = _workspace(L.ragraph_lp_workspace_bytes(), dev)
    N.check(L.ragraph_lp_compare_loss_fwd_f32(h.data_ptr(), n, D, t.data_ptr(), S, float(temperature), loss.data_ptr(),
                                              Li.data_ptr(), coef.data_ptr(), csim.data_ptr(), hhat.data_ptr(), nrm.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _stream()), "lp_compare_loss")
    return loss, Li, coef, csim, hhat, nrm


def lp_combine(x: torch.Tensor, h: torch.Tensor, nrm: torch.Tensor, beta: torch.Tensor, go: torch.Tensor,
               inv_rows: float) -> torch.Tensor:
    """go[0] * inv_rows * (x / N - beta * h / (N ||h||)) per row, N = max(||h||, 1e-8) (ragraph_lp_combine_f32)."""
    L = _ready()
    x, h = _f32c(x, "lp_combine.x"), _f32c(h, "lp_combine.h")
    nrm, beta, go = _f32c(nrm, "lp_combine.nrm"), _f32c(beta, "lp_combine.beta"), _f32c(go, "lp_combine.go")
    n, D = h.shape
    out = torch.empty_like(h)
    N.check(L.ragraph_lp_combine_f32(x.data_ptr(), h.data_ptr(), nrm.data_ptr(), beta.data_ptr(), go.data_ptr(),
                                     float(inv_rows), n, D, out.data_ptr(), _stream()), "lp_combine")
    return out


# ---- edge flavour pre-training (csrc/pretrain.hip) --------------------------------------------------------------------
def edge_hist_check(rowptr: torch.Tensor, items: torch.Tensor, num_items: int) -> None:
    """Validate a training-history CSR (rowptr int64 [num_users + 1], items int64, strictly ascending per user) once, when it
    is built (ragraph_edge_hist_check_i64, one read-back).  A user whose history covers every item raises ValueError (the
    reference's rejection loop never ends there); any other bad CSR raises RagraphNativeError."""
    L = _ready()
    rp = _idxc(rowptr, "edge_hist_check.rowptr")
    it = _idxc(items, "edge_hist_check.items")
    ws = _workspace(L.ragraph_lp_workspace_bytes(), rp.device)
    rc = L.ragraph_edge_hist_check_i64(rp.data_ptr(), it.data_ptr() if it.numel() else None, rp.numel() - 1, int(num_items),
                                       it.numel(), ws.data_ptr(), ws.numel(), _stream())
    if rc == N.EINVAL and "covers every item" in N.last_error():
        raise ValueError(N.last_error())
    N.check(rc, "edge_hist_check")


def edge_neg_sample(rowptr: torch.Tensor, items: torch.Tensor, num_items: int, users: torch.Tensor, n_negs: int,
                    seed: torch.Tensor, check_users: bool = True) -> torch.Tensor:
    """negative_sampling (RAGraph_edge/utils/dataloader.py:142-152) on the device: int64 [len(users) * n_negs], slot
    b * n_negs + j uniform over [0, num_items) minus the history of users[b], every slot an independent draw.  The history
    (rowptr, items) must have passed edge_hist_check.  `seed` is a one-element int64 device tensor (read on the device).
    check_users: user ids outside [0, num_users) raise RagraphNativeError before anything is written (one read-back);
    without it the call makes no read-back (the caller vouches for the ids)."""
    L = _ready()
    rp = _idxc(rowptr, "edge_neg_sample.rowptr")
    it = _idxc(items, "edge_neg_sample.items")
    u = _idxc(users, "edge_neg_sample.users")
    sd = _idxc(seed, "edge_neg_sample.seed")
    B = u.numel()
    out = torch.empty(B * int(n_negs), dtype=torch.int64, device=rp.device)
    ws = _workspace(L.ragraph_lp_workspace_bytes(), rp.device) if check_users else None
    N.check(L.ragraph_edge_neg_sample_i64(rp.data_ptr(), it.data_ptr() if it.numel() else None, rp.numel() - 1,
                                          int(num_items), u.data_ptr() if B else None, B, int(n_negs), 1 if check_users else 0,
                                          sd.data_ptr(), out.data_ptr() if B else None, _ptr(ws),
                                          ws.numel() if ws is not None else 0, _stream()), "edge_neg_sample")
    return out


# ---- noisy fine-tuning with the noise drawn on the device (csrc/noise.hip) ---------------------------------------------
def _noise_keys(seed: torch.Tensor, row_ids, B: int, what: str):
    sd = _idxc(seed, f"{what}.seed")
    if sd.numel() != 1:
        raise RagraphNativeError(f"{what}: seed must hold one int64, got {tuple(sd.shape)}")
    if row_ids is not None:
        row_ids = _idxc(row_ids, f"{what}.row_ids").reshape(-1)
        if row_ids.numel() != B:
            raise RagraphNativeError(f"{what}: {row_ids.numel()} row ids for {B} rows")
    return sd, row_ids


def noise_rows(seed: torch.Tensor, B: int, m: int, n: int, row_ids: torch.Tensor | None = None, row_base: int = 0,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """int64 [B, m]: m rows of a bank of n per query, slot (b, j) the hash of (seed[0], row id of b, j) reduced to [0, n)
    (ragraph_noise_rows_i64) -- what torch.randint(0, n, (B, m)) is to the reference's noisy retrieval.  `seed` is a
    one-element int64 device tensor (read on the device).  row_ids: the queries' ids, int64 [B] on the device; without them
    row b has the id row_base + b.  out: an int64 [B, m] view to fill in place -- contiguous, or columns of a wider
    contiguous matrix (the tail columns of a [B, k + m] index matrix)."""
    L = _ready()
    B, m = int(B), int(m)
    sd, row_ids = _noise_keys(seed, row_ids, B, "noise_rows")
    if out is None:
        out = torch.empty((B, max(m, 0)), dtype=torch.int64, device=sd.device)
        stride = m
    else:
        if (not out.is_cuda or out.dtype != torch.int64 or tuple(out.shape) != (B, m) or (m > 1 and out.stride(1) != 1)
                or (B > 1 and out.stride(0) < m)):
            raise RagraphNativeError(f"noise_rows: out must be an int64 device view [{B}, {m}] with unit column stride")
        stride = out.stride(0) if B > 1 else m
    N.check(L.ragraph_noise_rows_i64(sd.data_ptr(), _ptr(row_ids), int(row_base), B, m, int(n), out.data_ptr() if B else None,
                                     stride, _stream()), "noise_rows")
    return out


def gather_reduce_noisy(v: torch.Tensor, labels: torch.Tensor | None, idx: torch.Tensor, seed: torch.Tensor, m: int,
                        noise_n: int | None = None, row_ids: torch.Tensor | None = None, row_base: int = 0, idx_base: int = 0,
                        v_scale: float = 1.0, mix=None):
    """gather_reduce over idx [B, k] AND m noise rows per query behind them, with no index matrix for the noise: the bits of
    gather_reduce(v, labels, cat(idx, noise_rows(seed, B, m, noise_n, row_ids, row_base)), idx_base, v_scale); the label
    means are over k + m rows.  noise_n: the range of the draw (the whole bank; v.shape[0] when v is the whole bank).
    mix = (a, wa, wb): a * wa + (v_scale * sum) * wb instead of the sum, as gather_reduce_mix."""
    L = _ready()
    v = _f32c(v, "gather_reduce_noisy.v")
    idx = _idxc(idx, "gather_reduce_noisy.idx")
    B, k = idx.shape
    sd, row_ids = _noise_keys(seed, row_ids, B, "gather_reduce_noisy")
    a, wa, wb = None, 0.0, 0.0
    if mix is not None:
        a, wa, wb = mix
        a = _f32c(a, "gather_reduce_noisy.a")
        if tuple(a.shape) != (B, v.shape[1]):
            raise RagraphNativeError(f"gather_reduce_noisy: a is {tuple(a.shape)}, the reduction [{B}, {v.shape[1]}]")
    out = torch.empty((B, v.shape[1]), dtype=torch.float32, device=v.device)
    mean_l = None
    C = 0
    if labels is not None:
        labels = _f32c(labels, "gather_reduce_noisy.labels")
        C = labels.shape[1]
        mean_l = torch.empty((B, C), dtype=torch.float32, device=v.device)
    N.check(L.ragraph_gather_reduce_noisy_f32(v.data_ptr(), v.shape[1], _ptr(labels), C, v.shape[0], idx.data_ptr(), B, k,
                                              int(idx_base), float(v_scale), sd.data_ptr(), _ptr(row_ids), int(row_base), int(m),
                                              int(v.shape[0] if noise_n is None else noise_n), _ptr(a), float(wa), float(wb),
                                              out.data_ptr(), _ptr(mean_l), _stream()), "gather_reduce_noisy")
    return out, mean_l


def add_normal_noise(x: torch.Tensor | None, std: float, seed: torch.Tensor, row_ids: torch.Tensor | None = None,
                     row_base: int = 0, shape=None) -> torch.Tensor:
    """x + std * z for x [B, J, D] (or [B, D]: J = 1), z standard normal by Box-Muller on the hash of (seed[0], row id of b,
    j, d) (ragraph_add_normal_noise_f32) -- what adding torch.normal(0, std, x.shape) is to the reference's graph flavours.
    x = None with shape = (B, J, D): the noise alone."""
    L = _ready()
    if x is None:
        if shape is None:
            raise RagraphNativeError("add_normal_noise: x or shape")
        shape = tuple(int(s) for s in shape)
    else:
        x = _f32c(x, "add_normal_noise.x")
        shape = tuple(x.shape)
    if len(shape) not in (2, 3):
        raise RagraphNativeError(f"add_normal_noise: [B, J, D] or [B, D], got {shape}")
    B, J, D = (shape[0], 1, shape[1]) if len(shape) == 2 else shape
    sd, row_ids = _noise_keys(seed, row_ids, B, "add_normal_noise")
    out = torch.empty(shape, dtype=torch.float32, device=sd.device)
    N.check(L.ragraph_add_normal_noise_f32(_ptr(x), B, J, D, float(std), sd.data_ptr(), _ptr(row_ids), int(row_base),
                                           out.data_ptr() if out.numel() else None, _stream()), "add_normal_noise")
    return out


def draw_noise_seed(device) -> torch.Tensor:
    """One int64 on the device generator (torch.manual_seed reproduces it; capturable: the generator's state is the graph's)."""
    return torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=device)


def check_noise_rng(value: str) -> str:
    if value not in ("host", "device"):
        raise ValueError(f"noise_rng: 'host' or 'device', not {value!r}")
    return value


class NoiseRng:
    """The `noise_rng` attribute of the retrieval classes: "host" unless an instance sets it; a value other than "host" or
    "device" raises ValueError where it is set."""

    def __get__(self, obj, owner=None):
        return "host" if obj is None else obj.__dict__.get("_noise_rng", "host")

    def __set__(self, obj, value):
        obj.__dict__["_noise_rng"] = check_noise_rng(value)


# ---- bank construction with the draws made on the device (csrc/bank.hip) -----------------------------------
BUILD_SEED_COLUMNS = 7
(BUILD_SEED_FEATURE_NOISE, BUILD_SEED_NODE_DROP, BUILD_SEED_EDGE_SLOT, BUILD_SEED_PICK, BUILD_SEED_ANCHOR,
 BUILD_SEED_VALUE_NOISE, BUILD_SEED_VALUE_DROP) = range(BUILD_SEED_COLUMNS)   # the columns of a build seed tensor


def draw_build_seeds(passes: int, device) -> torch.Tensor:
    """int64 [passes, BUILD_SEED_COLUMNS] on the device generator (as draw_noise_seed: torch.manual_seed reproduces it, nothing is
    read back): row v holds the seeds of pass v of one batch of bank construction, one column per kind of draw."""
    return torch.randint(0, 2 ** 62, (int(passes), BUILD_SEED_COLUMNS), dtype=torch.int64, device=device)


def _seed1(seed: torch.Tensor, what: str) -> torch.Tensor:
    sd = _idxc(seed, f"{what}.seed")
    if sd.numel() != 1:
        raise RagraphNativeError(f"{what}: seed must hold one int64, got {tuple(sd.shape)}")
    return sd


def edge_rewrite_csr(prob: torch.Tensor, graph_ptr: torch.Tensor, seed: torch.Tensor):
    """Augmentation.augment_adj for a block-diagonal batch (ragraph_edge_rewrite_csr): slot (i, j) of a graph is 1 with
    probability (p_i + p_j) / 2, decided by the hash of (seed[0], i, local j).  Returns (rowptr int64 [n+1], col int32 [nnz]
    ascending per row, val fp32 ones).  Two passes (count, then fill, hashing again) around ONE read-back of the kept total;
    nothing is sized by the node pairs.  A kept total of 2^31 or more raises."""
    L = _ready()
    p = _f32c(prob, "edge_rewrite_csr.prob").reshape(-1)
    gp = _idxc(graph_ptr, "edge_rewrite_csr.graph_ptr").reshape(-1)
    sd = _seed1(seed, "edge_rewrite_csr")
    n, G = p.numel(), gp.numel() - 1
    dev = p.device
    rowptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(2, dtype=torch.int64, device=dev)
    ws = _workspace(L.ragraph_edge_rewrite_workspace_bytes(n), dev)
    N.check(L.ragraph_edge_rewrite_csr(sd.data_ptr(), p.data_ptr(), gp.data_ptr(), G, n, rowptr.data_ptr(), status.data_ptr(),
                                       None, None, 0, ws.data_ptr(), ws.numel(), _stream()), "edge_rewrite_csr")
    nnz, overflow = status.tolist()
    if overflow:
        raise RagraphNativeError("edge_rewrite_csr: 2^31 or more slots kept (int32 columns and counts cannot hold them)")
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev)
    if nnz:
        N.check(L.ragraph_edge_rewrite_csr(sd.data_ptr(), p.data_ptr(), gp.data_ptr(), G, n, rowptr.data_ptr(), None,
                                           col.data_ptr(), val.data_ptr(), nnz, None, 0, _stream()), "edge_rewrite_csr")
    return rowptr, col, val


def multinomial_segments(prob: torch.Tensor, seg_ptr: torch.Tensor, S: int, seed: torch.Tensor) -> torch.Tensor:
    """torch.multinomial(prob, S, replacement=True) for every segment [seg_ptr[g], seg_ptr[g+1]) of prob
    (ragraph_multinomial_segments_i64): int64 [G, S] GLOBAL positions, -1 for a segment without weight.  Draw (g, s) is the
    hash of (seed[0], g, s) pushed through the inverse CDF of the integer weights (uint64)(min(p, 1) * 2^40)."""
    L = _ready()
    p = _f32c(prob, "multinomial_segments.prob").reshape(-1)
    sp = _idxc(seg_ptr, "multinomial_segments.seg_ptr").reshape(-1)
    sd = _seed1(seed, "multinomial_segments")
    n, G, S = p.numel(), sp.numel() - 1, int(S)
    out = torch.empty((max(G, 0), max(S, 0)), dtype=torch.int64, device=p.device)
    ws = _workspace(L.ragraph_multinomial_segments_workspace_bytes(n), p.device)
    N.check(L.ragraph_multinomial_segments_i64(sd.data_ptr(), p.data_ptr(), n, sp.data_ptr(), G, S, out.data_ptr(), ws.data_ptr(),
                                               ws.numel(), _stream()), "multinomial_segments")
    return out


def csr_induced_blocks(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, pick: torch.Tensor) -> torch.Tensor:
    """adj[pick_g][:, pick_g] of every graph (ragraph_csr_induced_blocks_f32): a CSR with ascending columns per row and pick
    int64 [G, S] global ids (repeats allowed) -> dense fp32 [G, S, S]."""
    L = _ready()
    rp = _idxc(rowptr, "csr_induced_blocks.rowptr")
    c = _idxc(col, "csr_induced_blocks.col", torch.int32)
    v = _f32c(val, "csr_induced_blocks.val")
    pk = _idxc(pick, "csr_induced_blocks.pick")
    if pk.dim() != 2:
        raise RagraphNativeError(f"csr_induced_blocks: pick must be [G, S], got {tuple(pk.shape)}")
    G, S = pk.shape
    nnz = c.numel()
    out = torch.empty((G, S, S), dtype=torch.float32, device=pk.device)
    N.check(L.ragraph_csr_induced_blocks_f32(rp.data_ptr(), c.data_ptr() if nnz else None, v.data_ptr() if nnz else None,
                                             rp.numel() - 1, nnz, pk.data_ptr(), G, S, out.data_ptr(), _stream()),
            "csr_induced_blocks")
    return out


def blocks_to_csr(blocks: torch.Tensor):
    """Dense [G, S, S] blocks, S <= 64 -> the block-diagonal CSR over G * S rows (ragraph_blocks_to_csr_f32): (rowptr int64
    [G*S+1], col int32, val fp32), the non-zeros in row-major order.  Reads the entry count back, nothing else."""
    L = _ready()
    b = _f32c(blocks, "blocks_to_csr.blocks")
    if b.dim() != 3 or b.shape[1] != b.shape[2]:
        raise RagraphNativeError(f"blocks_to_csr: blocks must be [G, S, S], got {tuple(b.shape)}")
    G, S = b.shape[0], b.shape[1]
    dev = b.device
    rowptr = torch.empty(G * S + 1, dtype=torch.int64, device=dev)
    col = torch.empty(G * S * S, dtype=torch.int32, device=dev)
    val = torch.empty(G * S * S, dtype=torch.float32, device=dev)
    nnz = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _workspace(L.ragraph_blocks_to_csr_workspace_bytes(G, S), dev)
    N.check(L.ragraph_blocks_to_csr_f32(b.data_ptr(), G, S, rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), nnz.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _stream()), "blocks_to_csr")
    m = int(nnz.item())
    return rowptr, col[:m], val[:m]


def augment_features(x: torch.Tensor, prob: torch.Tensor, seed_drop: torch.Tensor, seed_noise: torch.Tensor,
                     rate: float = 0.01, std: float = 0.1, row_ids: torch.Tensor | None = None, row_base: int = 0) -> torch.Tensor:
    """Augmentation.augment_features (ragraph_augment_features_f32): row i of x [n, D] survives with probability prob[i] * rate
    -- the hash of (seed_drop[0], id of i) -- as x + std * z, z the normals of add_normal_noise(x, std, seed_noise, ...) for
    that id; every other row is +0.  row_ids int64 [n] / row_base: the ids, as in the noise entries."""
    L = _ready()
    x = _f32c(x, "augment_features.x")
    if x.dim() != 2:
        raise RagraphNativeError(f"augment_features: x must be [n, D], got {tuple(x.shape)}")
    n, D = x.shape
    p = _f32c(prob, "augment_features.prob").reshape(-1)
    if p.numel() != n:
        raise RagraphNativeError(f"augment_features: {p.numel()} probabilities for {n} rows")
    sd, row_ids = _noise_keys(seed_drop, row_ids, n, "augment_features")
    sn = _seed1(seed_noise, "augment_features")
    out = torch.empty_like(x)
    N.check(L.ragraph_augment_features_f32(x.data_ptr() if n else None, n, D, p.data_ptr() if n else None, float(rate), float(std),
                                           sd.data_ptr(), sn.data_ptr(), _ptr(row_ids), int(row_base),
                                           out.data_ptr() if n else None, _stream()), "augment_features")
    return out


def check_build_rng(value: str) -> str:
    if value not in ("host", "device"):
        raise ValueError(f"build_rng: 'host' or 'device', not {value!r}")
    return value


class BuildRng:
    """The `build_rng` attribute of the classes that build a bank: "host" unless an instance sets it; a value other than
    "host" or "device" raises ValueError where it is set."""

    def __get__(self, obj, owner=None):
        return "host" if obj is None else obj.__dict__.get("_build_rng", "host")

    def __set__(self, obj, value):
        obj.__dict__["_build_rng"] = check_build_rng(value)
