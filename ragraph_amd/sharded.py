"""Key-bank sharding across the GPUs of one node: one process per GPU, torch.distributed (backend "nccl" = RCCL over
xGMI on ROCm; "gloo" in the CPU tests).  The reference is single-GPU (no collective call exists in it).

Partition: rank r owns bank rows [base_r, base_r + N_r).  Per retrieve:
  1. every rank runs the fused cosine+top-k kernel on ITS shard with idx_base = base_r      -> [B,k] scores + global ids
  2. ONE all_gather of the (B,k) score and id tensors (B*k*12 bytes per rank: latency-bound, single hop on the
     fully connected xGMI mesh)                                                               -> [G,B,k]
  3. every rank merges the G lists with the canonical order (score desc, id asc)            -> identical on all ranks,
     and identical to the 1-GPU result bit for bit (scores are shard-independent fmaf chains)
  4. values / labels: either REPLICATED on every rank (default in bench.py: 1 GB at 1M x 256 -- nothing next to 288 GB
     of HBM -- so sum_k V[idx], mean_k L[idx] are local gathers, bit-identical to 1 GPU, and the all_gather of step 2 is
     the only collective), or row-sharded like the keys: every rank sums the winners IT owns and one all_reduce(sum)
     of [B, D+C] finishes it (no [B,k,D] traffic; sums then differ from 1 GPU by fp32 re-association, <= 1e-6 rel).
Indices and scores are exact for any G.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from ._native import TOPK_MAX, RagraphNativeError


# ---- collectives ------------------------------------------------------------------------------------------------------
# RCCL ("nccl") moves device tensors directly.  Under "gloo" (CPU tests; two ranks sharing ONE GPU in
# tests/test_gpu_two_rank.py -- RCCL refuses two ranks on one device) device tensors are staged through the host: the
# collective itself then runs on CPU copies, and the device work enqueued before it has completed (the copy to the host
# synchronises the stream), which is exactly the ordering the exchange callback of the filtered call relies on.
def _staged(group, *tensors) -> bool:
    return dist.get_backend(group) == "gloo" and any(t.is_cuda for t in tensors)


class CollectiveTimes:
    """Optional per-collective timing (bench.py, N > 1): while enabled, every collective of this module is bracketed by
    events on the current stream (the stream the collective is ordered on); ms() sums them per kind after a synchronise."""

    def __init__(self):
        self.enabled = False
        self.events = {}   # kind -> [(start, end, bytes)]

    def start(self, kind: str, tensor: torch.Tensor):
        if not (self.enabled and tensor.is_cuda):
            return None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.events.setdefault(kind, []).append((e0, e1, tensor.numel() * tensor.element_size()))
        return e1

    def report(self) -> dict:
        torch.cuda.synchronize()
        return {kind: {"calls": len(ev), "ms": round(sum(a.elapsed_time(b) for a, b, _ in ev), 4),
                       "MB": round(sum(n for _, _, n in ev) / 1e6, 3)} for kind, ev in self.events.items()}

    def reset(self):
        self.events = {}


collective_times = CollectiveTimes()

# Optional progress hook (bench.py, N > 1): a callable taking one short string, called BEFORE every collective of this module
# and at every exchange of a filtered retrieval -- a rank that hangs in a collective (a peer that diverged, a dead link) has
# then named the phase it is waiting in (bench.py writes it to a per-rank heartbeat file that its watchdog prints).
heartbeat = None


def _beat(what: str) -> None:
    if heartbeat is not None:
        heartbeat(what)


def all_gather_into(out: torch.Tensor, inp: torch.Tensor, group=None) -> None:
    _beat(f"all_gather {tuple(out.shape)}")
    end = collective_times.start("all_gather", out)
    if _staged(group, out, inp):
        host = torch.empty(out.shape, dtype=out.dtype)
        dist.all_gather_into_tensor(host, inp.cpu().contiguous(), group=group)
        out.copy_(host)
    else:
        dist.all_gather_into_tensor(out, inp, group=group)
    if end is not None:
        end.record()


def all_to_all_single(out: torch.Tensor, inp: torch.Tensor, recv, send, group=None) -> None:
    _beat(f"all_to_all {tuple(out.shape)}")
    end = collective_times.start("all_to_all", out)
    if _staged(group, out, inp):
        host = torch.empty(out.shape, dtype=out.dtype)
        dist.all_to_all_single(host, inp.cpu().contiguous(), recv, send, group=group)
        out.copy_(host)
    else:
        dist.all_to_all_single(out, inp, recv, send, group=group)
    if end is not None:
        end.record()


def all_reduce(t: torch.Tensor, op, group=None) -> None:
    _beat(f"all_reduce {tuple(t.shape)}")
    end = collective_times.start("all_reduce", t)
    if _staged(group, t):
        host = t.cpu()
        dist.all_reduce(host, op=op, group=group)
        t.copy_(host)
    else:
        dist.all_reduce(t, op=op, group=group)
    if end is not None:
        end.record()


def shard_bounds(N: int, world: int, rank: int):
    """Contiguous, balanced row ranges: the first N % world ranks hold one extra row."""
    q, r = divmod(N, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


class QueryShard:
    """The other way to use G GPUs: the bank (1 GB at 1M x 256 -- nothing next to 288 GB of HBM) is REPLICATED and the
    batch of queries is split, rank r answering rows shard_bounds(B, G, r).  Queries are independent, so there is no
    data-path collective at all; the only exchange is the all_gather of the per-query results (C logits per node),
    which every rank needs only if it wants the whole output.  Results are those of one GPU bit for bit (a score does
    not depend on the query batch).  Key sharding (ShardedToyGraphBase) is for banks that should not be replicated."""

    def __init__(self, group=None, force_collectives: bool = False):
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.collective = self.world > 1 or (force_collectives and dist.is_initialized())

    def bounds(self, B: int):
        return shard_bounds(B, self.world, self.rank)

    def gather_rows(self, local: torch.Tensor, B: int) -> torch.Tensor:
        """[hi-lo, C] per rank -> [B, C] on every rank (rows in query order).  Ranks hold ceil or floor(B / G) rows:
        padded to the larger size for one all_gather_into_tensor, then the padding rows are dropped."""
        if not self.collective:
            return local
        per = -(-B // self.world)
        lo, hi = self.bounds(B)
        buf = local
        if hi - lo < per:
            buf = torch.cat([local, local.new_zeros((per - (hi - lo),) + tuple(local.shape[1:]))], 0)
        out = local.new_empty((self.world * per,) + tuple(local.shape[1:]))
        all_gather_into(out, buf.contiguous(), self.group)
        if self.world * per == B:
            return out
        parts = []
        for r in range(self.world):
            a, b = shard_bounds(B, self.world, r)
            parts.append(out[r * per: r * per + (b - a)])
        return torch.cat(parts, 0)


class HybridLayout:
    """G = Q x S ranks: rank r = q * S + s holds KEY shard s of S and answers QUERY group q of Q -- the layout between the
    two pure ones (S = G: key-sharded, every rank scores all queries against 1 / G of the keys and takes part in G-wide
    exchanges at every phase; S = 1: query-sharded, bank replicated, no exchange).  With S = 2 at G = 8 a rank scores a
    quarter of the queries against half of the keys and has ONE exchange partner: [B / Q, m] bound exchanges and one
    all_to_all of its group's lists with that partner, then the tail on B / G rows; two all_gathers of [., C] outputs (key
    group, then query axis) complete the step.  Every result row is the single-GPU row bit for bit: a score depends neither
    on the query batch nor on the shard (include/ragraph_hip.h, numerics contract).

    Two families of process groups are created here -- by EVERY rank, in the same order (torch.distributed.new_group is a
    collective over the default group): `key_group` = the S ranks of my query group (ShardedToyGraphBase's group),
    `query_group` = the Q ranks that hold my key shard (QueryShard's group for the final gather)."""

    def __init__(self, key_shards: int, timeout=None):
        if not dist.is_initialized():
            raise RuntimeError("HybridLayout: torch.distributed is not initialised")
        world, rank = dist.get_world_size(), dist.get_rank()
        if key_shards < 1 or world % key_shards:
            raise ValueError(f"HybridLayout: {key_shards} key shards do not divide {world} ranks")
        self.S, self.Q = int(key_shards), world // int(key_shards)
        self.q, self.s = divmod(rank, self.S)
        kw = {} if timeout is None else {"timeout": timeout}
        key_groups = [dist.new_group([qq * self.S + ss for ss in range(self.S)], **kw) for qq in range(self.Q)]
        query_groups = [dist.new_group([qq * self.S + ss for qq in range(self.Q)], **kw) for ss in range(self.S)]
        self.key_group, self.query_group = key_groups[self.q], query_groups[self.s]
        self.name = f"hybrid {self.Q}x{self.S} (query groups x key shards)"

    def key_rows(self, N: int):
        """Bank rows of my key shard."""
        return shard_bounds(N, self.S, self.s)

    def query_shard(self) -> "QueryShard":
        return QueryShard(self.query_group, force_collectives=True)

    # The entry points for (query shard, bank of my key group).  qs = None is the layout with ONE query group: pure key sharding.
    @staticmethod
    def rows(qs: "QueryShard", tgb: "ShardedToyGraphBase", B: int):
        """(qlo, qhi, lo, hi): my query group answers rows [qlo, qhi) of the batch, and within the group I finish rows
        [qlo + lo, qlo + hi)."""
        qlo, qhi = (0, B) if qs is None else qs.bounds(B)
        lo, hi = tgb.tail_bounds(qhi - qlo)
        return qlo, qhi, lo, hi

    @staticmethod
    def _group_queries(qs, search_keys):
        if qs is None:
            return search_keys
        qlo, qhi = qs.bounds(search_keys.shape[0])
        return search_keys[qlo:qhi].contiguous()

    @staticmethod
    def retrieve_reduced_rows(qs: "QueryShard", tgb: "ShardedToyGraphBase", search_keys, k=None, defer_verify: bool = False):
        """(sum_k V[idx], mean_k L[idx], idx) of MY rows of the batch: my group's slice of the queries against the group's
        key shards (exchanges and the all_to_all stay inside the key group)."""
        return tgb.retrieve_reduced_rows(HybridLayout._group_queries(qs, search_keys), k, defer_verify=defer_verify)

    @staticmethod
    def retrieve_rows_with_tail(qs: "QueryShard", tgb: "ShardedToyGraphBase", search_keys, tail, k=None):
        """tail(sum_k V[idx], mean_k L[idx]) of MY rows of the batch, proven (ShardedToyGraphBase.retrieve_rows_with_tail: the
        speculative first bound is decided, proven and withdrawn inside the KEY group, and the verdict is read before any
        collective of the query axis, so the query groups never disagree on how many of those run)."""
        return tgb.retrieve_rows_with_tail(HybridLayout._group_queries(qs, search_keys), tail, k)

    @staticmethod
    def gather_output_rows(qs: "QueryShard", tgb: "ShardedToyGraphBase", local: torch.Tensor, B: int) -> torch.Tensor:
        """[hi - lo, C] per rank -> [B, C] on every rank: the key group's rows first, then the query groups' slices."""
        if qs is None:
            return tgb.gather_output_rows(local, B)
        qlo, qhi = qs.bounds(B)
        return qs.gather_rows(tgb.gather_output_rows(local, qhi - qlo), B)


class GroupPrior:
    """The speculative first bound of a row-sharded bank's filtered calls: ONE decision per call for the whole group of ranks.
    Every rank keeps this object and feeds it the same numbers -- the pooled statistics of each call (all_reduce MAX of
    [misses, -lowest, highest merged k-th best, candidates per query, overflowed lists]) --, so every rank derives the same
    prior, withdraws it at the same call and re-probes at the same call: the number of exchanges of a call (the prior removes
    phase 0) can never differ between ranks.  The policy is KeyIndex's (ragraph_amd/kernels_index.py), on a clock of calls:
    warm after WARM_CALLS calls with a bound pass, prior = lowest seen - max(MARGIN x spread, MIN_MARGIN); a call that reports a
    miss, overflowed lists or a flood of candidates withdraws it for `after` calls (a failed re-probe quadruples that)."""
    WARM_CALLS = 2
    MARGIN = 0.5
    MIN_MARGIN = 0.01
    HISTORY = 16
    REPROBE_CALLS = 64
    MAX_CANDIDATES = 1.5
    MIN_BATCH = 17

    def __init__(self, enabled: bool = True):
        import os
        self.enabled = enabled and os.environ.get("RAGRAPH_SPEC", "1") != "0"
        self.forced = None            # tests: a prior to use whatever the history says (None: the policy)
        self._st = {}
        self.calls = 0                # the clock: filtered calls of the group so far
        self.used = self.missed_calls = 0

    def _state(self, k):
        st = self._st.get(k)
        if st is None:
            st = self._st[k] = {"hist": [], "off_at": None, "after": self.REPROBE_CALLS, "cand": None, "probed_at": None}
        return st

    def prior_for(self, B: int, k: int):
        if self.forced is not None:
            return float(self.forced)
        if not self.enabled or B < self.MIN_BATCH:
            return None
        st = self._state(k)
        if st["off_at"] is not None:
            if self.calls - st["off_at"] < st["after"]:
                return None
            st["off_at"] = None
            st["probed_at"] = self.calls
        if len(st["hist"]) < self.WARM_CALLS:
            return None
        lo = min(h[0] for h in st["hist"])
        hi = max(h[1] for h in st["hist"])
        return lo - max(self.MARGIN * (hi - lo), self.MIN_MARGIN)

    def record(self, k: int, speculative: bool, misses: int, lo: float, hi: float, cand: float, lists_over: int) -> bool:
        """One call's pooled statistics.  Returns True when the call's result stands (no query missed the prior)."""
        self.calls += 1
        st = self._state(k)
        have = lo <= hi and lo != float("inf")
        if lists_over:
            st["hist"] = []
        elif have and not (speculative and misses):
            st["hist"].append((lo, hi))
            del st["hist"][:-self.HISTORY]
        if not speculative:
            if cand >= 0 and not lists_over:
                st["cand"] = cand
            return True
        self.used += 1
        loose = cand >= 0 and st["cand"] is not None and cand > self.MAX_CANDIDATES * max(st["cand"], 32.0)
        if misses or loose or lists_over:
            if st["probed_at"] is not None and self.calls - st["probed_at"] < st["after"]:
                st["after"] = min(st["after"] * 4, 1 << 40)
            st["off_at"] = self.calls
            if misses:
                st["hist"] = []
                self.missed_calls += 1
        return misses == 0


class ShardedToyGraphBase:
    """Retrieval over a row-sharded bank.  `ops` supplies the five kernels (default: ragraph_amd.kernels, i.e. the HIP
    library); the CPU tests inject an oracle-backed object to exercise the collective logic under gloo."""

    def __init__(self, keys, values, labels, idx_base: int, retrieve_num: int, group=None, ops=None,
                 force_collectives: bool = False, values_replicated: bool = False, emulate_world: int = 0,
                 plan_n: int = 0):
        """keys: this rank's key rows.  values/labels: this rank's rows (values_replicated=False) or the WHOLE bank's
        (values_replicated=True).  plan_n: the largest shard's row count (default: all_reduce MAX of the shard sizes).
        emulate_world = G (single process, TIMING ONLY): behave as rank 0 of a G-rank job whose other shards look like
        this one -- the exchanges use this shard's numbers G times; results are not the global top-k."""
        if ops is None:
            from . import kernels as ops  # the HIP library; raises loudly without a GPU
        self.ops = ops
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.idx_base = int(idx_base)
        self.values_replicated = values_replicated
        # run the collectives even in a 1-rank group (exercises the RCCL path on a single-GPU box)
        self.collective = self.world > 1 or (force_collectives and dist.is_initialized())
        self.retrieve_num = retrieve_num
        self.resource_keys, self.resource_values, self.resource_labels = keys, values, labels
        self.keys_normalized = ops.normalize_rows(keys)
        from .kernels_index import KeyIndex  # torch-only helper: copies for the faster kernels, made on first use
        self._index = KeyIndex(self.keys_normalized, ops)
        self.emulate_world = int(emulate_world)
        self.n_shards = self.emulate_world if self.emulate_world > 1 else self.world   # the shard count of the exchanges
        self.exchanges = self.collective or self.emulate_world > 1                     # does this bank exchange at all?
        self._out_shard = None
        self.exchange_count = {}   # phase -> how many exchanges of that phase this rank has taken part in (diagnostic)
        self.prior = GroupPrior()  # the speculative first bound: one decision per call for the whole group
        self._pending = None       # (pinned words, event, k, speculative) of a call whose verdict confirm() has not read yet
        self.reruns = 0            # calls repeated without the prior because a query missed it (diagnostic)

        def exchange_fn(phase, theta, scores):
            return self._exchange(phase, theta, scores)

        exchange_fn.n_shards = self.n_shards
        self._exchange_fn = exchange_fn
        # rows this shard SEARCHES: its unique rows when KeyIndex collapses exact duplicates (the reference's bank recipe stores
        # most rows many times over; every shard judges its own rows) -- plan_n is the largest of those over the ranks
        n_local = self._index.search_rows(min_unique=64)
        if plan_n:
            self.plan_n = max(int(plan_n), n_local) if n_local != int(keys.shape[0]) else int(plan_n)
        elif self.collective:
            t = torch.tensor([n_local], dtype=torch.int64, device=keys.device)
            all_reduce(t, dist.ReduceOp.MAX, group)
            self.plan_n = int(t.item())
        else:
            self.plan_n = n_local

    # ---- the exchanges of a filtered retrieval over the sharded bank (kernels.topk_cosine_filtered) ---------------------
    def _exchange(self, phase: int, theta, scores):
        """theta [B]: this shard's lower bound of every query's final k-th best score -> a bound over ALL shards.
        Every phase alike: `scores` [B, k] holds (descending) lower bounds of the exact scores of k distinct keys of this
        shard -- after the bound pass the parts' best approximate scores minus eps, after a level the running exact
        top-k -- and the k-th largest of the union of every shard's best m = 2 ceil(k / G) of them is a lower bound of
        the global k-th best (k-th of a subset): one all_gather of [B, m] scores, 4 m B per query and rank, + a k-th
        selection over [B, G m] (theta_sharpen).  Because phase 0 pools the shards' samples, each shard scans only 1 / G
        of the prefix (n_shards below)."""
        if not self.exchanges:
            return
        G = self.n_shards
        self.exchange_count[phase] = self.exchange_count.get(phase, 0) + 1
        _beat(f"exchange phase {phase} (#{self.exchange_count[phase]})")
        k = scores.shape[1]
        m = min(k, 2 * (-(-k // G)))
        while G * m > 64 and m > -(-k // G):
            m -= 1
        self.ops.theta_sharpen(self._gather_shards(scores[:, :m].contiguous()), theta, k)

    def _gather_shards(self, t, rows=None):
        """[B, m] of this shard -> [G, n, m] (shard-major): every shard's rows of ALL queries on every rank (rows None: one
        all_gather), or of MY rows (lo, hi) of the batch (one all_to_all: a rank receives its rows from every shard)."""
        G, (B, m) = self.n_shards, t.shape
        lo, hi = rows or (0, B)
        if self.emulate_world > 1:   # (timing only: this shard's numbers stand in for the other shards')
            return t[lo:hi].unsqueeze(0).expand(G, hi - lo, m).contiguous()
        out = torch.empty((G * (hi - lo), m), dtype=t.dtype, device=t.device)
        if rows is None:
            all_gather_into(out, t, self.group)
        else:
            send = [b - a for a, b in (shard_bounds(B, G, r) for r in range(G))]   # rows of my lists that go to rank r
            all_to_all_single(out, t, [hi - lo] * G, send, self.group)
        return out.view(G, hi - lo, m)

    def _merge(self, s, i, rows=None):
        """This shard's lists [B, k] -> (scores, idx, merged scores) of `rows` of the batch (_gather_shards): the group's lists
        in the canonical order, and the scores on which the verdict on a prior is taken.  Shards that cannot hold k winners of a
        query pad with sentinels that lose every comparison (-inf, INT64_MAX)."""
        ms, mi = self.ops.topk_merge(self._gather_shards(s.contiguous(), rows), self._gather_shards(i.contiguous(), rows))
        if self.emulate_world > 1:
            # (timing only: the merge launch of a real rank, whose verdict is taken on what it returns -- a shard's own list
            # under the pooled bound is far shorter than k --; the rows handed out are this shard's)
            lo, hi = rows or (0, s.shape[0])
            return s[lo:hi].contiguous(), i[lo:hi].contiguous(), ms
        return ms, mi, ms

    # ---- the speculative first bound of a sharded call: chosen, proven and withdrawn by the whole group ------------------
    @property
    def _stats_index(self):
        """The index whose statistics are read: the one the kernels stream (KeyIndex.search_index)."""
        return self._index.search_index

    def _choose_prior(self, B: int, k: int):
        """The prior of THIS call (None: a bound pass), the same on every rank: GroupPrior's state is fed pooled numbers
        only, and whether the shape speculates at all comes from the shared plan."""
        if not self._stats_index.sharded_speculates(B, k, self.plan_n, self.n_shards):
            return None
        return self.prior.prior_for(B, k)

    def _post_verify(self, merged_s, k: int, prior) -> None:
        """Behind the merge: this rank's rows' merged k-th best scores against the prior (a row is proven iff it reaches the
        prior; an all-zero query -- every score +0 -- is answered by index order and needs no proof), the smallest / largest of
        them, this shard's candidates per query and overflowed lists; ONE all_reduce MAX of five floats makes them the group's.
        The words travel to a pinned buffer behind an event: confirm() reads them."""
        speculative = prior is not None
        ix = self._stats_index
        native = getattr(self.ops, "verify_merged_prior", None)
        if native is not None and merged_s.is_cuda:   # one launch (csrc/topk_filter.hip: verify_merged_prior_kernel)
            st, ov = ix.last_stats, ix.last_over
            words = native(merged_s, prior, st if torch.is_tensor(st) else None, ov if torch.is_tensor(ov) else None)
        else:                                          # the same five numbers with torch ops (the CPU tests' oracle shim)
            kth, top = merged_s[:, k - 1], merged_s[:, 0]
            zero = (top == 0) & (kth == 0)
            ok = zero | (kth >= prior) if speculative else torch.ones_like(zero)
            live = ok & ~zero & (kth > float("-inf"))
            inf = torch.full_like(kth, float("inf"))
            none = torch.tensor(float("-inf"), device=merged_s.device)   # (a rank without rows of this batch)
            words = torch.stack([(~ok).sum().to(torch.float32),
                                 -torch.where(live, kth, inf).min() if kth.numel() else none,
                                 torch.where(live, kth, -inf).max() if kth.numel() else none,
                                 self._cand_per_query(merged_s.device), self._lists_over(merged_s.device)])
        if self.collective:
            all_reduce(words, dist.ReduceOp.MAX, self.group)
        if words.is_cuda:
            if getattr(self, "_host_words", None) is None:
                self._host_words = torch.zeros(5, dtype=torch.float32).pin_memory()
                self._event = torch.cuda.Event()
            self._host_words.copy_(words, non_blocking=True)
            self._event.record()
            self._pending = (self._host_words, self._event, k, speculative)
        else:
            self._pending = (words, None, k, speculative)

    def _cand_per_query(self, device):
        st = self._stats_index.last_stats
        if st is None or not torch.is_tensor(st) or st.numel() < 8:
            return torch.tensor(-1.0, device=device)
        w = st[:8].to(torch.float32)
        return (w[2:5] / w[5:8].clamp(min=1.0)).sum()

    def _lists_over(self, device):
        ov = self._stats_index.last_over
        if ov is None or not torch.is_tensor(ov):
            return torch.tensor(0.0, device=device)
        return ov.reshape(-1)[0].to(device=device, dtype=torch.float32)

    def confirm(self) -> bool:
        """The pooled verdict on the last sharded call: True = its result stands.  False = a query's merged k-th best fell
        below the speculative prior somewhere in the group: EVERY rank sees the same words, withdraws the prior and repeats
        the call with no_prior=True (topk / topk_rows / retrieve_rows_with_tail do that themselves; a caller that asked
        topk_rows to defer the verdict must)."""
        p = self._pending
        if p is None:
            return True
        self._pending = None
        if p[1] is not None:
            p[1].synchronize()
        w = [float(x) for x in p[0].tolist()]
        if self.emulate_world > 1:
            w[0] = 0.0   # (timing only: the same launches, no verdict -- an emulated rank's lists are one shard's, not the group's)
        ok = self.prior.record(p[2], p[3], int(w[0]), -w[1], w[2], w[3], int(w[4]))
        if not ok:
            self.reruns += 1
        return ok

    def _topk(self, search_keys, k, own_rows: bool, defer: bool = False, no_prior: bool = False):
        """THE sharded call: the group's canonical top-k of all queries on every rank, or (own_rows) of this rank's rows of the
        batch.  Where the shards exchange bounds it may run under the group's speculative first bound: choose the prior, run
        once, prove the merged rows; on a miss run once more with a bound pass (withdrawn on every rank alike) and prove that.
        defer: the first verdict is left to the caller's confirm().  no_prior: this call repeats one that missed."""
        if self._pending is not None:
            raise RagraphNativeError("ShardedToyGraphBase: the deferred verdict on the previous sharded call was never read -- "
                                     "its rows are unproven; call confirm() (and repeat the call with no_prior=True when it "
                                     "returns False) before the next call, or use retrieve_rows_with_tail")
        k = self.retrieve_num if k is None else k
        # The sharded merge (exchanges, topk_merge of the gathered lists) is written for the fused kernels' lists.  k is the
        # same on every rank, so every rank raises here, before any collective.
        if k > TOPK_MAX:
            raise RagraphNativeError(f"ShardedToyGraphBase: k={k} exceeds the sharded top-k limit of {TOPK_MAX} "
                                     "(TOPK_MAX); larger k needs an unsharded ToyGraphBase")
        q = search_keys.reshape(1, -1) if search_keys.dim() == 1 else search_keys
        B = q.shape[0]
        mine = self.tail_bounds(B) if own_rows else None
        kl = min(k, self.keys_normalized.shape[0])
        if not self.exchanges or kl < k:
            # no exchange, nothing to prove: the shard's exact list (a shard smaller than k pads with sentinels that lose every
            # comparison), merged over ALL rows where there is a group
            s, i = self._index.topk(q, kl, idx_base=self.idx_base, exchange=None, plan_n=self.plan_n, prior=None)
            if kl < k:
                pad_s = torch.full((B, k - kl), float("-inf"), dtype=s.dtype, device=s.device)
                pad_i = torch.full((B, k - kl), torch.iinfo(torch.int64).max, dtype=i.dtype, device=i.device)
                s, i = torch.cat([s, pad_s], 1), torch.cat([i, pad_i], 1)
            if self.exchanges:
                s, i, _ = self._merge(s, i)
            return (s[mine[0]:mine[1]].contiguous(), i[mine[0]:mine[1]].contiguous()) if own_rows else (s, i)

        def once(prior):
            s, i = self._index.topk(q, k, idx_base=self.idx_base, exchange=self._exchange_fn, plan_n=self.plan_n, prior=prior)
            s, i, merged = self._merge(s, i, mine)
            self._post_verify(merged, k, prior)
            return s, i

        out = once(None if no_prior else self._choose_prior(B, k))
        if not defer and not self.confirm():
            out = once(None)
            self.confirm()
        return out

    def topk(self, search_keys, k=None):
        """Global canonical top-k: (scores [B,k], idx [B,k]) identical on every rank."""
        return self._topk(search_keys, k, own_rows=False)

    # ---- key-sharded bank, query-sharded tail -----------------------------------------------------------------------
    # Everything behind the per-shard filter is per query: merge, value / label gather, fusion, decoder.  With the
    # values replicated, rank r finishes only rows shard_bounds(B, G, r) of the batch: the per-shard lists travel by ONE
    # all_to_all (a rank receives its rows' lists from every shard: B k 12 (G - 1) / G bytes instead of the all_gather's
    # B k 12 (G - 1)), the merge, the gathers and the decoder run on B / G rows, and one all_gather of the [B, C] outputs
    # (RAGraph.forward) completes the step.  Same bits as the replicated tail: every step is per row.
    def tail_bounds(self, B: int):
        return shard_bounds(B, self.n_shards, 0 if self.emulate_world > 1 else self.rank)

    def topk_rows(self, search_keys, k=None, defer_verify: bool = False, no_prior: bool = False):
        """Global canonical top-k of THIS RANK'S rows of the batch: (scores, idx) [hi - lo, k], (lo, hi) = tail_bounds.
        defer_verify: the caller enqueues more work first and calls confirm() itself before it hands out anything -- when that
        returns False it repeats this call with no_prior=True (retrieve_rows_with_tail is that protocol; the next sharded call
        raises while the verdict is unread)."""
        return self._topk(search_keys, k, own_rows=True, defer=defer_verify, no_prior=no_prior)

    def retrieve_reduced_rows(self, search_keys, k=None, defer_verify: bool = False, no_prior: bool = False):
        """(sum_k V[idx], mean_k L[idx], idx) for this rank's rows of the batch (values replicated)."""
        if not self.values_replicated:
            raise ValueError("retrieve_reduced_rows: needs the values / labels replicated on every rank")
        _, idx = self.topk_rows(search_keys, k, defer_verify=defer_verify, no_prior=no_prior)
        sum_v, mean_l = self.ops.gather_reduce(self.resource_values, self.resource_labels, idx)
        return sum_v, mean_l, idx

    def retrieve_rows_with_tail(self, search_keys, tail, k=None):
        """tail(sum_k V[idx], mean_k L[idx]) for this rank's rows of the batch -- `tail` maps the rank's retrieved rows to its
        output rows (RAGraph: fusion + decoder).  The filtered call may run under the group's speculative first bound: its
        proof -- the merged k-th best of every row against the prior, pooled over the ranks -- is read AFTER the tail has been
        enqueued, just before the output leaves; a miss anywhere repeats retrieval and tail without the prior on every rank
        alike.  What this returns is proven."""
        sum_v, mean_l, _ = self.retrieve_reduced_rows(search_keys, k, defer_verify=True)
        try:
            out = tail(sum_v, mean_l)
        except BaseException:
            self._pending = None   # (no row leaves: nothing to prove)
            raise
        if not self.confirm():
            sum_v, mean_l, _ = self.retrieve_reduced_rows(search_keys, k, no_prior=True)
            out = tail(sum_v, mean_l)
        return out

    def gather_output_rows(self, local: torch.Tensor, B: int) -> torch.Tensor:
        """[hi - lo, C] per rank -> [B, C] on every rank (QueryShard.gather_rows over this bank's group)."""
        if self.emulate_world > 1 or not self.collective:
            return local
        if self._out_shard is None:
            self._out_shard = QueryShard(self.group, force_collectives=True)
        return self._out_shard.gather_rows(local, B)

    def retrieve_reduced(self, search_keys, k=None):
        """(sum_k V[idx], mean_k L[idx], idx) over the whole bank."""
        k = self.retrieve_num if k is None else k
        _, idx = self.topk(search_keys, k)
        if self.values_replicated:  # every winner's row is local: same kernel, same bits as a single GPU
            sum_v, mean_l = self.ops.gather_reduce(self.resource_values, self.resource_labels, idx)
            return sum_v, mean_l, idx
        sum_v, _ = self.ops.gather_reduce(self.resource_values, None, idx, idx_base=self.idx_base)
        sum_l, _ = self.ops.gather_reduce(self.resource_labels, None, idx, idx_base=self.idx_base)
        if self.collective:
            packed = torch.cat([sum_v, sum_l], dim=1)
            all_reduce(packed, dist.ReduceOp.SUM, self.group)
            sum_v, sum_l = packed[:, :sum_v.shape[1]].contiguous(), packed[:, sum_v.shape[1]:].contiguous()
        return sum_v, sum_l / float(k), idx  # label counts are small integers: exact sums, one rounded division

    def retrieve(self, search_keys, search_adj=None, add_noise=False):
        """Public (B,k,D)/(B,k,C) form of ToyGraphBase.retrieve: owner-gather + all_reduce (zeros elsewhere)."""
        _, idx = self.topk(search_keys, self.retrieve_num)
        if self.values_replicated:
            return self.ops.gather_rows(self.resource_values, idx), self.ops.gather_rows(self.resource_labels, idx)
        e = self.ops.gather_rows(self.resource_values, idx, idx_base=self.idx_base)
        l = self.ops.gather_rows(self.resource_labels, idx, idx_base=self.idx_base)
        if self.collective:
            all_reduce(e, dist.ReduceOp.SUM, self.group)
            all_reduce(l, dist.ReduceOp.SUM, self.group)
        return e, l
