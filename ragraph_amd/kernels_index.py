"""Bank-side dispatch of the exact top-k (torch only: importable on a CPU box for the gloo tests)."""
from __future__ import annotations

import math
import os

import torch

from . import filter_stats as FS
from ._native import TOPK_FILTER_MAX, TOPK_MAX, TOPK_ORDERED_MAX, RagraphNativeError

# The kernel paths KeyIndex._route names (SLAB: plain ops.topk_cosine), and the filtered entries of one bank
# by list length: (longest list, route, the ops' rule that says where it pays -- None: asked before the bank's clock moves).
ROUTES = (SLAB, PACKED, FUSED, SMALL, FILTERED, WIDE, WIDE128, SHARDED, COLLAPSED, SLABS_OF_FILTERED) = (
    "SLAB", "PACKED", "FUSED", "SMALL", "FILTERED", "WIDE", "WIDE128", "SHARDED", "COLLAPSED", "SLABS_OF_FILTERED")
FILTERED_BY_K = ((32, FILTERED, "filter_helps"), (TOPK_MAX, WIDE, "filter_wide_helps"), (TOPK_FILTER_MAX, WIDE128, None))


class KeyIndex:
    """One bank on the device: the normalised keys plus the copies the faster kernels stream (packed fp32 for
    the LDS-DMA ring, bf16 for the filter), made on first use, and the dispatch to the fastest exact top-k for a batch.
    `ops` supplies the kernels (default: this module); an object without the optional entries (the CPU tests' oracle
    shim) simply always takes topk_cosine.

    A bank that grows (extend) is a SEALED part -- the rows the copies, the duplicate groups and the int8 verdict were made
    from -- and a short TAIL of rows appended since: topk searches the sealed rows exactly as it would a bank of only those
    rows, then continues the finished lists over the tail (ops.topk_cosine_tail: the same fmaf chains, the same canonical
    order, so the bits of one search over all rows).  seal() folds the tail in: it drops what was derived from the ROWS and
    keeps what was learnt from the QUERIES (priors, demotions, re-probe clocks).  DESIGN.md section 4.19.

    A bank that shrinks (retire) keeps its physical rows and marks the rows taken out in a bitmap: topk searches for k +
    retired_rows keys exactly as above and drops the retired entries from the finished lists (ops.topk_drop_rows) -- the bits
    of a fresh index over the live rows.  rebase() is the owner's word that the rows themselves changed (a compaction).
    DESIGN.md section 4.21."""

    MAX_FILTERED_BATCH = 262144
    # int8 levels only for banks whose int8 copy is accurate enough: max |dk| of the dequantised rows.  Gaussian-like unit
    # rows of 256 elements give 0.015 (eps ~ 0.022, ~3x the bf16 candidates: pays); the error grows
    # with the bank's largest entry (ONE scale for all keys), and a bank with a one-hot row reaches 0.036 -- thousands of
    # candidates per query.  Above this the levels stay on bf16; a bank that still overflows on int8 is caught by
    # _poll_overflow.
    I8_MAX_ERR = 0.02
    OVERFLOW_FRACTION = 1.0 / 64   # of a call of >= 64 queries sent to the exact scan: the filter (level dtype) costs more than it saves
    # Exact duplicates (the reference's bank recipe stores three of four rows as copies of ONE vector, ToyGraphBase.py:91-119
    # + Augmentation.py:9-20; the sampled rows repeat as well, :98 replacement=True): banks of at least DEDUP_MIN_ROWS rows
    # are grouped once per bank version (hash + sort + bit-wise compare on the device, one synchronisation), and when at
    # most DEDUP_MAX_UNIQUE of the rows are unique -- or one row is stored more than DEDUP_MAX_GROUP times: every query
    # next to it would fill its candidate list with copies -- the search runs over the unique rows (their own copies,
    # their own dispatch) and the winners are expanded to bank rows in canonical order: the same bits.
    # Candidates per query the int8 levels of a call may pass (sampled by the call itself, read back asynchronously): an int8
    # level saves ~0.2 ps of matrix time per (query, key) against bf16 and passes ~3x the candidates at ~0.25 ns each, so
    # 2/3 of its candidates must stay below ~0.8e-3 x its keys; with a floor for short levels.  A bank beyond that is
    # slower on int8 than on bf16 although nothing overflows (near-duplicate clusters of a few hundred rows): bf16 from
    # then on.
    # (measured, 17 000 queries x 70 000 keys: an ordinary bank passes 117 + 102 on its two int8 levels -- 54 + 41 on bf16 --, a
    # bank with a 3000-key cluster around the queries 665 -- 64 on bf16 --, nothing overflowing: tools/stats_probe.py)
    I8_MAX_CANDIDATES_BASE = 300.0
    I8_MAX_CANDIDATES_PER_KEY = 1.2e-3
    # A demotion (int8 -> bf16, filter -> fp32 kernels) is a verdict on the QUERIES seen so far as much as on the bank: after
    # this many more queries the bank is tried one level up again, on a call of at most REPROBE_MAX_BATCH queries (a probe that
    # overflows costs an exact scan per overflowed query); a probe that fails demotes again and quadruples the interval.
    REPROBE_QUERIES = 1 << 20
    REPROBE_MAX_BATCH = 4096
    # Speculative first bound (ops.set_filter_prior, csrc/topk_filter.hip): every filtered call reports the smallest and the
    # largest final k-th best score of its queries; once SPEC_WARM_CALLS calls over SPEC_WARM_QUERIES queries have, the next
    # calls of at least SPEC_MIN_BATCH queries start from prior = lowest seen - max(SPEC_MARGIN x (highest - lowest seen),
    # SPEC_MIN_MARGIN) instead of running a bound pass (a fifth to a quarter of a mid-sized call).  The call proves every
    # answer and scans exactly for the queries the prior was too high for: one such query costs more than the pass saves, so
    # a call that reports misses -- or candidates beyond SPEC_MAX_CANDIDATES x the bound pass's calls' -- withdraws the
    # prior until the re-probe interval has passed (a failed re-probe quadruples it).  Banks whose queries' k-th best
    # scores spread widely (a prior far below most of them: a flood of candidates) end there after one call.
    SPEC_MIN_BATCH = 17
    SPEC_WARM_CALLS = 2
    SPEC_WARM_QUERIES = 64
    SPEC_MARGIN = 0.5
    SPEC_MIN_MARGIN = 0.01
    SPEC_MAX_CANDIDATES = 1.5
    SPEC_HISTORY = 16
    # Tight bound (ops.set_filter_tight_prior, csrc/filter_schedule.h: filter_call_plan): a call of at least TIGHT_MIN_BATCH
    # queries that runs under the prior above ALSO starts every query from t = lowest k-th best of the history - TIGHT_MARGIN
    # and runs ONE level; a query whose k-th best found is below t is repaired on the device from max(prior, what it found),
    # up to 256 of them by a 256-query call of the direct kernel, more by one more level over the bank.  So a miss of t costs
    # about 0.1 ms (any number up to 256) where a miss of the prior costs a scan: t needs no margin of the spread.  The scores
    # of the bench's queries have sigma = 1 / 16 and their k-th best sits 4 sigma out, where 0.002 of score is 13 % more
    # candidates (measured at the bench shape: 0 soft misses in every polled step over its 8 distinct batches, 152 candidates
    # per query; t 0.004 higher: 10 soft misses, 0.2 ms less per call -- which the rule below TIGHT_MAX_SOFT now collects).  This
    # rule is where t STARTS and what calls without tail counts follow: a call that reports more than TIGHT_MAX_SOFT soft
    # misses doubles the margin (up to TIGHT_MARGIN_MAX), one
    # whose repair took the all-queries level withdraws t for the re-probe interval.  RAGRAPH_SPEC_TIGHT=0: the prior alone (A/B).
    # From TIGHT_MIN_BATCH queries: the verdict and the (empty) repair are eight more launches, ~13 us, and up to 4096 queries
    # the call under the prior already runs one level, so t only saves candidates there -- 1M x 256, ms per call without / with
    # t: 512 queries 0.154 / 0.167, 4096: 0.894 / 0.865, 100 000: 19.2 / 17.8 (profiles/tight_prior.txt).
    TIGHT_MIN_BATCH = 2048
    TIGHT_MARGIN = 0.002
    TIGHT_MARGIN_MAX = 0.064
    TIGHT_MAX_SOFT = 32
    # Placing t at a soft-miss COUNT.  The rule above knows the minimum of the k-th best scores only, so it keeps t below all of
    # them, and every query admits the keys between t and its own k-th best for nothing: at the bench shape t = 0.2455 passes
    # 129.6 candidates per query, t = 0.2494 (10 soft misses) 101.0 and saves 0.22 ms per call net of the 0.1 ms repair, which
    # costs the same for 1 or 256 rows (profiles/tight_prior.txt section 5).  A tight call reports five points of the low
    # tail's cumulative count -- the judged queries whose final k-th best is below t (SOFT_MISSES) and below t + m delta,
    # m = 1, 2, 4, 8, delta = (t - prior) / 16 (TAIL_DELTA, TAIL_BELOW; csrc/filter_verify_fixup.h) --, and a polled call that
    # does moves t to where their log-linear interpolation meets TIGHT_TARGET_SOFT (_aim_tight).  Conditions, none of them a
    # measurement: the target is at most TIGHT_TARGET_SOFT_MAX = 64, a quarter of the 256-row repair, so a call at four times
    # its expected count still takes the cheap repair and not one more level (+15 ms); t never moves above the highest reported
    # edge t + 8 delta, which is also the most it rises per polled call; it never goes to or below the prior, nor below the
    # rule above (lowest - margin: fewer misses than none buy nothing); a count within a factor of two of the target leaves t
    # where it is (a count of 32 scatters by +-6 between batches of one distribution: chasing that moves t every call);
    # a call beyond twice the target re-aims DOWN from its own counts, by the slope of its lowest rising segment.  The
    # all-queries repair withdraws t exactly as above and forgets the aimed t (the re-probe starts from the rule above); calls
    # whose words lack TAIL_DELTA follow the rule above unchanged.  RAGRAPH_TIGHT_TARGET_SOFT=n sets the target (clamped to 64);
    # 0 keeps the rule above (A/B).
    # Batch classes: the repair is one pass of the direct kernel over the bank, about 0.1 ms at 1M x 256 whatever its row count,
    # and what a higher t saves grows with the batch -- measured against the rule above (profiles/tight_quantile.txt): 100 000 x
    # 1M x 256 -0.3 ms per step and 20 000 x 500k x 128 1.22 -> 1.12 ms, but 4096 x 1M x 256 0.83 - 0.86 -> 0.89 - 0.91 ms and 4096
    # x 4M x 64 0.85 -> 0.92.  Saving and cost both grow with the bank, the cost also with the row width, so the break-even
    # batch is proportional to D (about 128 D from those four points): t is aimed for calls of at least
    # TIGHT_TARGET_QUERIES_PER_DIM x D queries -- twice the break-even -- and from such calls' counts only; smaller calls keep the
    # rule above.  A count is a count of ONE batch size: an aimed t serves calls of up to twice the queries of the call it was
    # aimed from (at most twice its soft misses), larger ones start from the rule above and aim for themselves.
    TIGHT_TARGET_SOFT = 32
    TIGHT_TARGET_SOFT_MAX = 64
    TIGHT_TARGET_QUERIES_PER_DIM = 256
    DEDUP_MIN_ROWS = 2048
    DEDUP_MAX_UNIQUE = 0.9
    DEDUP_MAX_GROUP = 64
    # The tail is folded in (seal) once it holds more than min(TAIL_MAX_ROWS, sealed_rows // TAIL_DIVISOR) rows, or when a call
    # asks for more keys than the sealed part has.  TAIL_DIVISOR is derived, not measured: a small bank then grows by at least
    # a ninth between two re-seals, so the rows re-converted over its life are a geometric sum -- at most nine times its final
    # size -- and a 40-row bank that receives 40 more re-seals at once.  TAIL_MAX_ROWS is measured: the largest swept tail
    # whose call takes at most 1.10 x the call without one at 4096 and at 100 000 queries against 1M x 256 keys
    # (profiles/bank_append.txt: 512 rows cost 5 %, 4096 rows 17 - 18 %; the tail defers a rebuild, it is not a second search
    # path).  RAGRAPH_BANK_TAIL=0: extend seals at once -- the bank of one version this class was before (A/B, escape hatch).
    TAIL_DIVISOR = 8
    TAIL_MAX_ROWS = 512
    # Mixed retrieval through the filter (topk_mix): a call whose unproven share exceeds this is answered all the same -- its
    # unproven rows by the exact call -- but later calls with its weights and k go straight to the exact call, until the rows
    # or the weights change.  The largest of 1/16, 1/8, 1/4, 1/2 at which the route still beat the exact call by more than the
    # spread at both 4096 and 100 000 queries x 1M x 256 (profiles/topk_mix_filtered.txt, forced shares; ms exact vs routed at
    # 1/16, 1/8, 1/4, 1/2: 18.0 vs 3.0, 4.2, 6.5, 10.9 and 393 vs 49.7, 76.6, 131, 226).
    MIX_FILTER_MAX_UNPROVEN = 1.0 / 2

    def __init__(self, keys_normalized: torch.Tensor, ops=None, dedup: bool = True):
        if ops is None:
            from . import kernels as ops  # the HIP library; raises loudly without a GPU
        self.ops = ops
        # Row widths the fused kernels are not written for (the reference takes any emb_size, SimilarityFunctions.py:6-16):
        # up to 256 the bank is zero-padded ONCE to the next fused width and every query per call -- zero columns change no
        # bit of a norm or a score (kernels.padded_dim) --; wider banks take the score-slab path of topk_cosine (any D).
        self.dim = int(keys_normalized.shape[1])
        pad = getattr(ops, "padded_dim", None)
        self._width = pad(self.dim) if pad is not None else self.dim   # None: no fused kernel for this width
        if self._width is not None and self._width != self.dim:
            keys_normalized = ops.pad_cols(keys_normalized, self._width)
        self.keys_normalized = keys_normalized      # all rows, sealed and tail
        self._store = keys_normalized               # padded widths: the growable padded matrix keys_normalized is a prefix of
        self._sealed_rows = int(keys_normalized.shape[0])
        self._tail_rows = 0
        self._dedup = dedup
        self.tail_enabled = os.environ.get("RAGRAPH_BANK_TAIL", "1") != "0"
        self._packed = None
        self._bf16 = None
        self._filter_off = False  # set when this bank defeats the filter (see _poll_overflow)
        self._i8_off = False      # set when this bank defeats the INT8 levels only (clustered keys: too many within the int8 bound)
        self.i8_classes = None    # the int8 copy's two classes of granules as read for _i8_ok (kernels.int8_copy_classes)
        self._pending = None      # (pinned word, event, batch, had int8 levels, k, tight bound) of the last filtered call's overflow count
        self._i8_ok = None        # the int8 copy's error row read (once, lazily): accurate enough for int8 levels?
        self._seen_i8, self._seen_bf16 = [0, 0], [0, 0]   # [queries, overflowed] of the polled calls with / without int8
        self._queries = 0                                  # queries answered so far (the clock of the re-probes)
        self._demoted = {"i8": None, "filter": None}       # query count at the demotion, or None
        self._reprobe_after = {"i8": self.REPROBE_QUERIES, "filter": self.REPROBE_QUERIES}
        self._probed_at = {"i8": None, "filter": None}     # query count at the last re-probe
        self._host_word = self._event = None
        self._overflowed = 0
        self.last_i8_candidates = None   # candidates per query over the int8 levels of the last polled call (sampled)
        # speculative first bound, per k: {"hist": [(lowest, highest k-th best of a polled call)], "queries": seen, "off_at":
        # query count at which it was withdrawn (None: in use), "after": re-probe interval, "cand": candidates per query of
        # the last polled call WITH a bound pass, "failed": misses so far}
        self._spec = {}
        self.spec_enabled = os.environ.get("RAGRAPH_SPEC", "1") != "0"   # (RAGRAPH_SPEC=0: every call with its bound pass -- A/B)
        self.tight_enabled = os.environ.get("RAGRAPH_SPEC_TIGHT", "1") != "0"
        self.tight_target = min(max(int(os.environ.get("RAGRAPH_TIGHT_TARGET_SOFT", self.TIGHT_TARGET_SOFT)), 0), self.TIGHT_TARGET_SOFT_MAX)
        self.last_tight = None           # the tight bound the last filtered call ran with (None: none)
        self._notes = 0                  # calls offered to _note_overflow (small calls report every fourth once settled)
        self.last_stats = None           # device view of the last filtered call's statistics words (this index, this stream)
        self.last_prior = None           # the speculative first bound the last filtered call ran with (None: a bound pass)
        self.last_over = None            # sharded calls: the last call's overflow count (device int; the owner of the bank reads it)
        # None: duplicates not looked at yet; False: looked at, searched as it is; else (KeyIndex over the unique rows,
        # group_ptr, members)
        self._collapsed = None if dedup else False
        self.duplicate_stats = None   # (rows, unique rows, largest group) once judged
        # retired rows (retire): the sorted host ids (int64 CPU tensor; the authority) and the device bitmap over the physical
        # rows (int32 words, bit r & 31 of word r >> 5); both None until a row is retired
        self._retired = self._bitmap = None
        # topk_mix: the (w_struct, w_sem, k) whose calls go straight to the exact call, the weights they were judged under, and
        # counters for the tests and the probe
        self._mix_demoted, self._mix_weights = set(), None
        self.mix_stats = {"filtered_calls": 0, "exact_calls": 0, "rows_unproven": 0, "demotions": 0}

    @property
    def sealed_rows(self) -> int:
        """Rows the copies, groups and verdicts of this index cover."""
        return self._sealed_rows

    @property
    def tail_rows(self) -> int:
        """Rows appended since (searched by the seeded tail pass)."""
        return self._tail_rows

    @property
    def retired_rows(self) -> int:
        """Physical rows taken out of the bank (retire) and still stored."""
        return 0 if self._retired is None else int(self._retired.numel())

    @property
    def live_rows(self) -> int:
        """sealed_rows + tail_rows - retired_rows: the rows topk answers over."""
        return self._sealed_rows + self._tail_rows - self.retired_rows

    @property
    def retired_ids(self) -> torch.Tensor:
        """The retired physical row ids, sorted (an int64 host tensor)."""
        return torch.empty(0, dtype=torch.int64) if self._retired is None else self._retired

    @property
    def retired_bitmap(self):
        """The device bitmap over the physical rows (None while nothing is retired): the one topk_drop_rows reads."""
        return self._bitmap

    def retire(self, rows) -> None:
        """Take the physical rows `rows` (a tensor, array or list of ids over sealed_rows + tail_rows: what topk returns minus
        idx_base) out of the answers.  Nothing stored is touched -- the copies' scales and error rows are functions of the whole
        bank (csrc/filter_common.h) and every bound is a proof over them --: the ids join one sorted host array (the authority
        for retired_rows) and have their bits set in a device bitmap, made on the first call.  Validated and de-duplicated on the
        host (not a hot path: one copy); an id out of range raises IndexError before anything changes; retiring a row twice is a
        no-op.  A learnt prior stays: the physical rows it was learnt over are unchanged, and the state is per k_in."""
        if getattr(self.ops, "topk_drop_rows", None) is None or getattr(self.ops, "retire_rows", None) is None:
            raise RagraphNativeError("KeyIndex.retire: the kernels (ops) have no topk_drop_rows / retire_rows entry")
        ids = torch.as_tensor(rows).detach().to("cpu", torch.int64).reshape(-1)
        n = self._sealed_rows + self._tail_rows
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n):
            raise IndexError(f"KeyIndex.retire: row ids outside [0, {n}) (lowest {int(ids.min())}, highest {int(ids.max())})")
        old = self._retired if self._retired is not None else ids.new_empty(0)
        merged = torch.unique(torch.cat([old, ids]))   # (sorted)
        if merged.numel() == old.numel():
            return
        new = merged[~torch.isin(merged, old)]
        self._grow_bitmap(n)
        self.ops.retire_rows(self._bitmap, new.to(self.keys_normalized.device), n)
        self._retired = merged
        self._mix_demoted.clear()   # (the live rows changed: topk_mix judges them again)

    def _grow_bitmap(self, n_rows: int) -> None:
        """The bitmap covers n_rows rows (new words zero: new rows are live); made here on first use."""
        words = max(-(-n_rows // 32), 1)
        if self._bitmap is None:
            self._bitmap = torch.zeros(words, dtype=torch.int32, device=self.keys_normalized.device)
        elif self._bitmap.numel() < words:
            grown = self._bitmap.new_zeros(max(words, 2 * self._bitmap.numel()))
            grown[:self._bitmap.numel()] = self._bitmap
            self._bitmap = grown

    def overfetch_keeps_class(self, k: int, ceilings=None) -> bool:
        """Does a list of k + retired_rows keys lie under the same ceiling as one of k keys, among 32, TOPK_MAX, TOPK_FILTER_MAX
        (the ceilings of FILTERED_BY_K; TOPK_MAX is also the seeded tail pass's) and TOPK_ORDERED_MAX?  The owner of the rows
        compacts when it does not (ToyGraphBase.topk): this index never does, it does not own the rows.  ceilings: those of
        another search over the same rows (ToyGraphBase's two-metric branch: its fused limit and TOPK_ORDERED_MAX)."""
        if ceilings is None:
            ceilings = tuple(c for c, _, _ in FILTERED_BY_K) + (TOPK_ORDERED_MAX,)
        under = lambda n: next((c for c in ceilings if n <= c), None)
        return under(k + self.retired_rows) is not None and under(k + self.retired_rows) == under(k)

    def rebase(self, keys_normalized: torch.Tensor) -> None:
        """The physical rows changed arbitrarily (the owner compacted them): `keys_normalized` is the bank's new normalised
        matrix, of the same width.  A new bank for everything derived from ROWS -- what seal drops, the tail count, the bitmap
        and the retired ids, the padded store, a statistics word still in flight -- and for _spec: a learnt prior is a lower bound
        of a k-th best score, which removing rows can only LOWER (seal's argument the other way round: there rows only arrive),
        so the priors are learnt again.  Kept: _i8_off / _filter_off, _demoted and the re-probe clocks, _queries, _overflowed --
        verdicts on the queries and on what kind of bank this is, which taking a few rows out does not change."""
        if keys_normalized.dim() != 2 or keys_normalized.shape[1] != self.dim:
            raise ValueError(f"KeyIndex.rebase: {tuple(keys_normalized.shape)} is not a bank of width {self.dim}")
        if self._width is not None and self._width != self.dim:
            keys_normalized = self.ops.pad_cols(keys_normalized, self._width)
        self.keys_normalized = self._store = keys_normalized
        self._sealed_rows, self._tail_rows = int(keys_normalized.shape[0]), 0
        self._bf16 = self._packed = None
        self._collapsed = None if self._dedup else False
        self._i8_ok = self.i8_classes = None
        self._retired = self._bitmap = None
        self._pending = None
        self._spec = {}
        self._mix_demoted.clear()

    @staticmethod
    def _capturing() -> bool:
        # (is_initialized, not is_available: nothing captures before the runtime is up, and is_available costs ~2 us of every call)
        return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()

    def _sealed_keys(self) -> torch.Tensor:
        return self.keys_normalized[:self._sealed_rows] if self._tail_rows else self.keys_normalized

    def extend(self, keys_normalized: torch.Tensor) -> None:
        """The bank grew: `keys_normalized` is its new, longer normalised matrix, whose first sealed_rows + tail_rows rows
        are bit-equal to what this index holds (the caller's contract; checked by shape only).  The new rows join the tail;
        nothing is rebuilt and no counter, history, demotion or pending statistics word is touched.  A padded width keeps its
        own growable padded matrix and pads the new rows only."""
        n_old, n_new = self._sealed_rows + self._tail_rows, int(keys_normalized.shape[0])
        if keys_normalized.dim() != 2 or keys_normalized.shape[1] != self.dim or n_new < n_old:
            raise ValueError(f"KeyIndex.extend: {tuple(keys_normalized.shape)} does not continue a bank of {n_old} x {self.dim}")
        if self._width is not None and self._width != self.dim:
            if self._store.shape[0] < n_new:
                grown = self._store.new_zeros((max(n_new, 2 * self._store.shape[0]), self._width))
                grown[:n_old] = self._store[:n_old]
                self._store = grown
            self._store[n_old:n_new, :self.dim] = keys_normalized[n_old:]
            self.keys_normalized = self._store[:n_new]
        else:
            self.keys_normalized = self._store = keys_normalized
        self._tail_rows = n_new - self._sealed_rows
        if n_new > n_old:
            self._mix_demoted.clear()   # (new rows: topk_mix judges the bank again)
        if self._bitmap is not None:
            self._grow_bitmap(n_new)   # (zero bits: the new rows are live)
        if not self.tail_enabled or getattr(self.ops, "topk_cosine_tail", None) is None:
            self.seal()
        else:
            self._maybe_seal()

    def _maybe_seal(self, k: int = 0) -> None:
        """The sealing rule (at extend and at the start of topk); never while a stream is being captured."""
        if self._tail_rows and not self._capturing() and (
                self._tail_rows > min(self.TAIL_MAX_ROWS, self._sealed_rows // self.TAIL_DIVISOR) or k > self._sealed_rows):
            self.seal()

    def seal(self) -> None:
        """Fold the tail into the sealed part.  Dropped: what was derived from the rows (the bf16 / int8 and packed copies, the
        duplicate groups, the int8 copy's verdict), rebuilt lazily as for a new bank.  Kept: what was learnt from the queries
        (_spec with its priors and tight-bound state, _i8_off / _filter_off, _demoted and the re-probe clocks, _queries,
        _overflowed) -- a learnt prior is a lower bound of a k-th best score, which more rows can only raise, and every
        answer is proven anyway."""
        if not self._tail_rows:
            return
        self._sealed_rows += self._tail_rows
        self._tail_rows = 0
        self._bf16 = self._packed = None
        self._collapsed = None if self._dedup else False
        self._i8_ok = self.i8_classes = None

    @property
    def overflowed_queries(self) -> int:
        """Queries of polled filtered calls that went to the exact scan (diagnostic)."""
        return self._overflowed + (self._collapsed[0].overflowed_queries if self._collapsed else 0)

    @property
    def search_index(self) -> "KeyIndex":
        """The index whose rows the kernels actually stream: the one over the unique rows when the bank was collapsed."""
        return self._collapsed[0] if self._collapsed else self

    def search_rows(self, min_unique: int = 0) -> int:
        """Rows the kernels search for this bank: judges its duplicates now (ShardedToyGraphBase calls this on every rank
        before the ranks agree on plan_n).  A collapsed bank of fewer than min_unique unique rows is searched as it is."""
        if self._collapsed is None:
            self._judge_duplicates()
        if self._collapsed and self._collapsed[0].keys_normalized.shape[0] < min_unique:
            self._collapsed = False
        return int(self.search_index._sealed_keys().shape[0])

    def _judge_duplicates(self):
        """Once per sealed part (never while a HIP graph is being captured: one read-back)."""
        kn = self._sealed_keys()
        dedup = getattr(self.ops, "dedup_rows", None)
        if dedup is None or kn.shape[0] < self.DEDUP_MIN_ROWS:
            self._collapsed = False
            return
        if kn.is_cuda and self._capturing():
            return   # (stays undecided: searched as it is for now)
        U, largest, uniq_row, group_ptr, members = dedup(kn)
        self.duplicate_stats = (kn.shape[0], U, largest)
        if U > self.DEDUP_MAX_UNIQUE * kn.shape[0] and largest <= self.DEDUP_MAX_GROUP:
            self._collapsed = False
            return
        unique = self.ops.gather_rows(kn, uniq_row)   # (normalised rows copied bit for bit: still normalised)
        self._collapsed = (KeyIndex(unique, self.ops, dedup=False), group_ptr, members)

    def _poll_overflow(self):
        """The filtered call repairs overflowed rows on the device and reads nothing back; its count arrives here after
        the fact (pinned host word + event, polled without waiting).  A bank of near-duplicates (thousands of keys within
        the bound of a query's k-th best) sends its queries to the exact fallback scan: still exact, but a scan reads the
        whole bank for ONE query (~0.2 ms of HBM time at 1M x 256 keys, 1.7 ms when it is the only one) where the fp32
        kernels spend ~3.5 us more per query than the filter: beyond OVERFLOW_FRACTION of a batch the levels first leave
        int8 (the bf16 bound is ~5x tighter), then the bank leaves the filter."""
        pend = self._pending
        if pend is None or self._capturing() or not pend[1].query():   # (an event query is not a capturable call)
            return
        self._pending = None
        (n_over, *words), B = pend[0].tolist(), pend[2]   # the pinned word: the count, then the call's statistics words (filter_stats)
        labelled = len(words) > FS.MAGIC and words[FS.MAGIC] == FS.MAGIC_VALUE
        if n_over < 0:                          # (the statistics words came in one copy: they hold the count themselves)
            n_over = words[FS.OVERFLOW] if labelled else 0   # (no kernel counts all-zero queries: answered without a scan)
        speculative = False
        if len(pend) > 4 and pend[4] and len(words) > FS.KTH_HI and labelled:
            speculative = bool(words[FS.SPECULATIVE])
            n_over = self._judge_prior(pend[4], B, words, n_over, pend[5] if len(pend) > 5 else None)   # (what is left is the lists' fault)
        self._overflowed += n_over
        i8_was_off = self._i8_off               # (the call ran under this setting: the overflow rule below judges IT)
        # the call's sampled candidate counts (int8 levels only are judged -- and only of a call with a bound pass: what a
        # prior far below the queries' k-th best lets through says nothing about the int8 copy, _judge_prior withdraws the prior)
        if pend[3] and len(words) >= FS.LEVEL_WORDS and not speculative:
            i8 = [(keys, c) for dt, keys, c in FS.levels(words) if dt == "int8" and c is not None]
            if i8:
                self.last_i8_candidates = sum(c for _, c in i8)
                if self.last_i8_candidates > self.I8_MAX_CANDIDATES_BASE + self.I8_MAX_CANDIDATES_PER_KEY * sum(kk for kk, _ in i8):
                    self._demote("i8")
        # judged over whole calls of >= 64 queries, or over the calls seen so far once they add up to 8 queries (graph
        # classification retrieves ONE query per forward: a bank that sends every such call to the exact scan must not stay)
        acc = self._seen_i8 if pend[3] else self._seen_bf16
        acc[0] += B
        acc[1] += n_over
        if (B >= 64 and n_over >= 2 and n_over > self.OVERFLOW_FRACTION * B) or (acc[0] >= 8 and 4 * acc[1] > acc[0]):
            if pend[3] and not i8_was_off:     # the call(s) had int8 levels: their wider bound is the first suspect
                self._demote("i8")
            else:
                self._demote("filter")
            acc[0] = acc[1] = 0
        elif acc[0] >= 4096:
            acc[0] = acc[1] = 0

    def _judge_prior(self, k: int, B: int, words, n_over: int, tight=None) -> int:
        """A polled call's statistics words (`tight`: the tight bound that call ran with, if known): feed the k-th-best history;
        judge a speculative call (misses, candidates, overflowed lists).  Returns the overflow count the LISTS are to be judged by: a speculative call's misses are not
        their fault, and neither are lists that overflowed under a prior (far below most queries' k-th best it floods them:
        the prior goes, the bank is judged by its calls with a bound pass)."""
        st = self._spec_state(k)
        spec, failed, lo, hi = words[FS.SPECULATIVE], words[FS.SPEC_FAILED], words[FS.KTH_LO], words[FS.KTH_HI]
        lists_over = max(n_over - failed, 0)
        cand = FS.candidates_per_query(words)
        if lists_over:
            st["hist"], st["queries"] = [], 0      # (a bank whose lists overflow is no ground for a prior)
        elif lo != 0x7FFFFFFF and hi != -0x80000000 and B - failed > 0:
            st["hist"].append((FS.ord2f(lo), FS.ord2f(hi)))
            del st["hist"][:-self.SPEC_HISTORY]
            st["queries"] += B
        if not spec:
            if cand is not None and not lists_over:
                st["cand"] = cand
            return lists_over
        st["used"] += 1
        st["failed"] += failed
        self._judge_tight(st, words, tight)
        loose = cand is not None and st["cand"] is not None and cand > self.SPEC_MAX_CANDIDATES * max(st["cand"], 32.0)
        if failed or loose or lists_over:
            probed_at = st.get("probed_at")
            if probed_at is not None and self._queries - probed_at < st["after"]:
                st["after"] = min(st["after"] * 4, 1 << 40)   # the re-probe failed
            st["off_at"] = self._queries
            if failed:   # the history missed these queries' scores: start it over (their k-th best arrives with the next calls)
                st["hist"] = []
                st["queries"] = 0
        return 0   # (a speculative call says nothing about the lists)

    def _judge_tight(self, st: dict, words, tight=None):
        """A polled speculative call's words TIGHT (a tight bound was in force), SOFT_MISSES and REPAIR (1: the 256-query
        repair ran, 2: the all-queries level): withdraw t after the level; a call that reports its tail counts (TAIL_DELTA; `tight`
        is the t it ran with) aims the next t at the target count, any other widens the margin after a flood of soft misses."""
        if len(words) <= FS.REPAIR or not words[FS.TIGHT]:
            return
        st["soft"] = st.get("soft", 0) + words[FS.SOFT_MISSES]
        st["tight_used"] = st.get("tight_used", 0) + 1
        points = FS.tail_points(words, tight) if self.tight_target and tight is not None else None
        if words[FS.REPAIR] == 2:
            st["tight_off_at"] = self._queries
            st.pop("tight_aimed", None)
        elif points is not None and self._aims_tight(words[FS.QUERIES]):
            st["tight_aimed"] = (self._aim_tight(points, self.tight_target), words[FS.QUERIES])
        else:
            points = None   # (a batch class that keeps the rule of the margin)
        if words[FS.REPAIR] == 2 or (points is None and words[FS.SOFT_MISSES] > self.TIGHT_MAX_SOFT):
            st["tight_margin"] = min(2.0 * st.get("tight_margin", self.TIGHT_MARGIN), self.TIGHT_MARGIN_MAX)

    def _aims_tight(self, B: int) -> bool:
        """Is t placed at a soft-miss count for calls of B queries against this bank (TIGHT_TARGET_QUERIES_PER_DIM)?"""
        return bool(self.tight_target) and B >= self.TIGHT_TARGET_QUERIES_PER_DIM * (self._width or self.dim)

    @staticmethod
    def _aim_tight(points, target: int) -> float:
        """The t at which the cumulative count [(score, queries below it)] of a tight call -- its own t first -- meets `target`,
        log-linear between the points (a count of 0 stands for half a query); at most the highest point; below the first point
        by the slope of the lowest rising segment; the first point itself within a factor of two of the target."""
        (t, c0), top = points[0], points[-1][0]
        if target <= 2 * c0 <= 4 * target:
            return t
        lg = lambda c: math.log(max(float(c), 0.5))
        if c0 < target:
            for (x0, n0), (x1, n1) in zip(points, points[1:]):
                if n1 >= target:   # (n0 < target <= n1: the segment rises)
                    return min(x0 + (x1 - x0) * (lg(target) - lg(n0)) / (lg(n1) - lg(n0)), top)
            return top
        for x1, n1 in points[1:]:
            if n1 > c0:
                return t - (lg(c0) - lg(target)) * (x1 - t) / (lg(n1) - lg(c0))
        return t - (top - t)   # (every judged query below t: one span down)

    def _tight_for(self, B: int, k: int, prior):
        """The tight bound for a call of B queries that runs under `prior`, or None (no prior -- which covers captures and
        RAGRAPH_SPEC=0 --, switched off, withdrawn, a batch the direct or single-launch kernels take, nothing above the prior)."""
        if prior is None or not self.tight_enabled or B < self.TIGHT_MIN_BATCH or \
                getattr(self.ops, "set_filter_tight_prior", None) is None:
            return None
        st = self._spec_state(k)
        off_at = st.get("tight_off_at")
        if off_at is not None:
            if self._queries - off_at < self.REPROBE_QUERIES:
                return None
            st["tight_off_at"] = None
        if not st["hist"]:
            return None
        t = min(h[0] for h in st["hist"]) - st.get("tight_margin", self.TIGHT_MARGIN)
        aimed = st.get("tight_aimed")
        if aimed is not None and self._aims_tight(B) and B <= 2 * aimed[1]:
            t = max(t, aimed[0])   # (aimed at a soft-miss count by the tail counts of a polled call of aimed[1] queries: _judge_tight)
        return t if t > prior else None

    def _demote(self, what: str):
        """int8 -> bf16 levels ("i8") or filter -> fp32 kernels ("filter"), until the re-probe.  A demotion within one interval
        of the previous re-probe of the same kind is a failed probe: the next one waits four times as long."""
        if what == "i8":
            self._i8_off = True
        else:
            self._filter_off = True
        if self._demoted[what] is None:
            probed_at = self._probed_at[what]
            if probed_at is not None and self._queries - probed_at < self._reprobe_after[what]:
                self._reprobe_after[what] = min(self._reprobe_after[what] * 4, 1 << 40)   # the probe failed
            else:
                self._reprobe_after[what] = self.REPROBE_QUERIES
            self._demoted[what] = self._queries

    def _maybe_reprobe(self, B: int):
        """Before a dispatch: lift a demotion whose interval has passed (filter first: it is the larger loss), on a call small
        enough that a failed probe is cheap."""
        if B > self.REPROBE_MAX_BATCH:
            return
        for what in ("filter", "i8"):
            at = self._demoted[what]
            if at is not None and self._queries - at >= self._reprobe_after[what]:
                if what == "i8":
                    self._i8_off = False
                    self._seen_i8 = [0, 0]
                else:
                    self._filter_off = False
                    self._seen_bf16 = [0, 0]
                self._demoted[what] = None
                self._probed_at[what] = self._queries
                return

    def _spec_state(self, k: int) -> dict:
        st = self._spec.get(k)
        if st is None:
            st = self._spec[k] = {"hist": [], "queries": 0, "off_at": None, "after": self.REPROBE_QUERIES, "cand": None,
                                  "failed": 0, "used": 0}
        return st

    def _prior_for(self, B: int, k: int, small: bool = False):
        """The speculative first bound for a call of B queries, or None (not warm yet, withdrawn, switched off, capturing).
        small: the single-launch kernel's call (any batch size it takes)."""
        if not self.spec_enabled or (B < self.SPEC_MIN_BATCH and not small) or getattr(self.ops, "set_filter_prior", None) is None:
            return None
        if self._capturing():
            # a captured launch would carry TODAY's prior by value into every replay, and the statistics that could withdraw it
            # are not read under capture: captured calls keep their bound pass (a proof, whatever queries the replays bring)
            return None
        st = self._spec_state(k)
        if st["off_at"] is not None:
            if self._queries - st["off_at"] < st["after"] or B > self.REPROBE_MAX_BATCH:
                return None
            st["off_at"] = None          # re-probe: a miss now quadruples the interval (see _poll_overflow)
            st["probed_at"] = self._queries
        if len(st["hist"]) < self.SPEC_WARM_CALLS or st["queries"] < self.SPEC_WARM_QUERIES:
            return None
        lo = min(h[0] for h in st["hist"])
        hi = max(h[1] for h in st["hist"])
        return lo - max(self.SPEC_MARGIN * (hi - lo), self.SPEC_MIN_MARGIN)

    def _note_overflow(self, over, B: int, had_i8: bool, stats=None, k: int = 0):
        """After a filtered call: its overflow count travels to a pinned host word behind an event (no wait) and is
        judged by _poll_overflow at a later call."""
        if not over.is_cuda:  # (the CPU tests' oracle shim)
            self._overflowed += int(over)
        elif self._pending is None and not self._capturing():
            # a call of a few queries takes ~60 us and the copy + event below ~2 us of its stream: once the bank's dispatch
            # has settled (a prior in use, nothing withdrawn or demoted) such calls report every fourth time only
            self._notes += 1
            if B <= 64 and (self._notes & 3) and self.last_prior is not None:
                return
            if self._host_word is None:
                self._host_word = torch.zeros(1 + FS.N_WORDS, dtype=torch.int32).pin_memory()   # [0] overflow, [1:] the call's statistics
                self._event = torch.cuda.Event()
            if stats is not None and stats.numel() >= FS.N_WORDS:
                # ONE copy: the statistics words carry the call's final overflow count themselves (FS.OVERFLOW)
                self._host_word[1:].copy_(stats[:FS.N_WORDS], non_blocking=True)
                self._host_word[0] = -1            # (host store: "read it from the words")
            else:
                self._host_word[:1].copy_(over, non_blocking=True)
                self._host_word[1:].zero_()
                if stats is not None:
                    self._host_word[1:1 + stats.numel()].copy_(stats, non_blocking=True)
            self._event.record()
            self._pending = (self._host_word, self._event, B, had_i8, k, self.last_tight if stats is not None else None)

    def _cap_i8(self):
        """Before a filtered call: cap this thread's int8 levels for THIS bank (ops.set_max_i8_levels; the caller resets it
        to -1 afterwards).  The bank's int8 error row is read once per bank version (one synchronisation; never while a
        HIP graph is being captured -- an unjudged bank then stays on bf16).  Returns (the setter or None, int8 allowed)."""
        cap = getattr(self.ops, "set_max_i8_levels", None)
        if cap is None:
            return None, False
        if self._i8_ok is None and not self._capturing():
            # (the copy has two scales, csrc/filter_common.h: the NORMAL granules' error decides, unless more than a quarter
            # of the granules are HEAVY ones with a useless bound -- a bank of heavy-tailed rows throughout)
            c = self.ops.int8_copy_classes(self._bf16, self._sealed_rows)
            many_heavy = 4 * c["heavy_granules"] > c["granules"] and c["err_heavy"] > self.I8_MAX_ERR
            self._i8_ok = c["err"] <= self.I8_MAX_ERR and not many_heavy
            self.i8_classes = c
        allowed = bool(self._i8_ok) and not self._i8_off
        cap(-1 if allowed else 0)
        return cap, allowed

    def sharded_speculates(self, B: int, k: int, plan_n: int, n_shards: int) -> bool:
        """Would topk(..., exchange, plan_n, prior) of B queries skip its bound pass and exchange 0?  Taken from what every
        rank shares (B, k, the padded width, plan_n, the shard count): the same answer on every rank."""
        ops = self.ops
        if self._width is None or getattr(ops, "set_filter_prior", None) is None or getattr(ops, "sharded_speculates", None) is None:
            return False
        fhelps = getattr(ops, "filter_helps", None)
        if fhelps is None or B > self.MAX_FILTERED_BATCH or not fhelps(B, plan_n, self._width, k):
            return False
        return bool(ops.sharded_speculates(B, plan_n, self._width, k, n_shards))

    def topk(self, q: torch.Tensor, k: int, idx_base: int = 0, exchange=None, plan_n: int = 0, prior=None):
        """The canonical top-k of the bank's LIVE rows, indices over the physical rows (+ idx_base).  With nothing retired this is
        _topk_rows and nothing else: no bitmap, no extra launch.  With r retired rows the whole of _topk_rows -- sealing rule,
        route, tail pass, collapsed expansion, padding -- runs for k_in = min(k + r, physical rows) keys and ONE
        ops.topk_drop_rows brings the lists back to k: the same bits as a fresh index over the live rows, mapped through the
        increasing map from live to physical rows.  The other arguments: _topk_rows."""
        if self._retired is None:
            return self._topk_rows(q, k, idx_base, exchange, plan_n, prior)
        if exchange is not None:
            raise RagraphNativeError("KeyIndex.topk: a shard of a sharded bank (exchange) with retired rows: removal from a "
                                     "key-sharded bank is not supported")
        n, r = self._sealed_rows + self._tail_rows, self.retired_rows
        if k > n - r:
            raise RagraphNativeError(f"KeyIndex.topk: k={k} exceeds the {n - r} live rows of the bank ({r} of {n} retired)")
        k_in = min(k + r, n)
        if k_in > TOPK_ORDERED_MAX:
            raise RagraphNativeError(f"KeyIndex.topk: k={k} with {r} retired rows needs lists of {k_in} > {TOPK_ORDERED_MAX} "
                                     "(TOPK_ORDERED_MAX) keys: compact the bank (the owner of the rows: ToyGraphBase.compact, "
                                     "then KeyIndex.rebase)")
        s, i = self._topk_rows(q, k_in, idx_base)
        s, i, _ = self.ops.topk_drop_rows(s, i, self._bitmap, n, k, idx_base=idx_base)   # (never short: k <= live rows)
        return s, i

    def _mix_filter_open(self, B: int, k: int, k_list: int, w_struct: float, w_sem: float) -> bool:
        """Does topk_mix take the filtered route for this call as the index stands?  No side effect."""
        ops = self.ops
        if not (0.0 < w_sem < math.inf) or not math.isfinite(w_struct) or self._capturing():
            return False
        if any(getattr(ops, name, None) is None for name in ("topk_mix_rerank", "mask_positions", "gather_rows", "scatter_topk_rows_")):
            return False
        n, D = self._sealed_rows + self._tail_rows, self._width or self.dim
        if k_list > n - self.retired_rows or not self._says("mix_filter_helps", B, n, D, k):
            return False
        k_in = min(k_list + self.retired_rows, n)   # (topk's over-fetch)
        if k_in > TOPK_FILTER_MAX:
            return False
        route = self._route(B, self._sealed_rows, D, k_in)
        if route == COLLAPSED:   # the unique rows' own index answers: its route counts
            inner = self._collapsed[0]
            route = inner._route(B, inner._sealed_rows, D, min(k_in, inner._sealed_rows))
        return route in (FILTERED, WIDE, WIDE128) and (float(w_struct), float(w_sem), k) not in self._mix_demoted

    def topk_mix(self, q: torch.Tensor, pos_q: torch.Tensor, pos_normalized: torch.Tensor, w_struct: float, w_sem: float, k: int,
                 exact):
        """The canonical top-k of  w_struct * cos(position codes) + w_sem * cos(embeddings)  over the bank's live rows: the bits
        of `exact(q, pos_q, k)`, the owner's exact mixed call (ops.topk_cosine_mix over its rows, with its own over-fetch for
        retired rows), reached through the filter where that pays:
        1. topk(q, k'), k' = ops.mix_filter_list(k) > k -- the canonical semantic candidates, by whatever route, tail, retired
           rows, collapsed duplicates and priors as ever;
        2. ops.topk_mix_rerank: the exact mixed scores of those k' keys, their canonical top-k, and per row the proof that no
           key outside the list can enter or tie (k-th best mixed score > fl(fl(s_last * w_sem) + slack));
        3. ONE 4-byte read-back of the unproven count -- the price of this route: a synchronisation, so never under a capture;
        4. unproven rows (ops.mask_positions of the flags: one more read-back, only then) are gathered, answered by `exact`
           and written back (ops.scatter_topk_rows_).  Nothing approximate is ever returned.
        The route is taken when w_sem > 0, the stream is not being captured, ops.mix_filter_helps says so, _route sends a list
        of k' keys to one of the filtered entries and (w_struct, w_sem, k) is not demoted; otherwise the call IS exact(q, pos_q,
        k).  A call whose unproven share exceeds MIX_FILTER_MAX_UNPROVEN demotes its (w_struct, w_sem, k) until the rows (extend,
        retire, rebase) or the weights change: a demotion never changes a bit, only the cost.  mix_stats counts the calls of
        either kind, the unproven rows and the demotions."""
        ops, st, B = self.ops, self.mix_stats, int(q.shape[0])
        weights = (float(w_struct), float(w_sem))
        if weights != self._mix_weights:
            self._mix_weights = weights
            self._mix_demoted.clear()
        k_list = getattr(ops, "mix_filter_list", lambda kk: min(128, max(32, 2 * kk)))(k)
        if B == 0 or not self._mix_filter_open(B, k, k_list, w_struct, w_sem):
            st["exact_calls"] += 1
            return exact(q, pos_q, k)
        s_sem, i_sem = self.topk(q, k_list)
        s, i, flags, count = ops.topk_mix_rerank(s_sem, i_sem, pos_q, pos_normalized, w_struct, w_sem, k)
        unproven = int(count.item())   # the read-back
        st["filtered_calls"] += 1
        st["rows_unproven"] += unproven
        if unproven == B:
            s, i = exact(q, pos_q, k)
        elif unproven:
            rows = ops.mask_positions(flags.ne(0))
            rs, ri = exact(ops.gather_rows(q, rows), ops.gather_rows(pos_q, rows), k)
            ops.scatter_topk_rows_(s, i, rows, rs, ri)
        if unproven > self.MIX_FILTER_MAX_UNPROVEN * B:
            self._mix_demoted.add((*weights, k))
            st["demotions"] += 1
        return s, i

    def _topk_rows(self, q: torch.Tensor, k: int, idx_base: int = 0, exchange=None, plan_n: int = 0, prior=None):
        """The canonical top-k of the PHYSICAL rows.  exchange / plan_n: this index holds one shard of a row-sharded bank (ShardedToyGraphBase): the filtered path
        sharpens its per-query bounds across the shards through `exchange` (kernels.topk_cosine_filtered), and every
        decision that changes which collectives run is taken from plan_n -- the largest shard's size -- so that all
        ranks take it alike.  prior (with exchange only): the speculative first bound the owner of the sharded bank chose for
        THIS call on every rank alike (it removes the bound pass and exchange 0; the owner proves the merged rows).
        With a tail: the sealed rows are searched as a bank of their own (every rule of _route unchanged), then one
        ops.topk_cosine_tail call continues the lists over the tail; idx_base applies to both parts.  Calls without a seeded
        pass -- k > TOPK_MAX, banks wider than every fused kernel -- run over all rows as ever; a shard of a sharded bank
        (exchange) seals first."""
        ops = self.ops
        if q.shape[1] != self.dim:
            raise ValueError(f"KeyIndex.topk: queries of {q.shape[1]} columns against a bank of {self.dim}")
        if self._width is not None and self._width != self.dim:
            q = ops.pad_cols(q, self._width)   # (the only place: _search and the tail pass take q at the bank's width)
        if self._tail_rows and exchange is not None:
            self.seal()
        else:
            self._maybe_seal(k)   # (nothing without a tail)
        if not self._tail_rows or k > TOPK_MAX or self._width is None:
            return self._search(self.keys_normalized, q, k, idx_base, exchange, plan_n, prior)
        if k > self._sealed_rows:   # (only while capturing: the rule above seals otherwise) exact over all rows, no seed
            return ops.topk_cosine(q, self.keys_normalized, k, idx_base=idx_base)
        s, i = self._search(self._sealed_keys(), q, k, idx_base)
        step = getattr(ops, "TOPK_TAIL_MAX", 65536)   # (a longer tail only exists under capture: one call per TOPK_TAIL_MAX rows)
        for t0 in range(self._sealed_rows, self._sealed_rows + self._tail_rows, step):
            t1 = min(t0 + step, self._sealed_rows + self._tail_rows)
            s, i = ops.topk_cosine_tail(q, self.keys_normalized[t0:t1], s, i, idx_base + t0)
        return s, i

    def _says(self, rule: str, *shape) -> bool:
        """The ops' own rule for a shape; an ops object without the rule never takes that route."""
        rule = getattr(self.ops, rule, None)
        return rule is not None and bool(rule(*shape))

    def _wide128_open(self, k: int) -> bool:
        """May lists of 65 .. 128 keys ask the wide128 rule?  (The bf16 / int8 copy covers the sealed rows only.)"""
        return k <= TOPK_FILTER_MAX and self._width is not None and not self._filter_off and not self._tail_rows and \
            hasattr(self.ops, "filter_wide128_helps")

    def _route(self, B: int, n_rows: int, D: int, k: int, exchange=None, plan_n: int = 0, tick: bool = False) -> str:
        """The kernel path (one of ROUTES) a call of B queries of width D against n_rows sealed rows takes as the index stands, and
        the only place that orders the paths.  Without tick no side effect: it reads _filter_off, _collapsed (undecided: searched
        as it is), _tail_rows and _width and asks each of the ops' rules at most once.  tick: _search's call (its docstring)."""
        shape = (B, n_rows, D, k)
        if self._width is None:   # wider than every fused kernel: exact score slabs, this shard's own top-k (no exchange needed)
            return SLAB
        if k > TOPK_MAX and exchange is None:
            # ordered large k over the full bank (duplicate rows score alike and the lower row wins: no collapse needed) unless the
            # wide128 entry pays -- never through unique rows: topk_expand_groups stops at 64
            if self._collapsed or not (self._wide128_open(k) and self._says("filter_wide128_helps", *shape)):
                return SLAB
        elif self._collapsed:
            return COLLAPSED
        elif exchange is not None and self._says("filter_helps", B, max(plan_n, n_rows), D, k) and B <= self.MAX_FILTERED_BATCH:
            return SHARDED   # (the rule is asked about the largest shard: every rank takes the same collectives)
        if tick:   # the bank's clock: judge the last polled call, lift a demotion that is due, count the queries
            self._poll_overflow()
            self._maybe_reprobe(B)
            self._queries += B
        if not self._filter_off:
            if self._says("fused_helps", *shape):   # small bank: every phase in one launch
                return FUSED
            ready = getattr(self.ops, "small_state_ready", None)   # a handful of queries against a large bank: ONE launch
            if self._says("small_helps", *shape) and (ready is None or ready(self.keys_normalized.device)):
                return SMALL
            for longest, route, rule in FILTERED_BY_K if exchange is None else ():   # (a shard the sharded rule refused: fp32)
                if k <= longest:   # (no rule: it was asked above, once per call)
                    if rule is None or self._says(rule, *shape):
                        return route if B <= self.MAX_FILTERED_BATCH else SLABS_OF_FILTERED
                    break
        return PACKED if self._says("packed_keys_help", B, D, k) else SLAB

    def _bf16_copy(self, kn: torch.Tensor) -> torch.Tensor:
        if self._bf16 is None:
            self._bf16 = self.ops.keys_to_bf16(kn)
        return self._bf16

    def _guarded(self, entry, q, kn, k: int, prior, tight, **kwargs):
        """ONE call entry(q, kn, bf16 copy, k, **kwargs) under the library's thread-local knobs -- this bank's int8 cap, the prior,
        the tight bound --, each knob it set reset whatever the call does; a call that returns leaves its prior in last_prior.
        Returns (scores, idx, over, the call's statistics words or None from an ops object without FILTER_STATS, int8 allowed)."""
        kb = self._bf16_copy(kn)
        knobs = [(getattr(self.ops, name), v) for name, v in (("set_filter_prior", prior), ("set_filter_tight_prior", tight)) if v is not None]
        cap, had_i8 = self._cap_i8()
        for knob, v in knobs:
            knob(v)
        with_stats = getattr(self.ops, "FILTER_STATS", False)   # this call's own statistics words, handed on explicitly
        try:
            out = entry(q, kn, kb, k, **(dict(kwargs, return_stats=True) if with_stats else kwargs))
        finally:
            if cap is not None:
                cap(-1)
            for knob, _ in knobs:
                knob(None)
        self.last_prior = prior
        s, i, over, stats = out if with_stats else (*out, None)
        return s, i, over, stats, had_i8

    def _search(self, kn: torch.Tensor, q: torch.Tensor, k: int, idx_base: int = 0, exchange=None, plan_n: int = 0, prior=None):
        """topk over the rows kn (the sealed part, or all rows of a bank without a tail), q at the bank's width: prepare, route,
        dispatch.  The order is behaviour:
        * duplicates are judged first (a large k: only where the wide128 rule could be asked);
        * a large k that stays on the slabs, a collapsed bank (the inner index counts, not this one) and a sharded filtered call are
          settled on _filter_off AS IT STANDS: no poll, no re-probe, _queries and _pending as they are, never a _note_overflow;
        * every other call: _poll_overflow(), _maybe_reprobe(B), _queries += B, and only then is _filter_off read for the fused,
          small and filtered routes (so a demotion that is due is lifted by the call that then takes the filter)."""
        ops = self.ops
        (B, D), n_rows = q.shape, kn.shape[0]
        if self._collapsed is None and self._width is not None and (k <= TOPK_MAX or exchange is not None or self._wide128_open(k)):
            self._judge_duplicates()
        route = self._route(B, n_rows, D, k, exchange, plan_n, tick=True)
        if route == SLAB:
            return ops.topk_cosine(q, kn, k, idx_base=idx_base)
        if route == PACKED:
            if self._packed is None:
                self._packed = ops.pack_keys(kn)
            return ops.topk_cosine(q, kn, k, idx_base=idx_base, keys_packed=self._packed)
        if route == FUSED:
            return ops.topk_cosine_fused(q, kn, self._bf16_copy(kn), k, idx_base=idx_base)
        if route == COLLAPSED:
            # (a shard: its unique rows take part in the exchanges, plan_n being the largest search_rows() of the ranks)
            inner, group_ptr, members = self._collapsed
            U = inner.keys_normalized.shape[0]
            if exchange is not None and U < k:
                raise RuntimeError("KeyIndex: a collapsed shard of fewer unique rows than k cannot take part in the exchanges; "
                                   "ShardedToyGraphBase keeps such a shard uncollapsed (search_rows(min_unique=k))")
            su, iu = inner.topk(q, min(k, U)) if exchange is None else inner.topk(q, k, 0, exchange, plan_n, prior)
            return ops.topk_expand_groups(su, iu, group_ptr, members, k, idx_base=idx_base)
        if route == SLABS_OF_FILTERED:
            # the candidate lists take 8 KiB per query: slabs of 256 k queries keep the workspace at 2 GiB (the edge flavour
            # asks for all 4 M nodes at once) at the throughput of one big call
            self._bf16_copy(kn)
            outs = [self._search(kn, q[b0:b0 + self.MAX_FILTERED_BATCH], k, idx_base) for b0 in range(0, B, self.MAX_FILTERED_BATCH)]
            return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
        if route == SHARDED:   # the caller's prior, no tight bound; the owner of the sharded bank reads last_over: no _note_overflow
            s, i, self.last_over, stats, _ = self._guarded(ops.topk_cosine_filtered, q, kn, k, prior, None,
                                                           idx_base=idx_base, exchange=exchange, plan_n=plan_n)
            if stats is not None:   # (only an ops object with FILTER_STATS has any)
                self.last_stats = stats
        elif route == SMALL:   # records the prior only: last_stats and last_tight stay those of the last filtered call
            s, i, over, stats, had_i8 = self._guarded(ops.topk_cosine_small, q, kn, k, self._prior_for(B, k, small=True), None,
                                                      idx_base=idx_base)
            self._note_overflow(over, B, had_i8 and D in (128, 256), stats, k)
        else:                  # FILTERED, WIDE, WIDE128: one entry (the packed fp32 copy is passed on, never made here)
            prior = self._prior_for(B, k)
            tight = self._tight_for(B, k, prior)
            s, i, over, stats, had_i8 = self._guarded(ops.topk_cosine_filtered, q, kn, k, prior, tight, idx_base=idx_base, keys_packed=self._packed)
            # (did THIS call have int8 levels?  The plan is asked for k <= 32, under the open cap the call ran with; a call of more
            # keys under an open cap is taken to have had them: an overflowing bank then leaves int8 first and the filter at the
            # next verdict.  The plan answers for every k now, but asking it there would change when a bank is demoted: kept.)
            had_i8 = had_i8 and (k > 32 or ops.filtered_i8_levels(B, n_rows, D, k) > 0)
            self.last_tight = tight
            self._note_overflow(over, B, had_i8, stats, k)
            self.last_stats = stats   # (diagnostic: bench.py / tools read the levels' candidate counts of the last call)
        return s, i

