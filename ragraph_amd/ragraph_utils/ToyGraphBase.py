"""Mirror of RAGraph_node/ragraph_utils/ToyGraphBase.py (and the graph flavour): the toy-graph vector library.

Bank layout in HBM: keys [N,D] fp32 (unit rows, as stored by the reference, ToyGraphBase.py:109), values [N,D],
labels [N,C] one-hot fp32, plus `keys_normalized` -- F.normalize(keys) computed ONCE per row; the reference
recomputes it on every retrieve (SimilarityFunctions.py:11; 2 GB of traffic per call at 1M x 256).
Storage grows geometrically (the reference re-allocates with torch.cat per resource graph, ToyGraphBase.py:116-119), and so
do the normalised caches once they exist: an append normalises the NEW rows into them and hands the longer matrix to the
bank's K.KeyIndex (KeyIndex.extend: the new rows are its tail), instead of dropping caches and index.
Rows leave the same way (remove_resources): they are retired behind the live index -- stored still, marked in a bitmap,
dropped from every answer -- until compact() gathers the live rows of every store.
"""
from __future__ import annotations

import torch
from torch import Tensor

from .. import kernels as K
from .Propagation import Propagation


class _Bank:
    """Append-only row store with amortised growth."""

    def __init__(self, width: int, device):
        self.buf = torch.empty((0, width), dtype=torch.float32, device=device)
        self.n = 0

    def append(self, rows: Tensor):
        rows = rows.to(self.buf.device, torch.float32)
        need = self.n + rows.shape[0]
        if need > self.buf.shape[0]:
            new = torch.empty((max(need, 2 * self.buf.shape[0], 1024), self.buf.shape[1]), dtype=torch.float32,
                              device=self.buf.device)
            new[:self.n] = self.buf[:self.n]
            self.buf = new
        self.buf[self.n:need] = rows
        self.n = need

    def reserve(self, m: int) -> Tensor:
        """Room for m more rows (old rows carried over bit for bit when the store reallocates): the view to fill them in."""
        need = self.n + m
        if need > self.buf.shape[0]:
            new = torch.empty((max(need, 2 * self.buf.shape[0], 1024), self.buf.shape[1]), dtype=torch.float32,
                              device=self.buf.device)
            new[:self.n] = self.buf[:self.n]
            self.buf = new
        out = self.buf[self.n:need]
        self.n = need
        return out

    def view(self) -> Tensor:
        if _Bank.reads is not None:   # (a training step being prepared for capture: ragraph_amd.capture)
            _Bank.reads[id(self)] = self
        return self.buf[:self.n]

    reads = None   # dict id -> _Bank while ragraph_amd.capture.CapturedTrainStep records which banks a step reads


class ToyGraphBase:
    noise_rng = K.NoiseRng()   # "host" (the default) | "device".
                           # "host": the reference's draws (torch.randint / torch.normal on the CPU generator, then a copy to the
                           # device) -- the same noise as the reference for the same seed, at the cost of host work on every
                           # noisy step, which a stream capture cannot record; "device": one seed per noisy call, drawn on the
                           # device generator and kept in `last_noise_seed` (a device tensor, never read back), and noise that is
                           # a hash of (seed, query row, draw) made inside the kernels (K.noise_rows, K.gather_reduce_noisy,
                           # K.add_normal_noise: another stream of random numbers, same law) -- no host work, capturable,
                           # reproduced by torch.manual_seed
    last_noise_seed = None
    build_rng = K.BuildRng()   # "host" (the default) | "device": where bank construction (ragraph_amd.bank_build) makes its draws.
                           # "host": torch's generators through torch chains, every bit as before; "device": one int64
                           # [1 + num_augment_scale, K.BUILD_SEED_COLUMNS] seed tensor per batch of resource graphs, drawn on the
                           # device generator and kept in `last_build_seed` (never read back), and every draw a hash of (seed,
                           # node or graph, draw) made inside the kernels of csrc/bank.hip -- another stream of the same laws,
                           # reproduced by torch.manual_seed, with nothing sized by the node pairs of a graph
    last_build_seed = None

    def _draw_noise_seed(self) -> Tensor:
        """The seed of this noisy call ("device" mode)."""
        self.last_noise_seed = K.draw_noise_seed(self.device)
        return self.last_noise_seed

    def __init__(self, pretrain_model, num_class, emb_size, query_graph_hop, device="cuda", flavour="node") -> None:
        self.flavour = flavour
        if flavour == "node":   # RAGraph_node/ragraph_utils/ToyGraphBase.py:18-29
            self.num_inverse_sample = 10
            self.num_augment_scale = 3
            self.retrieve_num = num_class + 1
        else:                   # RAGraph_graph/ragraph_utils/ToyGraphBase.py:21-27 (graph_fewshot: the same constants)
            self.num_inverse_sample = 0
            self.num_augment_scale = 0
            self.retrieve_num = min(3, num_class + 1)
        self.noise_retrieve_num = 1
        self.noise_std = 0.01
        self.toy_graph_hop = query_graph_hop - 1
        self.pretrain_model = pretrain_model
        self.device = torch.device(device)
        self._keys = _Bank(emb_size, self.device)
        self._values = _Bank(emb_size, self.device)
        self._labels = _Bank(num_class, self.device)
        self.num_anchors, self.dis_q = 10, 10             # ToyGraphBase.py:27-28
        self._positions = _Bank(self.num_anchors, self.device)   # position-aware codes of the sampled toy graphs (:114,119)
        self._keys_normalized = None  # cache: the current N-row tensor (made on first use; an append extends it by its rows), or None
        self._positions_normalized = None   # the same for the codes (read only when structure_weight != 0)
        self._kn_store = self._pn_store = None   # the growable stores the two caches are prefixes of
        self._index = None            # K.KeyIndex of this bank (packed / bf16 copies made on first use; an append extends it)
        # RAGraph_node/ragraph_utils/ToyGraphBase.py:28-29.  With structure_weight == 0 retrieval is the semantic top-k and
        # its scores are NOT scaled by semantic_weight, as in the reference's active code (:66-67); otherwise the score is
        # structure_weight * cos(position codes) + semantic_weight * cos(embeddings) (RAGraph_node_fewshot/.../ToyGraphBase.py:47-65)
        self.structure_weight = 0.0
        self.semantic_weight = 0.999
        # Position codes of the query graph (search_positions): None = to the fixpoint (graphs of more than 40000 nodes then
        # read a converged word back between batches of rounds, which a stream capture cannot record); R = exactly R
        # relaxation rounds and no read-back.  last_position_converged: the device int32 word of the last fixed-round call
        # (1 = the codes are final), never read back here.
        self.position_rounds = None
        self.last_position_converged = None

    # ---- bank state (attribute names of the reference) ---------------------------------------------------------
    @property
    def resource_keys(self) -> Tensor:
        return self._keys.view()

    @property
    def resource_values(self) -> Tensor:
        return self._values.view()

    @property
    def resource_labels(self) -> Tensor:
        return self._labels.view()

    @property
    def resource_positions(self) -> Tensor:
        return self._positions.view()

    def add_resources(self, keys: Tensor, values: Tensor, labels: Tensor, positions: Tensor | None = None) -> None:
        """Append rows to the bank (what ToyGraphBase.py:116-119 does with torch.cat)."""
        assert keys.shape[0] == values.shape[0] == labels.shape[0]
        n0, p0 = self._keys.n, self._positions.n
        self._keys.append(keys)
        self._values.append(values)
        self._labels.append(labels)
        if positions is not None:
            assert positions.shape[0] == keys.shape[0]
            self._positions.append(positions)
        # caches that exist grow by the new rows (normalised alone: a row's norm tree sees no other row); one that was never
        # read stays None and is made whole on first use
        if self._keys_normalized is not None:
            self._keys_normalized = self._extend_normalized(self._kn_store, self._keys, n0)
            if self._index is not None:
                self._index.extend(self._keys_normalized)
        else:
            self._index = None
        if self._positions_normalized is not None:
            self._positions_normalized = self._extend_normalized(self._pn_store, self._positions, p0)

    @staticmethod
    def _extend_normalized(store: _Bank, raw: _Bank, n0: int) -> Tensor:
        """Normalise raw's rows [n0, raw.n) into the store behind its n0 rows; the store's current view."""
        if raw.n > n0:
            K.normalize_rows(raw.buf[n0:raw.n], out=store.reserve(raw.n - n0))
        return store.buf[:store.n]

    @staticmethod
    def _adopt_normalized(rows: Tensor) -> _Bank:
        store = _Bank(rows.shape[1], rows.device)
        store.buf, store.n = rows, rows.shape[0]
        return store

    def set_resources(self, keys: Tensor, values: Tensor, labels: Tensor, positions: Tensor | None = None) -> None:
        """Adopt caller-owned device tensors as the bank without copying (e.g. a 1M-row synthetic bank).  Without
        `positions` the bank has no position codes (retrieval with structure_weight != 0 then raises)."""
        stores = [(self._keys, keys), (self._values, values), (self._labels, labels)]
        if positions is not None:
            if positions.shape[0] != keys.shape[0]:
                raise ValueError(f"set_resources: {positions.shape[0]} position rows for {keys.shape[0]} keys")
            stores.append((self._positions, positions))
        else:
            self._positions = _Bank(self._positions.buf.shape[1], self.device)
        for b, t in stores:
            b.buf, b.n = t.to(self.device, torch.float32).contiguous(), t.shape[0]
        self._reset_caches()

    def _reset_caches(self) -> None:
        self._keys_normalized = self._positions_normalized = self._index = self._kn_store = self._pn_store = None

    # ---- removal ------------------------------------------------------------------------------
    @property
    def retired_rows(self) -> int:
        """Physical rows removed (remove_resources) and still stored; the bank's index is the authority."""
        return 0 if self._index is None else self._index.retired_rows

    @property
    def num_resources(self) -> int:
        """The live rows: what retrieval answers over (resource_* stay physical until compact())."""
        return self._keys.n - self.retired_rows

    def remove_resources(self, rows) -> None:
        """Take the physical rows `rows` (ids over resource_keys: what topk returns) out of the bank.  With an index or a
        normalised cache alive the rows are RETIRED (K.KeyIndex.retire): nothing stored moves, every copy, duplicate group and
        learnt bound stays, and retrieval over-fetches by retired_rows and drops them (K.topk_drop_rows) -- until compact().
        A bank that has neither yet is simply compacted at once.  An id out of range raises IndexError before anything changes."""
        ids = torch.as_tensor(rows).detach().to("cpu", torch.int64).reshape(-1)
        n = self._keys.n
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n):
            raise IndexError(f"remove_resources: row ids outside [0, {n}) (lowest {int(ids.min())}, highest {int(ids.max())})")
        if not ids.numel():
            return
        if self._index is None and self._keys_normalized is None and self._positions_normalized is None:
            self._keep_rows(self._live_positions(ids))
            return
        if self._index is None:
            self._index = K.KeyIndex(self.keys_normalized)
        self._index.retire(ids)

    def _live_positions(self, retired: Tensor) -> Tensor:
        """The physical rows that are not in `retired` (host ids), ascending: an int64 device tensor."""
        live = torch.ones(self._keys.n, dtype=torch.bool, device=self.device)
        live[retired.to(self.device)] = False
        return K.mask_positions(live)

    def _keep_rows(self, live: Tensor) -> None:
        """Every store becomes its rows `live` (K.gather_rows: bit copies), one store at a time."""
        for bank in (self._keys, self._values, self._labels) + ((self._positions,) if self._positions.n else ()):
            bank.buf = K.gather_rows(bank.buf[:bank.n], live)
            bank.n = bank.buf.shape[0]
        # (a normalised row is a function of its own row alone: the gathered cache is the cache of the gathered rows, bit for bit)
        if self._keys_normalized is not None:
            self._keys_normalized = K.gather_rows(self._keys_normalized, live)
            self._kn_store = self._adopt_normalized(self._keys_normalized)
        if self._positions_normalized is not None:
            self._positions_normalized = K.gather_rows(self._positions_normalized, live)
            self._pn_store = self._adopt_normalized(self._positions_normalized)

    def compact(self):
        """Drop the retired rows from every store: keys, values, labels, the position codes when present, and the normalised
        key and code caches that exist; then K.KeyIndex.rebase (copies, groups and priors start over; demotions, re-probe
        clocks and counters stay).  Returns the int64 device tensor of live positions -- new row j was old row live[j] --, or None
        when nothing was retired.  The stores are gathered one at a time and each old store is released before the next is
        gathered: the peak extra memory is ONE store's worth (the widest: N x emb_size floats), not a second bank.  Reads the
        live count back (K.mask_positions): never under a stream capture."""
        if not self.retired_rows:
            return None
        live = self._live_positions(self._index.retired_ids)
        self._keep_rows(live)
        self._index.rebase(self.keys_normalized)
        return live

    def _compact_before_uniform_draws(self) -> None:
        """Noisy retrieval draws rows uniformly over the PHYSICAL rows and could draw a retired one: compact first."""
        if self.retired_rows:
            if K.KeyIndex._capturing():
                raise K.RagraphNativeError("noisy retrieval over a bank with retired rows compacts it first, which a stream "
                                           "capture cannot record: call compact() before capturing")
            self.compact()

    @property
    def keys_normalized(self) -> Tensor:
        if self._keys_normalized is None:
            self._keys_normalized = K.normalize_rows(self.resource_keys)
            self._kn_store = self._adopt_normalized(self._keys_normalized)
        return self._keys_normalized

    @property
    def positions_normalized(self) -> Tensor:
        """F.normalize(resource_positions), once per row (cosine_similarity re-normalises them on every call,
        RAGraph_node_fewshot/ragraph_utils/ToyGraphBase.py:51-53).  An all-zero code row stays zero."""
        if self._positions_normalized is None:
            self._positions_normalized = K.normalize_rows(self.resource_positions)
            self._pn_store = self._adopt_normalized(self._positions_normalized)
        return self._positions_normalized

    def _require_positions(self) -> None:
        n_pos, n_keys = self._positions.n, self._keys.n
        if n_pos != n_keys:
            raise ValueError(f"structure_weight = {self.structure_weight}: the bank holds {n_pos} position rows for {n_keys} "
                             "keys (resources added without positions, or a v1 bank file); retrieval by position codes "
                             "needs one per key")

    def search_positions(self, search_adj=None, search_positions: Tensor | None = None, anchors: Tensor | None = None):
        """The query rows' position codes when retrieval uses them (structure_weight != 0), else None: ready codes, or
        PositionAwareEncoder.py:6-24 on the query graph (`anchors`: drawn from the host generator when not given, as the
        reference does -- which a stream capture cannot record).  Raises before any kernel when the bank has no codes."""
        if self.structure_weight == 0:
            return None
        self._require_positions()
        if search_positions is not None:
            return search_positions
        if search_adj is None:
            raise ValueError("structure_weight != 0: retrieval needs the query graph (search_adj) or its position codes")
        if anchors is None and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise K.RagraphNativeError("structure-aware retrieval: pass `anchors` to a captured call (drawn on the host "
                                       "generator otherwise: PositionAwareEncoder.py:11)")
        from ..RAGraph_fewshot import PositionAwareEncoder
        if self.position_rounds is None:
            return PositionAwareEncoder.encode_position_aware_code(search_adj, self.num_anchors, self.dis_q, anchors)
        codes, self.last_position_converged = PositionAwareEncoder.encode_position_aware_code(
            search_adj, self.num_anchors, self.dis_q, anchors, rounds=self.position_rounds)
        return codes

    # ---- build (the step before the hot path; deterministic part) -----------------------------------------------
    def build_toy_graph(self, resource_dataset):
        """ToyGraphBase.py:40-45.  One resource graph per batch; the stochastic augmentation + inverse-importance
        sampling of the node flavour (ToyGraphBase.py:92-102) lives in ragraph_amd.bank_build."""
        from ..bank_build import build_toy_graph
        build_toy_graph(self, resource_dataset)

    # ---- retrieve (hot path) -----------------------------------------------------------------------------------
    def topk(self, search_keys: Tensor, k: int, search_positions: Tensor | None = None):
        """(scores [B,k], idx [B,k]) of the fused cosine + top-k kernel; canonical tie order.  With structure_weight != 0:
        of structure_weight * cos(search_positions, resource_positions) + semantic_weight * cos(search_keys, resource_keys)
        (K.topk_cosine_mix; `search_positions` [B, num_anchors] raw codes of the query rows)."""
        q = search_keys.reshape(1, -1) if search_keys.dim() == 1 else search_keys
        if self.structure_weight != 0:
            self._require_positions()
            if search_positions is None:
                raise ValueError("structure_weight != 0: topk needs the query rows' position codes (search_positions)")
        n_live = self.resource_keys.shape[0] - self.retired_rows   # (resource_keys: a captured step records that it reads the bank)
        if n_live < k:
            raise RuntimeError(f"selected index k out of range: bank has {n_live} rows, k={k}")
        # retired rows never move a call into a slower list class: past a ceiling the bank is compacted first (not under a
        # capture, where the over-fetch goes as far as TOPK_ORDERED_MAX)
        mixed_ceilings = (32, K.TOPK_ORDERED_MAX)   # (K.topk_cosine_mix: fused up to 32 keys, score slabs beyond)
        if self.retired_rows and not K.KeyIndex._capturing() and not self._index.overfetch_keeps_class(
                k, mixed_ceilings if self.structure_weight != 0 else None):
            self.compact()
        if self.structure_weight != 0:
            pos = search_positions.reshape(1, -1) if search_positions.dim() == 1 else search_positions
            if self._index is None and K.padded_dim(q.shape[1]) == q.shape[1]:   # (another width: no padded bank copy for this alone)
                self._index = K.KeyIndex(self.keys_normalized)
            if self._index is None:
                return self._topk_mix_exact(q, pos, k)
            # through the filter where that pays (K.KeyIndex.topk_mix: the same bits), else the exact call below
            return self._index.topk_mix(q, pos, self.positions_normalized, self.structure_weight, self.semantic_weight, k,
                                        self._topk_mix_exact)
        if self._index is None:
            self._index = K.KeyIndex(self.keys_normalized)
        return self._index.topk(q, k)  # fp32 streaming / tile kernel or, for large batches, the bf16-filtered exact path

    def _topk_mix_exact(self, q: Tensor, pos: Tensor, k: int):
        """The exact mixed top-k of the live rows (K.topk_cosine_mix: no filter, no read-back, capturable)."""
        r, n = self.retired_rows, self._keys.n
        if not r:
            return K.topk_cosine_mix(q, self.keys_normalized, pos, self.positions_normalized, self.structure_weight,
                                     self.semantic_weight, k)
        k_in = min(k + r, n)   # (this branch bypasses KeyIndex: the same over-fetch and the same drop around its own search)
        if k_in > K.TOPK_ORDERED_MAX:
            raise K.RagraphNativeError(f"topk: k={k} with {r} retired rows needs lists of {k_in} > {K.TOPK_ORDERED_MAX} "
                                       "keys: compact() the bank (not done under a stream capture)")
        s, i = K.topk_cosine_mix(q, self.keys_normalized, pos, self.positions_normalized, self.structure_weight,
                                 self.semantic_weight, k_in)
        s, i, _ = K.topk_drop_rows(s, i, self._index.retired_bitmap, n, k)
        return s, i

    def retrieve_indices(self, search_keys: Tensor, add_noise: bool, search_adj=None,
                         search_positions: Tensor | None = None, anchors: Tensor | None = None,
                         row_ids: Tensor | None = None, row_base: int = 0) -> Tensor:
        """The rows retrieve() gathers: the top-k' indices (k' = 2 * retrieve_num with add_noise, :66) and, in the node
        flavour with add_noise, noise_retrieve_num uniformly random rows behind them (:73-79).  The reference draws the
        noise from torch's default CPU generator (no device argument) and only then moves it to the bank's device: drawn
        the same way here, so torch.manual_seed reproduces the reference's rows.  With noise_rng = "device" the noise columns
        are K.noise_rows of a fresh seed (last_noise_seed), keyed by the query's row in the call -- or by `row_ids` /
        `row_base + b` when the caller holds a slice of a larger batch -- written into the tail of one [B, k' + m] matrix."""
        retrieve_num = 2 * self.retrieve_num if add_noise else self.retrieve_num
        if add_noise:
            self._compact_before_uniform_draws()
        pos = self.search_positions(search_adj, search_positions, anchors)         # (None unless structure_weight != 0)
        _, idx = self.topk(search_keys, retrieve_num, pos)                         # :66-67
        if add_noise and self.flavour == "node" and self.noise_rng == "device":
            B, k, m = idx.shape[0], idx.shape[1], self.noise_retrieve_num
            full = torch.empty((B, k + m), dtype=torch.int64, device=idx.device)
            full[:, :k] = idx
            K.noise_rows(self._draw_noise_seed(), B, m, self.resource_values.shape[0], row_ids, row_base, out=full[:, k:])
            return full
        if add_noise and self.flavour == "node":
            noise_idx = torch.randint(0, self.resource_values.shape[0], (idx.shape[0], self.noise_retrieve_num))
            idx = torch.cat([idx, noise_idx.to(idx.device)], dim=1)
        return idx

    def retrieve(self, search_keys: Tensor, search_adj, add_noise: bool, idx: Tensor | None = None,
                 search_positions: Tensor | None = None, anchors: Tensor | None = None,
                 row_ids: Tensor | None = None, row_base: int = 0):
        """ToyGraphBase.py:47-81 -> (rag_embeddings [B,k',D], rag_labels [B,k',C]).  A 1-D query (graph flavour,
        RAGraph_graph/ragraph_utils/ToyGraphBase.py:56-87) gives B = 1.  `idx`: the rows, when the caller already
        holds retrieve_indices(search_keys, add_noise) (one top-k per forward instead of two).  `search_adj` (the query
        graph), or ready `search_positions`, and `anchors` matter only with structure_weight != 0; `row_ids` / `row_base` key the
        noise of noise_rng = "device" (see retrieve_indices)."""
        if idx is None:
            idx = self.retrieve_indices(search_keys, add_noise, search_adj, search_positions, anchors, row_ids, row_base)
        rag_embeddings = K.gather_rows(self.resource_values, idx)                  # :70 (+ :76,78 noise rows)
        rag_labels = K.gather_rows(self.resource_labels, idx)                      # :71 (+ :77,79)
        if add_noise and self.flavour != "node" and self.noise_rng == "device":    # graph :84-85,131-134, drawn in the kernel
            rag_embeddings = K.add_normal_noise(rag_embeddings, self.noise_std, self._draw_noise_seed(), row_ids, row_base)
        elif add_noise and self.flavour != "node":                                 # graph :84-85,131-134
            noise = torch.normal(mean=0, std=self.noise_std, size=rag_embeddings.shape).to(rag_embeddings.device)
            rag_embeddings = K.axpby(rag_embeddings, 1.0, noise, 1.0)
        return rag_embeddings, rag_labels

    def retrieve_reduced_noisy(self, search_keys: Tensor, idx: Tensor | None = None, want_labels: bool = True,
                               search_adj=None, search_positions: Tensor | None = None, anchors: Tensor | None = None,
                               row_ids: Tensor | None = None, row_base: int = 0):
        """What RAGraph.forward consumes in noisy fine-tuning (RAGraph.py:42-49 with add_noise): (sum_k' V, mean_k' L)
        over the top-2k rows plus the noise -- every reduction on the HIP kernels, ONE top-k per call (`idx`: the rows
        when the caller already holds retrieve_indices(search_keys, True); want_labels=False skips the label means).
        Node flavour with noise_rng = "device" and no `idx`: the top-2k list alone goes into K.gather_reduce_noisy, which
        computes the noise rows itself -- the bits of the reduction over retrieve_indices' matrix for the same seed."""
        if idx is None:   # (a caller's own idx was made by retrieve_indices(search_keys, True), which compacted)
            self._compact_before_uniform_draws()
        if idx is None and self.flavour == "node" and self.noise_rng == "device":
            pos = self.search_positions(search_adj, search_positions, anchors)
            _, top = self.topk(search_keys, 2 * self.retrieve_num, pos)
            return K.gather_reduce_noisy(self.resource_values, self.resource_labels if want_labels else None, top,
                                         self._draw_noise_seed(), self.noise_retrieve_num, row_ids=row_ids, row_base=row_base)
        if idx is None:
            idx = self.retrieve_indices(search_keys, True, search_adj, search_positions, anchors, row_ids, row_base)
        if self.flavour == "node":   # noise = extra rows: still a gather-reduce over an index matrix
            return K.gather_reduce(self.resource_values, self.resource_labels, idx)
        rag_embeddings, _ = self.retrieve(search_keys, None, True, idx=idx, row_ids=row_ids, row_base=row_base)   # noise is
        # added to the gathered embeddings
        B, k, D = rag_embeddings.shape
        seg = torch.arange(0, B * k + 1, k, dtype=torch.int64, device=rag_embeddings.device)
        sum_v = K.segment_reduce(rag_embeddings.reshape(B * k, D), seg)
        mean_l = K.gather_reduce(self.resource_values, self.resource_labels, idx)[1] if want_labels else None
        return sum_v, mean_l

    def retrieve_reduced(self, search_keys: Tensor, k: int | None = None, search_adj=None,
                         search_positions: Tensor | None = None, anchors: Tensor | None = None):
        """What RAGraph.forward consumes (RAGraph.py:48-49): (sum_k V[idx] [B,D], mean_k L[idx] [B,C], idx) without
        materialising the [B,k,D] gather."""
        pos = self.search_positions(search_adj, search_positions, anchors)
        _, idx = self.topk(search_keys, self.retrieve_num if k is None else k, pos)
        sum_v, mean_l = K.gather_reduce(self.resource_values, self.resource_labels, idx)
        return sum_v, mean_l, idx

    # ---- persistence (the reference rebuilds its bank on every run) -------------------
    def save(self, path: str) -> None:
        """keys | values | labels | positions as one .pt, format v2 (the normalised caches are derived and rebuilt on
        load).  `positions` holds as many rows as the bank has codes for: all of them, or none.  Live rows only: a bank with
        retired rows is compacted first."""
        self.compact()
        torch.save({"format": "ragraph_amd.bank.v2", "keys": self.resource_keys.cpu(), "values": self.resource_values.cpu(),
                    "labels": self.resource_labels.cpu(), "positions": self.resource_positions.cpu()}, path)

    def load(self, path: str, append: bool = False) -> None:
        """Reads v2 and v1 files (v1 has no position codes: such a bank retrieves with structure_weight == 0 only)."""
        blob = torch.load(path, map_location="cpu")
        if blob.get("format") not in ("ragraph_amd.bank.v1", "ragraph_amd.bank.v2"):
            raise ValueError(f"{path}: not a ragraph_amd bank file")
        if not append:  # fresh stores: the old ones may be tensors adopted from the caller (set_resources)
            self._keys, self._values, self._labels, self._positions = (
                _Bank(b.buf.shape[1], self.device) for b in (self._keys, self._values, self._labels, self._positions))
            self._reset_caches()
        positions = blob.get("positions")
        if positions is not None and positions.shape[0] != blob["keys"].shape[0]:
            positions = None   # a bank saved without codes
        self.add_resources(blob["keys"], blob["values"], blob["labels"], positions)

    def show(self):
        print("resource_keys", self.resource_keys.shape)
        print("resource_values", self.resource_values.shape)
        print("resource_labels", self.resource_labels.shape)
        print("resource positions", self.resource_positions.shape)
        print("label count distribution", torch.sum(self.resource_labels, dim=0))
