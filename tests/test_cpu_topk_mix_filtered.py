"""Mixed retrieval through the filter (ragraph_topk_mix_rerank_f32, KeyIndex.topk_mix), the parts that need no GPU: the ABI,
argument validation, the rule itself restated in numpy over cref scores on the GPU tests' inputs, and the host logic of
KeyIndex.topk_mix on an ops object answered by the C checker."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mix_rerank_reference as R
from oracle import cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ragraph_topk_mix_rerank_workspace_bytes", "ragraph_topk_mix_rerank_f32", "ragraph_topk_rows_scatter_f32")


def _lib():
    from ragraph_amd import _native

    return _native, _native.lib()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- 1: the ABI ----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    header = open(os.path.join(ROOT, "include", "ragraph_hip.h")).read()
    native, lib = _lib()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", header), name + " is not declared in ragraph_hip.h"
        assert name in native.SIGNATURES
        assert getattr(lib, name) is not None
    assert "RAGraph_node_fewshot/ragraph_utils/ToyGraphBase.py:47-65" in header[header.index("Structure-aware retrieval from a semantic"):
                                                                                header.index("ragraph_topk_mix_rerank_workspace_bytes")]
    makefile = open(os.path.join(ROOT, "ragraph_amd", "csrc", "Makefile")).read()
    # (headers such as mix_slack.h are no hand-kept list any more: every object's dependencies come from the compiler)
    assert "topk_mix_rerank.hip" in makefile and "-MMD" in makefile and "-include $(OBJS:.o=.d)" in makefile
    deps = os.path.join(ROOT, "ragraph_amd", "csrc", "topk_mix_rerank.d")
    assert not os.path.exists(deps) or "mix_slack.h" in open(deps).read()
    # the slack is stated once, in the shared header
    csrc = os.path.join(ROOT, "ragraph_amd", "csrc")
    for f in ("topk_cosine.hip", "topk_mix_rerank.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert "mix_slack_of(" in text and "1.0 / 1024" not in text, f


def test_workspace_holds_the_normalised_query_codes():
    _, lib = _lib()
    for B, A in ((1, 1), (70, 10), (100000, 16)):
        assert B * A * 4 <= lib.ragraph_topk_mix_rerank_workspace_bytes(B, A) < B * A * 4 + 256
    for bad in ((0, 10), (4, 0), (4, 17)):
        assert lib.ragraph_topk_mix_rerank_workspace_bytes(*bad) == 0


def test_argument_validation_returns_einval_without_a_device():
    native, lib = _lib()
    buf = (ctypes.c_char * 8192)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16   # never dereferenced: every case must be refused before any launch
    b = a + 4096

    def call(sem=a, idx=a, pq=a, pn=a, A=10, kl=32, k=10, ws_w=0.3, wm_w=0.7, out_s=b, out_i=b, flags=b, count=b, ws=b,
             ws_bytes=1 << 40, base=0):
        return lib.ragraph_topk_mix_rerank_f32(sem, idx, 4, kl, pq, pn, 100, A, ws_w, wm_w, k, base, out_s, out_i, flags, count,
                                               ws, ws_bytes, None)

    for name in ("sem", "idx", "pq", "pn", "out_s", "out_i", "flags", "count", "ws"):
        assert call(**{name: None}) == native.EINVAL and "null" in native.last_error(), name
    assert call(k=32) == native.EINVAL and "k=32" in native.last_error()        # k >= k'
    assert call(k=40) == native.EINVAL
    assert call(k=0) == native.EINVAL
    assert call(kl=129, k=10) == native.EINVAL and "129" in native.last_error()  # k' > 128
    assert call(A=0) == native.EINVAL and "A=0" in native.last_error()
    assert call(A=17) == native.EINVAL
    assert call(wm_w=0.0) == native.EINVAL and "w_sem" in native.last_error()
    assert call(wm_w=-0.7) == native.EINVAL
    assert call(wm_w=float("inf")) == native.EINVAL
    assert call(wm_w=float("nan")) == native.EINVAL
    assert call(ws_w=float("nan")) == native.EINVAL and "w_struct" in native.last_error()
    assert call(ws_w=float("inf")) == native.EINVAL
    assert call(base=-1) == native.EINVAL
    assert call(out_s=a) == native.EINVAL and "alias" in native.last_error()
    assert call(ws_bytes=8) == native.EWORKSPACE and "workspace" in native.last_error()
    # the row scatter
    assert lib.ragraph_topk_rows_scatter_f32(a, a, a, 3, 10, 4, None, b, None) == native.EINVAL
    assert lib.ragraph_topk_rows_scatter_f32(None, a, a, 3, 10, 4, b, b, None) == native.EINVAL
    assert lib.ragraph_topk_rows_scatter_f32(a, a, a, 3, 0, 4, b, b, None) == native.EINVAL
    assert lib.ragraph_topk_rows_scatter_f32(None, None, None, 0, 10, 4, b, b, None) == native.OK    # nothing to write


# ---- 2: the rule, in numpy over cref scores, on the GPU tests' inputs ---------------------------------------------------
@pytest.mark.parametrize("ws,wm", R.WEIGHTS)
def test_proven_rows_hold_the_oracle_s_bits_and_the_counts_are_where_the_gpu_tests_need_them(ws, wm):
    q, kn, pq, pnn, sem, struct = R.route_inputs()
    sem_s, sem_i = cref.topk_rows(sem, R.KL0)
    s, i, unproven = R.np_rerank(sem_s, sem_i, pq, pnn, ws, wm, R.K0)
    os_, oi = R.oracle_mixed_topk(sem, struct, ws, wm, R.K0)
    proven = unproven == 0
    assert np.array_equal(i[proven], oi[proven]) and np.array_equal(_bits(s[proven]), _bits(os_[proven]))
    n_un = int(unproven.sum())
    print(f"weights ({ws}, {wm}): {n_un} of {R.B0} rows unproven")
    assert n_un == R.UNPROVEN0[(ws, wm)]
    differs = (np.sort(oi, 1) != np.sort(sem_i[:, :R.K0], 1)).any(1)
    if (ws, wm) == (0.02, 0.98):
        assert n_un == 0 and differs.sum() >= 1       # proven everywhere although the structural term changes answers
    elif (ws, wm) == (0.05, 0.95):
        assert 0 < n_un < R.B0
    else:
        assert n_un == R.B0
        assert ((i != oi).any(1)).sum() >= 1          # (and rightly so: the candidate lists miss winners at these weights)


def test_restatement_orders_ties_by_index_and_flags_non_finite_rows():
    pnn = cref.normalize_rows(np.array([[1, 0], [1, 0], [0, 1], [0, 0], [1, 1]], dtype=np.float32))
    pq = np.array([[2, 0]], dtype=np.float32)
    sem_s = np.array([[0.5, 0.5, 0.5, 0.25]], dtype=np.float32)
    sem_i = np.array([[1, 4, 0, 2]], dtype=np.int64) + 7      # (not a canonical list: the restatement orders by what it computes)
    s, i, u = R.np_rerank(sem_s, sem_i, pq, pnn, 0.5, 0.5, 2, idx_base=7)
    assert i.tolist() == [[7, 8]] and s.tolist() == [[0.75, 0.75]]  # rows 0 and 1 tie at 0.5 + 0.25: the lower index first
    assert u.tolist() == [0]                                        # 0.75 > bound = 0.125 + slack(0.5) = 0.6255
    s, i, u = R.np_rerank(sem_s, sem_i, pq, pnn, 0.5, 0.5, 3, idx_base=7)
    assert i.tolist() == [[7, 8, 11]] and u.tolist() == [1]         # third best 0.5 / sqrt 2 + 0.25 = 0.6036 is not above it
    bad = sem_s.copy()
    bad[0, 0] = np.inf
    assert R.np_rerank(bad, sem_i, pq, pnn, 0.5, 0.5, 2, idx_base=7)[2].tolist() == [1]
    assert float(R.np_slack(0.25)) > 0.25 * (1 + 2.0 ** -10) and float(R.np_slack(-0.25)) == float(R.np_slack(0.25))


# ---- 3: host logic of KeyIndex.topk_mix --------------------------------------------------------------------------------
class MixOps:
    """The entries KeyIndex.topk_mix needs, on torch CPU tensors: the filtered call is cref's exact top-k, the rerank the numpy
    restatement; every call is counted."""

    calls = {}

    @classmethod
    def _count(cls, name):
        cls.calls[name] = cls.calls.get(name, 0) + 1

    @staticmethod
    def topk_cosine(q, kn, k, idx_base=0):
        MixOps._count("topk_cosine")
        s, i = cref.topk_cosine(q.numpy(), kn.numpy(), k, idx_base)
        return torch.from_numpy(s), torch.from_numpy(i)

    @staticmethod
    def filter_helps(B, n, D, k):
        return k <= 32

    @staticmethod
    def keys_to_bf16(kn):
        return kn

    @staticmethod
    def topk_cosine_filtered(q, kn, kb, k, idx_base=0, keys_packed=None):
        MixOps._count("topk_cosine_filtered")
        s, i = cref.topk_cosine(q.numpy(), kn.numpy(), k, idx_base)
        return torch.from_numpy(s), torch.from_numpy(i), torch.zeros(1, dtype=torch.int32)

    @staticmethod
    def mix_filter_list(k):
        from ragraph_amd import kernels as K

        return K.mix_filter_list(k)

    @staticmethod
    def mix_filter_helps(B, n, D, k):
        from ragraph_amd import kernels as K

        return K.mix_filter_helps(B, n, D, k)

    @staticmethod
    def topk_mix_rerank(sem_s, sem_i, pos_q, pos_normalized, w_struct, w_sem, k, idx_base=0):
        MixOps._count("topk_mix_rerank")
        s, i, u = R.np_rerank(sem_s.numpy(), sem_i.numpy(), pos_q.numpy(), pos_normalized.numpy(), w_struct, w_sem, k, idx_base)
        return torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(u), torch.tensor([int(u.sum())], dtype=torch.int32)

    @staticmethod
    def mask_positions(mask):
        return torch.nonzero(mask).reshape(-1)

    @staticmethod
    def gather_rows(v, idx):
        MixOps._count("gather_rows")
        return v[idx]

    @staticmethod
    def scatter_topk_rows_(s, i, pos, rs, ri):
        MixOps._count("scatter_topk_rows_")
        s[pos], i[pos] = rs, ri
        return s, i


class Bank:
    """A small bank, its index over MixOps and the exact mixed call (the oracle's), counted."""

    def __init__(self, monkeypatch, n=300, B=64, D=64, A=10, seed=5, measured=True):
        from ragraph_amd import kernels as K
        from ragraph_amd.kernels_index import KeyIndex

        monkeypatch.setattr(K, "mix_filter_measured", lambda *shape: measured)
        monkeypatch.delenv("RAGRAPH_MIX_FILTER", raising=False)
        monkeypatch.delenv("RAGRAPH_EXACT_FP32", raising=False)
        self.q, self.kn, self.pq, self.pnn = R.make_inputs(seed, B, n + 40, D, A)
        self.n, self.exact_rows = n, []
        self.index = KeyIndex(torch.from_numpy(self.kn[:n]), ops=MixOps, dedup=False)
        MixOps.calls = {}

    def exact_for(self, ws, wm):
        def exact(q, pos, k):
            self.exact_rows.append(int(q.shape[0]))
            n = self.n
            sem = cref.linear(cref.normalize_rows(q.numpy()), self.kn[:n])
            struct = cref.linear(cref.normalize_rows(pos.numpy()), self.pnn[:n])
            s, i = R.oracle_mixed_topk(sem, struct, ws, wm, k)
            return torch.from_numpy(s), torch.from_numpy(i)
        return exact

    def unproven(self, ws, wm, k=4):
        """What the restatement says of this bank's rows at these weights."""
        sem_s, sem_i = cref.topk_cosine(self.q, self.kn[:self.n], min(128, max(32, 2 * k)))
        return int(R.np_rerank(sem_s, sem_i, self.pq, self.pnn[:self.n], ws, wm, k)[2].sum())

    def call(self, ws, wm, k=4):
        got = self.index.topk_mix(torch.from_numpy(self.q), torch.from_numpy(self.pq), torch.from_numpy(self.pnn[:self.n]), ws, wm, k,
                                  self.exact_for(ws, wm))
        want = self.exact_for(ws, wm)(torch.from_numpy(self.q), torch.from_numpy(self.pq), k)
        self.exact_rows.pop()
        assert torch.equal(got[1], want[1]) and np.array_equal(_bits(got[0].numpy()), _bits(want[0].numpy()))
        return got


def test_route_is_taken_proves_rows_and_repairs_the_rest(monkeypatch):
    bank = Bank(monkeypatch)
    st = bank.index.mix_stats
    assert st == {"filtered_calls": 0, "exact_calls": 0, "rows_unproven": 0, "demotions": 0}
    bank.call(0.001, 0.999)
    assert st["filtered_calls"] == 1 and st["exact_calls"] == 0 and MixOps.calls["topk_cosine_filtered"] == 1
    assert st["rows_unproven"] == 0 and bank.exact_rows == [] and "scatter_topk_rows_" not in MixOps.calls
    # weights at which SOME rows are unproven: exactly those go to the exact call and are written back
    for ws in (0.06, 0.08, 0.1, 0.11, 0.12, 0.13, 0.14, 0.15):   # (32 of 300 keys listed: the bound is loose on so small a bank)
        wm = 1.0 - ws
        n_un = bank.unproven(ws, wm)
        if 0 < n_un <= bank.index.MIX_FILTER_MAX_UNPROVEN * bank.q.shape[0]:
            break
    else:
        pytest.fail("no weights with a small positive unproven count on this data: change the seed")
    before = st["rows_unproven"]
    bank.call(ws, wm)
    assert st["filtered_calls"] == 2 and st["rows_unproven"] == before + n_un and bank.exact_rows == [n_un]
    assert MixOps.calls["scatter_topk_rows_"] == 1 and MixOps.calls["gather_rows"] == 2 and st["demotions"] == 0


def test_route_is_refused_for_weights_k_and_switches(monkeypatch):
    bank = Bank(monkeypatch)
    st = bank.index.mix_stats
    bank.call(0.3, 0.0)                                # w_sem = 0
    bank.call(0.3, -0.7)                               # w_sem < 0
    assert st["exact_calls"] == 2 and st["filtered_calls"] == 0 and bank.exact_rows == [64, 64]
    bank.call(0.001, 0.999, k=65)                      # k > 64
    assert st["exact_calls"] == 3 and st["filtered_calls"] == 0
    monkeypatch.setenv("RAGRAPH_MIX_FILTER", "0")      # read per call
    bank.call(0.001, 0.999)
    assert st["exact_calls"] == 4 and st["filtered_calls"] == 0
    monkeypatch.delenv("RAGRAPH_MIX_FILTER")
    monkeypatch.setenv("RAGRAPH_EXACT_FP32", "1")
    bank.call(0.001, 0.999)
    assert st["exact_calls"] == 5 and st["filtered_calls"] == 0
    monkeypatch.delenv("RAGRAPH_EXACT_FP32")
    bank.call(0.001, 0.999)
    assert st["exact_calls"] == 5 and st["filtered_calls"] == 1
    assert "topk_mix_rerank" in MixOps.calls and MixOps.calls["topk_mix_rerank"] == 1
    # the measured rule is what keeps a shape out
    assert Bank(monkeypatch, measured=False).index._mix_filter_open(64, 4, 32, 0.001, 0.999) is False
    # a route that is not a filtered one (k' = 64 here: MixOps has no wide rule) is refused as well
    bank2 = Bank(monkeypatch)
    bank2.call(0.001, 0.999, k=20)
    assert bank2.index.mix_stats["exact_calls"] == 1 and bank2.index.mix_stats["filtered_calls"] == 0


def test_demotion_follows_an_over_threshold_share_and_is_lifted_when_rows_or_weights_change(monkeypatch):
    bank = Bank(monkeypatch)
    st = bank.index.mix_stats
    B = bank.q.shape[0]
    n_un = bank.unproven(0.3, 0.7)
    assert n_un > bank.index.MIX_FILTER_MAX_UNPROVEN * B
    bank.call(0.3, 0.7)                                # (nearly) every row unproven: answered exactly, and demoted
    assert st == {"filtered_calls": 1, "exact_calls": 0, "rows_unproven": n_un, "demotions": 1} and bank.exact_rows == [n_un]
    bank.call(0.3, 0.7)                                # straight to the exact call
    assert st["filtered_calls"] == 1 and st["exact_calls"] == 1 and MixOps.calls["topk_mix_rerank"] == 1
    bank.call(0.3, 0.7, k=5)                           # another k is judged for itself
    assert st["filtered_calls"] == 2 and st["demotions"] == 2
    # the rows change: the demotion is lifted (and earned again)
    bank.n += 40
    bank.index.extend(torch.from_numpy(bank.kn[:bank.n]))
    bank.call(0.3, 0.7)
    assert st["filtered_calls"] == 3 and st["exact_calls"] == 1 and st["demotions"] == 3
    bank.call(0.3, 0.7)
    assert st["filtered_calls"] == 3 and st["exact_calls"] == 2
    # the weights change: judged anew, and the old verdict is forgotten with them
    bank.call(0.001, 0.999)
    assert st["filtered_calls"] == 4 and st["demotions"] == 3
    bank.call(0.3, 0.7)
    assert st["filtered_calls"] == 5 and st["demotions"] == 4
    # rebase (the owner compacted the rows) lifts it too
    bank.index.rebase(torch.from_numpy(bank.kn[:bank.n]))
    bank.call(0.3, 0.7)
    assert st["filtered_calls"] == 6 and st["demotions"] == 5
