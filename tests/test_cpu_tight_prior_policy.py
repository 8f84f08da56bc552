"""The host-side policy of the TIGHT speculative bound (ragraph_amd/kernels_index.py: KeyIndex._tight_for / _judge_tight) on
synthetic statistics words -- no GPU: when t appears, what it is, what widens its margin and what withdraws it."""
import struct

import torch

from ragraph_amd.kernels_index import KeyIndex

MAGIC = 0x52414753


def f2ord(x):
    b = struct.unpack("<i", struct.pack("<f", x))[0]
    return b if b >= 0 else b ^ 0x7FFFFFFF


class Ops:
    FILTER_STATS = True

    def set_filter_prior(self, p):
        pass

    def set_filter_tight_prior(self, t):
        pass


def words(spec, failed, lo, hi, tight=0, soft=0, repair=0, cand=100.0, B=4096):
    w = [0] * 32
    w[0], w[1] = MAGIC, 1
    w[2], w[5] = int(cand * 8), 8
    w[14], w[16], w[17], w[18], w[19] = B, spec, failed, f2ord(lo), f2ord(hi)
    w[21], w[22], w[23] = tight, soft, repair
    return w


def warm(lo=0.250, hi=0.290):
    idx = KeyIndex(torch.zeros(4, 64), ops=Ops(), dedup=False)
    idx._queries = 0
    for _ in range(2):
        idx._judge_prior(10, 512, words(0, 0, lo, hi), 0)
    return idx


def test_the_tight_bound_sits_a_small_margin_below_the_lowest_k_th_best_seen():
    idx = warm()
    p = idx._prior_for(4096, 10)
    t = idx._tight_for(4096, 10, p)
    assert abs(f2t(t) - (0.250 - KeyIndex.TIGHT_MARGIN)) < 1e-6 and t > p
    assert idx._tight_for(4096, 10, None) is None                 # no prior (not warm, withdrawn, capturing, RAGRAPH_SPEC=0): no t
    assert idx._tight_for(KeyIndex.TIGHT_MIN_BATCH - 1, 10, p) is None   # one level under the prior already: t would only add launches
    assert idx._tight_for(4096, 5, 0.2) is None                   # another k has its own history
    idx.tight_enabled = False
    assert idx._tight_for(4096, 10, p) is None                    # RAGRAPH_SPEC_TIGHT=0
    idx2 = warm(0.3000, 0.3001)                                  # a narrow spread: p = lowest - 0.01, t above it
    p2 = idx2._prior_for(4096, 10)
    assert idx2._tight_for(4096, 10, p2) > p2
    idx2._spec[10]["tight_margin"] = 0.02                        # a margin as wide as the prior's: nothing above the prior
    assert idx2._tight_for(4096, 10, p2) is None


def f2t(x):
    return float(x)


def test_ops_without_the_setter_never_get_a_tight_bound():
    idx = warm()

    class Old:
        FILTER_STATS = True

        def set_filter_prior(self, p):
            pass

    idx.ops = Old()
    assert idx._tight_for(4096, 10, idx._prior_for(4096, 10)) is None


def test_soft_misses_widen_the_margin_and_the_all_queries_repair_withdraws_it():
    idx = warm()
    p = idx._prior_for(4096, 10)
    t0 = idx._tight_for(4096, 10, p)
    idx._judge_prior(10, 512, words(1, 0, 0.251, 0.29, tight=1, soft=5, repair=1), 0)      # a handful: nothing changes
    assert idx._tight_for(4096, 10, p) == t0 and idx._spec[10]["soft"] == 5
    idx._judge_prior(10, 512, words(1, 0, 0.251, 0.29, tight=1, soft=KeyIndex.TIGHT_MAX_SOFT + 1, repair=1), 0)
    t1 = idx._tight_for(4096, 10, p)
    assert abs(t1 - (0.250 - 2 * KeyIndex.TIGHT_MARGIN)) < 1e-6                           # more than a few dozen: twice the margin
    assert idx._spec[10]["off_at"] is None                                                # ... and the prior stays
    idx._judge_prior(10, 512, words(1, 0, 0.251, 0.29, tight=1, soft=300, repair=2), 0)    # the all-queries level ran
    assert idx._tight_for(4096, 10, p) is None and idx._prior_for(4096, 10) is not None
    idx._queries += KeyIndex.REPROBE_QUERIES                                              # the interval passes: back, wider still
    assert abs(idx._tight_for(4096, 10, p) - (0.250 - 4 * KeyIndex.TIGHT_MARGIN)) < 1e-6
    for _ in range(12):                                                                    # the margin is bounded
        idx._judge_prior(10, 512, words(1, 0, 0.251, 0.29, tight=1, soft=100, repair=1), 0)
    assert idx._spec[10]["tight_margin"] == KeyIndex.TIGHT_MARGIN_MAX


def test_calls_without_a_tight_bound_are_not_judged_by_it():
    idx = warm()
    idx._judge_prior(10, 512, words(1, 0, 0.251, 0.29, tight=0, soft=999, repair=2), 0)
    assert "soft" not in idx._spec[10] and idx._spec[10].get("tight_off_at") is None
    idx._judge_prior(10, 512, words(1, 3, 0.251, 0.29, tight=1, soft=3, repair=1), 3)      # hard misses: the prior goes, t with it
    assert idx._prior_for(4096, 10) is None
    assert idx._tight_for(4096, 10, idx._prior_for(4096, 10)) is None
