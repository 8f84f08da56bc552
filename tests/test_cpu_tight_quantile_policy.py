"""The host-side policy that places the TIGHT bound at a soft-miss COUNT (ragraph_amd/kernels_index.py: KeyIndex._judge_tight /
_aim_tight / _tight_for) on synthetic statistics words -- no GPU.  The fake calls draw their words [22] and [24..28] from ONE
fixed low tail of k-th best scores, so a policy that moves t sees what a real bank would report at the new t."""
import math
import struct

import pytest
import torch

from ragraph_amd import filter_stats as FS
from ragraph_amd.kernels_index import KeyIndex

MAGIC = 0x52414753
K_, B_ = 10, 32768      # (the fake bank is 64 wide: t is aimed from 256 x 64 = 16384 queries)
LOWEST = 0.250          # the lowest k-th best of the fake bank's queries


def f2ord(x):
    b = struct.unpack("<i", struct.pack("<f", x))[0]
    return b if b >= 0 else b ^ 0x7FFFFFFF


def f2bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def below(x):
    """Queries of a fake call whose final k-th best is below x: none below LOWEST, then a count that doubles every 0.001 of
    score (2 at +0.001, 32 at +0.005, 256 at +0.008)."""
    return 0 if x <= LOWEST else int(2.0 ** ((x - LOWEST) / 0.001))


class Ops:
    FILTER_STATS = True

    def set_filter_prior(self, p):
        pass

    def set_filter_tight_prior(self, t):
        pass


def words(t, prior, tail=True, repair=None, count=below, B=B_):
    w = [0] * 32
    w[0], w[1] = MAGIC, 1
    w[2], w[5] = 800, 8
    w[14], w[16], w[17], w[18], w[19] = B, 1, 0, f2ord(LOWEST), f2ord(0.290)
    soft = count(t)
    w[21], w[22] = 1, soft
    w[23] = (0 if soft == 0 else (1 if soft <= 256 else 2)) if repair is None else repair
    if tail:
        delta = struct.unpack("<f", struct.pack("<f", (t - prior) / 16.0))[0]
        w[24] = f2bits(delta)
        for j, m in enumerate((1, 2, 4, 8)):
            w[25 + j] = count(t + m * delta)
    return w


def warm(target=None, monkeypatch=None):
    if target is not None:
        monkeypatch.setenv("RAGRAPH_TIGHT_TARGET_SOFT", str(target))
    idx = KeyIndex(torch.zeros(4, 64), ops=Ops(), dedup=False)
    idx._queries = 0
    for _ in range(2):
        w = [0] * 32
        w[0], w[1], w[2], w[5], w[14], w[18], w[19] = MAGIC, 1, 800, 8, 512, f2ord(LOWEST), f2ord(0.290)
        idx._judge_prior(K_, 512, w, 0)
    return idx


def polled_call(idx, **kw):
    """One call of the policy's loop: the bounds for this call, then its words polled.  Returns (t, prior, soft misses)."""
    p = idx._prior_for(B_, K_)
    t = idx._tight_for(B_, K_, p)
    w = words(t, p, **kw)
    idx._judge_prior(K_, B_, w, 0, t)
    return t, p, w[22]


def test_the_layout_of_the_tail_words():
    assert (FS.TAIL_DELTA, FS.TAIL_BELOW, FS.TAIL_STEPS) == (24, 25, (1, 2, 4, 8))
    w = words(0.251, 0.235)
    pts = FS.tail_points(w, 0.251)
    assert [c for _, c in pts] == [w[22], w[25], w[26], w[27], w[28]] and pts[0][0] == 0.251
    assert abs(pts[4][0] - (0.251 + 8 * 0.001)) < 1e-7 and FS.bits2f(w[24]) == pytest.approx(0.001, rel=1e-6)
    assert FS.tail_points(words(0.251, 0.235, tail=False), 0.251) is None      # word [24] = 0: not reported
    w[21] = 0
    assert FS.tail_points(w, 0.251) is None                                    # no tight bound was in force


def test_the_target_is_reached_within_two_polled_calls_from_a_t_without_soft_misses():
    idx = warm()
    T = idx.tight_target
    assert 0 < T <= KeyIndex.TIGHT_TARGET_SOFT_MAX == 64
    t0, p, soft0 = polled_call(idx)
    assert soft0 == 0 and abs(t0 - (LOWEST - KeyIndex.TIGHT_MARGIN)) < 1e-9     # the first t: today's rule
    t1, _, soft1 = polled_call(idx)
    t2, _, soft2 = polled_call(idx)
    assert t0 < t1 <= t0 + 8 * (t0 - p) / 16 + 1e-9                             # one edge span at the most
    assert T / 2 <= soft2 <= 2 * T, (t0, t1, t2, soft1, soft2)
    t3, _, soft3 = polled_call(idx)
    assert t3 == t2 and soft3 == soft2                                          # ... and stays there
    assert "tight_margin" not in idx._spec[K_]                                  # (no margin doubled on the way)


def test_t_never_passes_the_highest_edge_and_never_reaches_the_prior():
    idx = warm()
    never = lambda x: 0                                                          # a bank whose tail never shows up
    for _ in range(6):
        p = idx._prior_for(B_, K_)
        t = idx._tight_for(B_, K_, p)
        assert t is None or t > p
        if t is None:
            break
        idx._judge_prior(K_, B_, words(t, p, count=never), 0, t)
        nxt = idx._spec[K_]["tight_aimed"][0]
        assert nxt <= t + 8 * FS.bits2f(f2bits((t - p) / 16.0)) + 1e-9, (t, nxt)
    # a call whose every count is huge aims far down: the next t is today's rule, above the prior -- or none at all
    idx = warm()
    p = idx._prior_for(B_, K_)
    t = idx._tight_for(B_, K_, p)
    flood = lambda x: int(200 * 2.0 ** ((x - t) / 0.00001))
    idx._judge_prior(K_, B_, words(t, p, repair=1, count=flood), 0, t)
    assert idx._spec[K_]["tight_aimed"][0] < t
    t_next = idx._tight_for(B_, K_, p)
    assert t_next is not None and t_next > p and abs(t_next - (LOWEST - KeyIndex.TIGHT_MARGIN)) < 1e-9
    idx._spec[K_]["tight_aimed"] = (p - 1.0, B_)
    idx._spec[K_]["tight_margin"] = 0.5
    assert idx._tight_for(B_, K_, p) is None                                     # nothing above the prior: no t


def test_a_call_at_three_times_the_target_re_aims_downwards():
    idx = warm()
    T = idx.tight_target
    p = idx._prior_for(B_, K_)
    t_hot = LOWEST + 0.001 * math.log2(3 * T) + 1e-6
    assert 3 * T <= below(t_hot) <= 3 * T + 2
    idx._spec[K_]["tight_aimed"] = (t_hot, B_)
    t, _, soft = polled_call(idx)
    assert t == t_hot and soft >= 3 * T
    t_next, _, soft_next = polled_call(idx)                                      # re-aimed before the next call
    assert t_next < t_hot and T / 2 <= soft_next <= 2 * T, (t_next, soft_next)


def test_the_all_queries_repair_withdraws_t_as_before():
    idx = warm()
    polled_call(idx)
    polled_call(idx)
    assert idx._spec[K_].get("tight_aimed") is not None
    p = idx._prior_for(B_, K_)
    t = idx._tight_for(B_, K_, p)
    idx._judge_prior(K_, B_, words(t, p, repair=2, count=lambda x: 300), 0, t)
    assert idx._tight_for(B_, K_, p) is None and idx._prior_for(B_, K_) is not None
    assert idx._spec[K_]["tight_margin"] == 2 * KeyIndex.TIGHT_MARGIN and "tight_aimed" not in idx._spec[K_]
    idx._queries += KeyIndex.REPROBE_QUERIES                                     # the interval passes: today's rule, wider
    assert abs(idx._tight_for(B_, K_, p) - (LOWEST - 2 * KeyIndex.TIGHT_MARGIN)) < 1e-9


def test_words_without_the_tail_follow_the_old_rule():
    idx = warm()
    for _ in range(3):
        t, p, soft = polled_call(idx, tail=False)
        assert abs(t - (LOWEST - KeyIndex.TIGHT_MARGIN)) < 1e-9 and soft == 0
    assert "tight_aimed" not in idx._spec[K_]
    t = idx._tight_for(B_, K_, p)
    idx._judge_prior(K_, B_, words(t, p, tail=False, count=lambda x: KeyIndex.TIGHT_MAX_SOFT + 1), 0, t)
    assert abs(idx._tight_for(B_, K_, p) - (LOWEST - 2 * KeyIndex.TIGHT_MARGIN)) < 1e-9   # a flood: twice the margin
    idx = warm()
    t = idx._tight_for(B_, K_, idx._prior_for(B_, K_))
    idx._judge_prior(K_, B_, words(t, idx._prior_for(B_, K_)), 0)                # tail words, but the call's t is not known
    assert "tight_aimed" not in idx._spec[K_]


def test_a_target_of_zero_keeps_the_old_rule(monkeypatch):
    idx = warm(0, monkeypatch)
    assert idx.tight_target == 0
    for _ in range(3):
        t, p, soft = polled_call(idx)
        assert abs(t - (LOWEST - KeyIndex.TIGHT_MARGIN)) < 1e-9 and soft == 0
    assert "tight_aimed" not in idx._spec[K_]
    t = idx._tight_for(B_, K_, p)
    idx._judge_prior(K_, B_, words(t, p, count=lambda x: KeyIndex.TIGHT_MAX_SOFT + 1), 0, t)
    assert abs(idx._tight_for(B_, K_, p) - (LOWEST - 2 * KeyIndex.TIGHT_MARGIN)) < 1e-9
    assert warm(1000, monkeypatch).tight_target == 64                            # the target is at most a quarter of the repair


def test_the_other_switches_and_the_batch_rule_still_hold():
    idx = warm()
    polled_call(idx)
    polled_call(idx)
    p = idx._prior_for(B_, K_)
    assert idx._tight_for(B_, K_, p) > LOWEST                                    # aimed into the tail
    assert idx._tight_for(KeyIndex.TIGHT_MIN_BATCH - 1, K_, p) is None
    assert idx._tight_for(B_, K_, None) is None                                  # no prior (a capture, RAGRAPH_SPEC=0): no t
    idx.tight_enabled = False
    assert idx._tight_for(B_, K_, p) is None                                     # RAGRAPH_SPEC_TIGHT=0


def test_small_batch_classes_keep_the_old_rule_and_an_aimed_t_serves_its_own_batch_size():
    idx = warm()
    small = KeyIndex.TIGHT_TARGET_QUERIES_PER_DIM * 64 - 1
    assert small >= KeyIndex.TIGHT_MIN_BATCH
    p = idx._prior_for(small, K_)
    for _ in range(3):                                                           # tail words of a small call aim nothing
        t = idx._tight_for(small, K_, p)
        assert abs(t - (LOWEST - KeyIndex.TIGHT_MARGIN)) < 1e-9
        idx._judge_prior(K_, small, words(t, p, B=small), 0, t)
    assert "tight_aimed" not in idx._spec[K_]
    polled_call(idx)
    polled_call(idx)
    t_aimed, from_B = idx._spec[K_]["tight_aimed"]
    assert from_B == B_ and idx._tight_for(B_, K_, p) == t_aimed > LOWEST
    assert idx._tight_for(2 * B_, K_, p) == t_aimed                              # twice the queries: at most twice the soft misses
    assert abs(idx._tight_for(2 * B_ + 1, K_, p) - (LOWEST - KeyIndex.TIGHT_MARGIN)) < 1e-9   # more: the old rule, and its own aim
    assert abs(idx._tight_for(small, K_, p) - (LOWEST - KeyIndex.TIGHT_MARGIN)) < 1e-9        # the small class never sees it
