"""The six-group int8 ring kernel at D = 256 with its query groups in two sets (csrc/filter_ring.h, SKEW): set A = groups 0-2 of
a wave, set B = groups 3-5, each with its own hit decision and candidate path, B's one step behind A's inside a stage.
RAGRAPH_FILTER_SKEW=0 keeps the kernel with one decision per sub-tile; every case runs under both.

The smallest shapes that reach six groups: ONE int8 level over the whole bank (the plan says so) with
ceil(B / 768) x stages >= 32 x CUs and at most 2 % padding queries -- asserted from ragraph_topk_cosine_filtered_plan below.

Winners are PLANTED: keys that are copies of chosen queries, so that their sub-tile takes the candidate path of the chosen
set.  A wave holds 96 consecutive queries (tile = 768 = 8 waves); query r of a wave is in set A when r < 48.  A stage is 128
keys, a sub-tile 32.  Workgroups cut a tile's key stream into segments of >= 8 stages at places this file does not know, so
windows of consecutive stages carry a winner in EVERY stage, in the first and the last sub-tile by turns: whatever stage
starts or ends a segment inside a window holds one.  Every case must have the indices and the score bits of K.topk_cosine.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

D, K_TOP = 256, 10
STAGE, SUB, QW, TILE = 128, 32, 96, 768


def _six_groups_by_the_plan(K, B, N):
    """The launch rule (filter_pass_variant) from the exported plan: one int8 level over [0, N) that takes tiles of 768."""
    L = K.N.lib()
    plan = (ctypes.c_int64 * 7)()
    assert L.ragraph_topk_cosine_filtered_plan(B, N, D, K_TOP, plan) == 1 and int(plan[3]) == N
    assert K.filtered_i8_levels(B, N, D, K_TOP) == 1
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    stages = -(-N // STAGE)
    tiles = -(-B // TILE)
    pad512 = -(-B // 512) * 512 - B
    assert tiles * stages >= 32 * cus, (tiles, stages, cus)
    assert (tiles * TILE - B - pad512) * 50 <= B


def _q_of(wave, r):
    """Query r (0 .. 95) of wave `wave` (counted over the whole batch: 8 waves per tile of 768)."""
    return wave * QW + r


def _plant(kn, qn, plants):
    """kn[key] = the normalised query q: an exact score of 1 -- the query's best key and far above any threshold."""
    for key, q in plants:
        kn[key] = qn[q]


def _bank(B, N, seed, dev):
    from ragraph_amd import kernels as K

    g = torch.Generator(device=dev).manual_seed(seed)
    kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
    q = torch.randn(B, D, device=dev, generator=g)
    return kn, q, K.normalize_rows(q)


def _sets_plants(B, N):
    """(key, query) pairs: set A only, set B only, both sets in one sub-tile, consecutive sub-tiles, first and last sub-tile of a
    stage, windows of stages with a winner in each, the bank's first and last stages."""
    nst = -(-N // STAGE)
    last_q = B - 1
    waves = -(-B // QW)
    out = []
    used = set()

    def put(stage, sub, off, q):
        key = stage * STAGE + sub * SUB + off
        if key < N and key not in used and q <= last_q:
            used.add(key)
            out.append((key, q))

    w = 0

    def nextw():
        nonlocal w
        w = (w + 5) % waves
        return w

    # set A only / set B only / both in the same sub-tile (same wave), in every sub-tile of a stage
    for sub in range(4):
        put(100 + sub, sub, 3, _q_of(nextw(), 7))             # A (group 0)
        put(110 + sub, sub, 17, _q_of(nextw(), 47))           # A (group 2, its last query)
        put(120 + sub, sub, 31, _q_of(nextw(), 48))           # B (group 3, its first query)
        put(130 + sub, sub, 0, _q_of(nextw(), 95))            # B (group 5)
        ww = nextw()
        put(140 + sub, sub, 5, _q_of(ww, 20))                 # both sets, one sub-tile, one wave
        put(140 + sub, sub, 21, _q_of(ww, 70))
    # consecutive sub-tiles of one wave: A then B, B then A, A A, B B (accumulators written again right behind a hit), and
    # across a stage boundary (last sub-tile, then the next stage's first)
    for i, (ra, rb) in enumerate([(10, 60), (60, 10), (10, 30), (60, 90)]):
        ww = nextw()
        for sub in range(3):
            put(200 + 4 * i, sub, 9, _q_of(ww, ra if sub % 2 == 0 else rb))
            put(200 + 4 * i, sub + 1, 9 + sub, _q_of(ww, rb if sub % 2 == 0 else ra))
        put(202 + 4 * i, 3, 30, _q_of(ww, ra))
        put(203 + 4 * i, 0, 1, _q_of(ww, rb))
    # windows of consecutive stages: a winner in every stage, first / last sub-tile by turns, sets by turns -- segment starts and
    # ends fall inside (a workgroup's share of a tile's stream is a few dozen stages at these shapes)
    for s0 in (0, nst // 3, nst - 90):
        for t in range(90):
            st = s0 + t
            if st >= nst:
                break
            put(st, 0 if t % 2 == 0 else 3, (7 * t) % SUB, _q_of(nextw(), (48 if t % 4 < 2 else 0) + (11 * t) % 48))
    # the bank's last stage (partly padded when N is no multiple of 128): its last real keys, both sets
    tail = N - 1
    ww = nextw()
    out.append((tail, min(last_q, _q_of(ww, 5))))
    if tail - 1 not in used:
        out.append((tail - 1, min(last_q, _q_of(ww, 77))))
    # the batch's last queries (a ragged last tile: its last wave is partly -- or wholly -- padding)
    put(300, 1, 2, last_q)
    put(301, 2, 2, last_q - 50)
    return out


_REF = {}


def _case(dev, B, N, seed, kind):
    """(kn, q, kb, reference scores, reference indices) of a planted case, built once and shared by the knob's two settings."""
    from ragraph_amd import kernels as K

    key = (B, N, seed, kind)
    if key not in _REF:
        _REF.clear()     # (one case's tensors at a time)
        kn, q, qn = _bank(B, N, seed, dev)
        if kind == "sets":
            _plant(kn, qn, _sets_plants(B, N))
        elif kind == "heavy":
            # a heavy granule (128 keys = one stage at D = 256; tests/test_gpu_i8_classes.py): rows with one dominant entry, so the
            # class changes on the stage boundaries around it; winners in the heavy stage, the stage before and the stage after,
            # in the last / first sub-tiles, both sets
            for gr in (37, 38, 900, N // STAGE - 1):
                r = gr * STAGE + 17
                v = 0.03 * torch.randn(D, device=dev, generator=torch.Generator(device=dev).manual_seed(gr))
                v[gr % D] = 1.0
                kn[r] = v / v.norm()
            plants = []
            for i, gr in enumerate((37, 38, 900, N // STAGE - 1)):
                for st, sub, off, r in ((gr - 1, 3, 31, 12), (gr - 1, 3, 30, 80), (gr, 0, 0, 40), (gr, 3, 5, 50), (gr, 1, 9, 2),
                                        (gr + 1, 0, 0, 90), (gr + 1, 0, 1, 33)):
                    k_ = st * STAGE + sub * SUB + off
                    if k_ < N:
                        plants.append((k_, _q_of((3 * i + sub) % (B // QW), r)))
            _plant(kn, qn, plants)
            # noisy copies of the heavy rows as queries: their winners ARE heavy keys
            q[5] = kn[37 * STAGE + 17] + 0.05 * torch.randn(D, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
            q[60] = kn[900 * STAGE + 17] + 0.05 * torch.randn(D, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        elif kind == "cluster":
            def noise(n, sd, seed):
                return sd * torch.randn(n, D, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))

            # all 96 queries of wave 9 near-duplicates of one another, and 300 near-duplicate keys of them: every lane of every
            # group of both sets has candidates in ten consecutive sub-tiles -- the wave's buffer fills and flushes INSIDE the loop
            q[_q_of(9, 0):_q_of(9, 0) + QW] = q[_q_of(9, 0)][None, :] + noise(QW, 0.02, 90)
            # two queries (set B of wave 20, set A of wave 21) that share 2300 near-duplicate keys: more than the 2048 slots of a
            # list -- both lists overflow into the fixup scan
            q[_q_of(21, 5)] = q[_q_of(20, 50)] + noise(1, 0.02, 91)[0]
            qn = K.normalize_rows(q)
            # the case as the issue states it: 300 near-duplicates of one query in consecutive keys, for a set A and a set B query
            for base, n, qi in ((5000, 300, _q_of(3, 13)), (131000, 300, _q_of(17, 66)), (60000, 300, _q_of(9, 0)),
                                (200000, 2300, _q_of(20, 50))):
                kn[base:base + n] = K.normalize_rows(qn[qi][None, :] + noise(n, 0.01, base))
        kb = K.keys_to_bf16(kn)
        s0, i0 = K.topk_cosine(q, kn, K_TOP)
        _REF[key] = (kn, q, kb, s0, i0)
    return _REF[key]


def _run(K, monkeypatch, skew, q, kn, kb, prior=None, tight=None):
    monkeypatch.setenv("RAGRAPH_FILTER_SKEW", skew)
    K.set_filter_prior(prior)
    K.set_filter_tight_prior(tight)
    try:
        s, i, over, st = K.topk_cosine_filtered(q, kn, kb, K_TOP, return_stats=True)
        w = st.cpu().tolist()
    finally:
        K.set_filter_prior(None)
        K.set_filter_tight_prior(None)
    return s, i, int(over), w


# B, N: scored lists / a ragged last tile (72 padding queries: the last wave holds 24) / plain lists (fewer than 2048 queries) /
# a partly padded last stage (N = 2047 stages + 84 keys)
SHAPES = [(3072, 262_144), (3000, 262_144), (1536, 524_288), (3072, 262_100)]


@pytest.mark.parametrize("skew", ["0", "1"])
@pytest.mark.parametrize("B,N", SHAPES)
def test_planted_winners_of_both_sets_bit_exact(dev, monkeypatch, B, N, skew):
    from ragraph_amd import kernels as K

    _six_groups_by_the_plan(K, B, N)
    kn, q, kb, s0, i0 = _case(dev, B, N, B + N, "sets")
    s, i, over, w = _run(K, monkeypatch, skew, q, kn, kb)
    assert torch.equal(i, i0) and torch.equal(s, s0)
    assert w[0] == K.FILTER_STATS_MAGIC and w[1] == 1 and w[8] == 1          # one level, on the int8 copy
    # the planted keys ARE winners (score 1 up to rounding): every planted query's best key is a planted key
    plants = _sets_plants(B, N)
    best = i0[:, 0].cpu()
    keys_of = {}
    for key, qq in plants:
        keys_of.setdefault(qq, set()).add(key)
    assert all(int(best[qq]) in ks for qq, ks in keys_of.items())


@pytest.mark.parametrize("skew", ["0", "1"])
def test_class_change_on_stage_boundaries_bit_exact(dev, monkeypatch, skew):
    from ragraph_amd import kernels as K

    B, N = 3072, 262_144
    _six_groups_by_the_plan(K, B, N)
    kn, q, kb, s0, i0 = _case(dev, B, N, 11, "heavy")
    c = K.int8_copy_classes(kb, N)
    assert 4 <= c["heavy_granules"] < c["granules"] // 8
    s, i, over, w = _run(K, monkeypatch, skew, q, kn, kb)
    assert torch.equal(i, i0) and torch.equal(s, s0)
    assert int(i0[5, 0]) == 37 * STAGE + 17 and int(i0[60, 0]) == 900 * STAGE + 17


@pytest.mark.parametrize("skew", ["0", "1"])
def test_cluster_of_near_duplicates_flushes_and_overflows_bit_exact(dev, monkeypatch, skew):
    from ragraph_amd import kernels as K

    B, N = 3072, 262_144
    _six_groups_by_the_plan(K, B, N)
    kn, q, kb, s0, i0 = _case(dev, B, N, 12, "cluster")
    s, i, over, w = _run(K, monkeypatch, skew, q, kn, kb)
    assert torch.equal(i, i0) and torch.equal(s, s0)
    assert 5000 <= int(i0[_q_of(3, 13), 0]) < 5300 and 131000 <= int(i0[_q_of(17, 66), 0]) < 131300
    assert all(60000 <= int(x) < 60300 for x in i0[_q_of(9, 0):_q_of(9, 0) + QW, 0])
    assert all(200000 <= int(i0[qq, 0]) < 202300 for qq in (_q_of(20, 50), _q_of(21, 5)))
    assert over >= 2, (over, w[:24])                       # 2300 candidates do not fit the 2048 slots of either list


@pytest.mark.parametrize("skew", ["0", "1"])
@pytest.mark.parametrize("what", ["prior below", "prior among", "tight below", "tight among"])
def test_forced_prior_and_tight_bound_bit_exact(dev, monkeypatch, what, skew):
    """A forced prior, a forced tight bound: each once below every k-th best score and once among them (queries it is too
    high for are repaired or scanned)."""
    from ragraph_amd import kernels as K

    B, N = 3072, 262_144
    kn, q, kb, s0, i0 = _case(dev, B, N, B + N, "sets")
    srt = torch.sort(s0[:, K_TOP - 1]).values
    below, among = float(srt[0]) - 0.01, float(srt[B // 8])
    prior, tight = {"prior below": (below, None), "prior among": (among, None),
                    "tight below": (below - 0.01, below), "tight among": (below, among)}[what]
    s, i, over, w = _run(K, monkeypatch, skew, q, kn, kb, prior, tight)
    assert torch.equal(i, i0) and torch.equal(s, s0)
    assert w[16] == 1
    if tight is not None:
        assert w[21] == 1 and w[22] == int((s0[:, K_TOP - 1] < tight).sum())
