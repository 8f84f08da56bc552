"""Heavy ties through every ordered top-k entry: the canonical order (score descending, index ascending; csrc/topk_order.h) is
what makes the entries interchangeable, so each of them must break the SAME ties the same way.

Bank: 200 rows of D = 64 that are 8 distinct normalised rows, row j = distinct row j % 8 -- every score occurs 25 times, at
indices 8 apart, i.e. in different lanes, waves, tiles and (tail) on both sides of the seed.  Queries: two random ones and an
all-zero one (every score +0: the whole bank is one tie), as B = 3 and tiled to B = 130, the smallest batch beyond the
small-batch streaming kernel (SMALLB_MAX = 128 in csrc/topk_cosine.hip).

Expectation of every case, on the MATERIALISED scores S = linear(normalize_rows(q), bank) of that call (the same fmaf chains,
hence the same bits as the fused kernels' scores): indices = np.lexsort((index, -S))[:k] per row with -0 == +0, scores = S at
those indices up to the sign of a zero."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, D, DISTINCT = 200, 64, 8
SEED_ROWS = 100   # test_tail: the seed is the top-k of rows [0, 100), the tail is rows [100, 200)


@pytest.fixture(scope="module")
def tied(dev):
    """bank [200, 64] (device), {B: raw queries (device)}, {B: S [B, 200] (host)} -- computed once, read by every case."""
    from ragraph_amd import kernels as K

    rng = np.random.default_rng(20)
    rows = K.normalize_rows(torch.from_numpy(rng.standard_normal((DISTINCT, D), dtype=np.float32)).to(dev))
    bank = rows[torch.arange(N, device=dev) % DISTINCT].contiguous()
    q3 = rng.standard_normal((3, D), dtype=np.float32)
    q3[2] = 0.0
    qs = {B: torch.from_numpy(np.ascontiguousarray(np.resize(q3, (B, D)))).to(dev) for B in (3, 130)}
    S = {B: K.linear(K.normalize_rows(q), bank).cpu().numpy() for B, q in qs.items()}
    for B in S:
        assert all(np.array_equal(S[B][:, j], S[B][:, j % DISTINCT]) for j in range(N))         # the ties are exact
        assert not S[B][2].any() and not np.signbit(S[B][2]).any()                              # the zero query: all +0
        S[B].setflags(write=False)
    return bank, qs, S


def canonical(S, k):
    """(scores, indices) [B, k] of the canonical order on the rows of S, -0 and +0 one score."""
    Sz = S + np.float32(0.0)   # (-0 + +0 = +0)
    idx = np.stack([np.lexsort((np.arange(S.shape[1]), -row))[:k] for row in Sz])
    return np.take_along_axis(S, idx, axis=1), idx


def check(got_s, got_i, S, k, what):
    ref_s, ref_i = canonical(S, k)
    got_s, got_i = got_s.cpu().numpy(), got_i.cpu().numpy()
    assert np.array_equal(got_i, ref_i), (what, np.argwhere(got_i != ref_i)[:5])
    assert np.array_equal(got_s, ref_s), what   # (values: bitwise up to the sign of a zero, there is no NaN)
    assert np.array_equal(got_s.view(np.uint32) & 0x7FFFFFFF, ref_s.view(np.uint32) & 0x7FFFFFFF), what


@pytest.mark.parametrize("k", [1, 10])
def test_small_batch_streaming_kernel(dev, tied, monkeypatch, k):
    """K.topk_cosine at B = 3.  With RAGRAPH_TOPK_SLAB=0 (takes_slabs: fused width, k <= 32, slab rule off) plan_topk takes
    use_streaming (B <= 128, 8 x (16.5 KiB tile + 128 k B of lists) <= 160 KiB): topk_smallb_kernel<64>, one workgroup (200 keys
    are 4 tiles of 64, fewer than the 16 that eight waves take two each of), whose eight wave lists -- lane-private inserts while the lists fill, cooperative ones after -- are
    merged in the kernel; launch_merge_sorted writes the one partial list out."""
    from ragraph_amd import kernels as K

    bank, qs, S = tied
    monkeypatch.setenv("RAGRAPH_TOPK_SLAB", "0")
    check(*K.topk_cosine(qs[3], bank, k), S[3], k, f"smallb k={k}")


def test_tile_kernel(dev, tied, monkeypatch):
    """K.topk_cosine at B = 130, k = 10.  With RAGRAPH_TOPK_SLAB=0, B > SMALLB_MAX leaves use_streaming: topk_stream_kernel<64, 3>
    (no packed copy; the three-slot ring fits at k = 10), one query tile of 256, its partial lists selected by
    launch_select (topk_select_kernel)."""
    from ragraph_amd import kernels as K

    bank, qs, S = tied
    monkeypatch.setenv("RAGRAPH_TOPK_SLAB", "0")
    check(*K.topk_cosine(qs[130], bank, 10), S[130], 10, "tile kernel")


@pytest.mark.parametrize("B,k", [(3, 1), (3, 10), (130, 10)])
def test_slab_rule(dev, tied, monkeypatch, B, k):
    """The same calls as the dispatch rule sends them: use_slab (B <= 128 x N <= 8192; B >= 8 and B N <= 2^26 at D = 64) takes
    slab_topk -- ragraph_linear_f32 into a score slab, one key chunk, topk_rows_kernel."""
    from ragraph_amd import kernels as K

    bank, qs, S = tied
    monkeypatch.delenv("RAGRAPH_TOPK_SLAB", raising=False)
    check(*K.topk_cosine(qs[B], bank, k), S[B], k, f"slab B={B} k={k}")


@pytest.mark.parametrize("B", [3, 130])
@pytest.mark.parametrize("k", [1, 10])
def test_tail(dev, tied, k, B):
    """K.topk_cosine_tail: seed = the canonical top-k of rows [0, 100), tail = rows [100, 200), so every tied score has
    members in the seed AND in the tail.  tail_plan: 100 rows at D = 64 are 2 tiles <= 32, so S = 1: topk_tail_kernel<64>, one
    workgroup per 16 queries (1 / 9 groups), its four wave lists merged with the seed by rank (merge_ranked)."""
    from ragraph_amd import kernels as K

    bank, qs, S = tied
    seed_s, seed_i = canonical(S[B][:, :SEED_ROWS], k)
    got = K.topk_cosine_tail(qs[B], bank[SEED_ROWS:].contiguous(), torch.from_numpy(seed_s).to(dev),
                             torch.from_numpy(seed_i).to(dev), SEED_ROWS)
    check(*got, S[B], k, f"tail B={B} k={k}")


@pytest.fixture(scope="module")
def signed_zeros(dev, tied):
    """S of the B = 3 batch with a -0 / +0 mix in the zero query's row (one 200-way tie of zeros): host copy, device copy."""
    Sz = tied[2][3].copy()
    Sz[2, [0, 3, 4, 9, 10, 11, 29, 30, 63, 64, 127, 199]] = -0.0
    assert np.signbit(Sz[2]).sum() == 12 and not Sz[2].any()
    Sz.setflags(write=False)
    return Sz, torch.from_numpy(Sz.copy()).to(dev)


@pytest.mark.parametrize("k", [1, 10, 64])
def test_rows(dev, signed_zeros, k):
    """K.topk_rows on the materialised matrix, k <= TOPK_MAX = 64: topk_rows_kernel (one workgroup per row, four wave lists
    with the cooperative insert, merged by wave 0).  The zeros of either sign are one score: row 2 answers 0 .. k-1."""
    from ragraph_amd import kernels as K

    Sz, Sd = signed_zeros
    got = K.topk_rows(Sd, k)
    check(*got, Sz, k, f"rows k={k}")
    assert np.array_equal(got[1][2].cpu().numpy(), np.arange(k))


def test_select_rows(dev, signed_zeros):
    """K.topk_select_rows at k = 30 on the same matrix: N = 200 < 65536 takes topk_select_rows_kernel (radix select over
    order_key, then the ordered pass).  It returns the k-th score and the SET in ascending index order."""
    from ragraph_amd import kernels as K

    Sz, Sd = signed_zeros
    kth, idx = K.topk_select_rows(Sd, 30)
    ref_s, ref_i = canonical(Sz, 30)
    assert np.array_equal(idx.cpu().numpy(), np.sort(ref_i, axis=1))
    assert np.array_equal(kth.cpu().numpy(), ref_s[:, -1])
