"""The ring kernel's two-part plan (segment_plan.h: RING_SPLIT -- every XCD group walks qtiles / 8 query tiles, the leftover
tiles are cut over all workgroups) on the smallest shapes that take it: 65, 67 and 71 query tiles (1, 3, 7 left over) of every
tile width the launch table uses (512 / 768 / 1024 queries; no launch uses 256) against banks of ~300 stages (~470 for the 7
left over: at 301 stages the planner keeps the XCD groups) -- under 256 stages the leftover pieces' floor of lb_min = 8 stages
makes the split no better than XCD groups alone, and launch_ring keeps those.  tests/test_cpu_ring_plan.py asserts the plan of
each (tiles, stages) pair below.  Every row must have the indices and the score bits of K.topk_cosine.
Also here: the zero-query count of the statistics words ([15]) over repeated calls."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# what, B, N, D, k, switches (read per call), call: "plain" (bound pass + levels), "prior", "tight_many" (soft misses beyond the
# 256-query repair: the gated all-queries ring level runs), "tight_few" (~100 soft misses: the compact repair)
# B = tiles x width - 100 (- 200 at width 1024): the last tile's last wave holds no query.  N is no multiple of a stage.
CASES = [
    # 65 tiles x 301 stages: the leftover tile in 8-stage pieces on 38 workgroups, 218 get nothing
    ("bf16 D=256, tiles of 512, 1 left", 65 * 512 - 100, 19_230, 256, 10, {}, "plain"),
    # last level [16384, N) on int8: 67 tiles x 301 stages, pipelined epilogue, scored lists
    ("int8 pipelined D=256, tiles of 512, 3 left", 67 * 512 - 100, 54_850, 256, 10,
     {"RAGRAPH_FILTER_I8": "1", "RAGRAPH_FILTER_PIPE": "2"}, "plain"),
    ("int8 six groups D=256, tiles of 768, 3 left", 67 * 768 - 100, 54_850, 256, 10, {"RAGRAPH_FILTER_I8": "1"}, "prior"),
    # 71 tiles x 474 stages (two levels) or 602 (one)
    ("bf16 D=128, tiles of 512, 7 left", 71 * 512 - 100, 77_000, 128, 5, {"RAGRAPH_FILTER_I8": "0"}, "prior"),
    ("int8 six groups D=128, tiles of 768, 3 left", 67 * 768 - 100, 93_300, 128, 5, {"RAGRAPH_FILTER_I8": "1"}, "plain"),
    # one level over [0, N): 65 tiles x 301 stages
    ("bf16 D=64, tiles of 1024, 1 left", 65 * 1024 - 200, 77_000, 64, 8, {"RAGRAPH_FILTER_I8": "0"}, "tight_many"),
    ("int8 eight groups D=64, tiles of 1024, 1 left", 65 * 1024 - 200, 154_000, 64, 8, {}, "tight_few"),
]


@pytest.mark.parametrize("what,B,N,D,k,env,call", CASES, ids=[c[0] for c in CASES])
def test_split_plan_rows_have_the_bits_of_the_fp32_kernel(dev, monkeypatch, what, B, N, D, k, env, call):
    from ragraph_amd import kernels as K

    g = torch.Generator(device=dev).manual_seed(B + N + D)
    kn = K.normalize_rows(torch.randn(N, D, device=dev, generator=g))
    q = torch.randn(B, D, device=dev, generator=g)
    kb = K.keys_to_bf16(kn)
    s32, i32 = K.topk_cosine(q, kn, k)
    srt = torch.sort(s32[:, k - 1]).values
    prior = tight = None
    if call != "plain":
        prior = float(srt[0]) - 0.01
    if call == "tight_many":
        tight = float(srt[B // 2])
    elif call == "tight_few":
        tight = float(srt[100])
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    K.set_filter_prior(prior)
    K.set_filter_tight_prior(tight)
    try:
        s, i, over, st = K.topk_cosine_filtered(q, kn, kb, k, return_stats=True)
        w = st.cpu().tolist()
    finally:
        K.set_filter_prior(None)
        K.set_filter_tight_prior(None)
    assert torch.equal(i, i32) and torch.equal(s, s32), what
    assert int(over) == 0 and w[0] == K.FILTER_STATS_MAGIC and w[14] == B and w[15] == 0, (what, w[14:24])
    assert w[16] == (0 if call == "plain" else 1) and w[17] == 0, (what, w[14:24])
    if tight is not None:
        soft = int((s32[:, k - 1] < tight).sum())
        assert w[21] == 1 and w[22] == soft and w[23] == (2 if soft > 256 else 1), (what, soft, w[14:24])
        assert (soft > 256) == (call == "tight_many")


def test_zero_query_count_of_repeated_calls(dev):
    """filter_prep_kernel's workgroups count zero queries into word [15] in any order with the workgroup that labels the words:
    the word is zeroed on the stream in front of the launch.  4096 queries, every 64th a zero query, 20 calls."""
    from ragraph_amd import kernels as K

    g = torch.Generator(device=dev).manual_seed(15)
    kn = K.normalize_rows(torch.randn(20_000, 256, device=dev, generator=g))
    kb = K.keys_to_bf16(kn)
    q = torch.randn(4096, 256, device=dev, generator=g)
    q[::64] = 0.0
    seen = []
    for _ in range(20):
        _, _, _, st = K.topk_cosine_filtered(q, kn, kb, 10, return_stats=True)
        seen.append(int(st[15]))
    assert seen == [64] * 20, seen
