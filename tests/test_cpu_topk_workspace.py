"""Workspace sizes of the exact top-k entry points (csrc/topk_cosine.hip), on the host: no GPU.

The byte counts below were RECORDED FROM THE PARENT COMMIT'S LIBRARY, before the three size queries and the three calls
were put on one slab layout and one fused layout.  They pin that layout: a size query that drifts from the call's carve-up
is an out-of-bounds device write that no host check sees.  A deliberate change of a layout must re-record them.
(Without a device the CU count the fused plan reads is 256, an MI355X's own.)"""
import pytest

SIZE_QUERY = {"cosine": "ragraph_topk_cosine_workspace_bytes",          # (B, N, D, k)
              "mix": "ragraph_topk_cosine_mix_workspace_bytes",         # (B, N, D, A, k)
              "masked": "ragraph_topk_dot_masked_workspace_bytes"}      # (B, N, D, k, nnz)

# (flavour, arguments, RAGRAPH_TOPK_SLAB, bytes),  # what the shape reaches.  G = key chunks of the slab paths.
RECORDED = [
    ('cosine', (1, 1000000, 256, 10), None, 21504),  # streaming kernel
    ('cosine', (16, 1000000, 128, 28), None, 531456),  # streaming kernel
    ('cosine', (128, 131073, 64, 28), None, 1867776),  # streaming kernel, largest batch and k at D = 64
    ('cosine', (4, 33333, 256, 31), None, 134144),  # streaming kernel, largest k at D = 256
    ('cosine', (128, 1000000, 256, 32), None, 4325376),  # tile kernel: k = 32 lists do not fit the streaming kernel
    ('cosine', (129, 9000000, 64, 1), None, 297216),  # tile kernel
    ('cosine', (700, 1000000, 256, 10), None, 5476864),  # tile kernel
    ('cosine', (4096, 1000000, 256, 10), None, 9437184),  # tile kernel
    ('cosine', (100000, 131073, 128, 32), None, 256000000),  # tile kernel, XCD mapping
    ('cosine', (16, 1000, 256, 10), None, 80384),  # slabs by rule (tiny bank)
    ('cosine', (16, 1000, 256, 10), '0', 21504),  # the same shape on the streaming kernel
    ('cosine', (128, 8192, 256, 10), None, 4325376),  # slabs by rule
    ('cosine', (700, 33333, 128, 10), None, 5118464),  # slabs by rule
    ('cosine', (700, 33333, 128, 10), '0', 5118464),  # the same shape on the tile kernel
    ('cosine', (4096, 8193, 64, 31), None, 135282688),  # slabs by rule (D = 64 limit)
    ('cosine', (3, 10, 8, 1), None, 512),  # slabs by width
    ('cosine', (17, 33333, 96, 10), None, 2273536),  # slabs by width
    ('cosine', (700, 1000000, 8, 32), None, 1072022528),  # slabs by width, several query slabs
    ('cosine', (129, 131072, 256, 33), None, 67765248),  # slabs by k
    ('cosine', (4096, 1000000, 128, 64), None, 1074097152),  # slabs by k
    ('cosine', (16, 4194304, 96, 28), None, 268441600),  # lists: one chunk of exactly 2^22 keys
    ('cosine', (128, 4194305, 96, 10), None, 536935680),  # lists: G = 2
    ('cosine', (700, 4194305, 256, 64), None, 537686272),  # lists: G = 2 by k
    ('cosine', (17, 9000000, 8, 33), None, 204021248),  # lists: G = 3
    ('cosine', (700, 33333, 256, 65), None, 94049280),  # large k: G = 1
    ('cosine', (1, 1000, 64, 200), None, 4352),  # large k: G = 1, one query
    ('cosine', (4096, 131072, 128, 4096), None, 1210056704),  # large k: G = 1, largest k
    ('cosine', (17, 4194240, 8, 200), None, 292172288),  # large k: one chunk of exactly 65535 x 64 keys
    ('cosine', (17, 4194241, 8, 65), None, 143754496),  # large k: G = 2
    ('cosine', (3, 4194305, 256, 4096), None, 28904704),  # large k: G = 2, largest k
    ('cosine', (129, 9000000, 96, 200), None, 787198464),  # large k: G = 3
    ('mix', (16, 1000000, 256, 10, 10), None, 344832),  # streaming kernel
    ('mix', (4096, 1000000, 256, 16, 10), None, 9699328),  # tile kernel
    ('mix', (700, 131073, 64, 1, 32), None, 15414016),  # tile kernel
    ('mix', (128, 8192, 128, 16, 10), None, 8462336),  # slabs by rule
    ('mix', (128, 8192, 128, 16, 10), '0', 237568),  # the same shape on the streaming kernel
    ('mix', (17, 33333, 96, 16, 10), None, 4541696),  # slabs by width
    ('mix', (700, 1000000, 256, 1, 33), None, 1072719616),  # slabs by k, several query slabs
    ('mix', (16, 4194240, 8, 16, 10), None, 536864256),  # lists: one chunk of exactly 65535 x 64 keys
    ('mix', (129, 4194241, 8, 16, 31), None, 1073786368),  # lists: G = 2
    ('mix', (4, 9000000, 96, 1, 64), None, 96011008),  # lists: G = 3
    ('mix', (700, 33333, 256, 16, 200), None, 187426560),  # large k: G = 1
    ('mix', (17, 4194305, 64, 1, 65), None, 286376192),  # large k: G = 2
    ('mix', (100000, 9000000, 128, 16, 4096), None, 1702651904),  # large k: G = 3
    ('masked', (16, 1000000, 256, 10, 10), None, 8350208),  # streaming kernel
    ('masked', (700, 1000000, 64, 28, 0), None, 21508096),  # tile kernel, empty history
    ('masked', (4096, 131073, 128, 10, 200000), None, 26091264),  # tile kernel
    ('masked', (128, 8192, 256, 10, 10), None, 4397056),  # slabs by rule
    ('masked', (128, 8192, 256, 10, 10), '0', 530432),  # the same shape on the streaming kernel
    ('masked', (17, 33333, 96, 10, 200000), None, 20242688),  # slabs by width
    ('masked', (129, 131072, 256, 33, 0), None, 68814336),  # slabs by k
    ('masked', (100000, 10, 8, 1, 10), None, 8006144),  # more queries than keys (the sort runs over B)
    ('masked', (16, 4194304, 8, 10, 10), None, 301996544),  # lists: one chunk of exactly 2^22 keys
    ('masked', (3, 4194305, 8, 10, 10), None, 58727680),  # lists: G = 2
    ('masked', (700, 4194305, 128, 64, 200000), None, 588584960),  # lists: G = 2 by k
    ('masked', (16, 9000000, 96, 31, 0), None, 264024832),  # lists: G = 3
    ('masked', (700, 33333, 256, 65, 10), None, 94321920),  # k > 64 (the call refuses it): the size query keeps the list layout
    ('masked', (17, 9000000, 8, 200, 0), None, 276123904),  # k > 64, G = 3: the list layout
]


@pytest.mark.parametrize("flavour,args,slab_env,expected", RECORDED)
def test_workspace_bytes_equal_the_recorded_layout(monkeypatch, flavour, args, slab_env, expected):
    from ragraph_amd import _native as N

    if slab_env is None:
        monkeypatch.delenv("RAGRAPH_TOPK_SLAB", raising=False)
    else:
        monkeypatch.setenv("RAGRAPH_TOPK_SLAB", slab_env)      # (read per call)
    assert getattr(N.lib(), SIZE_QUERY[flavour])(*args) == expected


def test_size_queries_return_zero_for_arguments_the_calls_refuse():
    from ragraph_amd import _native as N

    L = N.lib()
    assert L.ragraph_topk_cosine_workspace_bytes(16, 100000, 256, 4097) == 0          # k > RAGRAPH_TOPK_ORDERED_MAX
    assert L.ragraph_topk_cosine_mix_workspace_bytes(16, 100000, 256, 10, 4097) == 0
    assert L.ragraph_topk_cosine_mix_workspace_bytes(16, 100000, 256, 17, 10) == 0    # A > 16
    assert L.ragraph_topk_cosine_mix_workspace_bytes(16, 100000, 256, 0, 10) == 0
    assert L.ragraph_topk_dot_masked_workspace_bytes(16, 100000, 256, 10, -1) == 0    # nnz < 0
    for fn, a in (("cosine", (0, 10, 8, 1)), ("mix", (1, 0, 8, 1, 1)), ("masked", (1, 10, 0, 1, 0))):
        assert getattr(L, SIZE_QUERY[fn])(*a) == 0
