"""The statistics words of a filtered top-k call, by name: the host-side mirror of the layout comment in csrc/filter_prepare.h
(N_WORDS ints at ragraph_topk_cosine_filtered_stats_offset of the call's workspace).  Plain Python: neither torch nor the library."""
import struct

N_WORDS = 32
MAGIC_VALUE = 0x52414753
MAX_LEVELS = 3     # levels the per-level words (+ l) describe
LEVEL_WORDS = 16   # levels() reads the words [0, LEVEL_WORDS) only
MAGIC = 0          # MAGIC_VALUE once the prepare launch has labelled the words
LEVELS = 1         # levels of the call
CAND = 2           # + l: sum of the candidate counts of every 64th query at level l
SAMPLED = 5        # + l: how many queries were sampled at level l
IS_I8 = 8          # + l: level l ran on the int8 copy
KEYS = 11          # + l: keys of level l
QUERIES = 14       # queries of the call
ZERO_QUERIES = 15  # all-zero queries among them
SPECULATIVE = 16   # 1: the call filtered under a speculative first bound
SPEC_FAILED = 17   # queries whose speculation failed (answered by the exact scan)
KTH_LO = 18        # smallest final exact k-th best score of the call's queries, as an order-preserving int (ord2f)
KTH_HI = 19        # largest
OVERFLOW = 20      # the call's final overflow count
TIGHT = 21         # a tight bound was in force
SOFT_MISSES = 22   # queries the tight bound was too high for
REPAIR = 23        # the repair that ran (1: the 256-query call, 2: the all-queries level)
TAIL_DELTA = 24    # a tight call's step delta = (t - prior) / 16 as float bits (bits2f); 0: the tail counts are not reported
TAIL_BELOW = 25    # + j, j < len(TAIL_STEPS): judged queries whose final k-th best is below t + TAIL_STEPS[j] * delta
TAIL_STEPS = (1, 2, 4, 8)   # [29, 32) reserved


def ord2f(v: int) -> float:
    """The float behind an order-preserving int (csrc/topk_order.h f2ord: negative floats have their 31 low bits flipped)."""
    v = int(v)
    return struct.unpack("<f", struct.pack("<i", v ^ 0x7FFFFFFF if v < 0 else v))[0]


def bits2f(v: int) -> float:
    """The float whose bits an int word holds (TAIL_DELTA)."""
    return struct.unpack("<f", struct.pack("<i", int(v)))[0]


def tail_points(words, t: float):
    """[(score, queries whose final k-th best is below it)] of a call that ran under the tight bound t: t itself (SOFT_MISSES)
    and the TAIL_STEPS edges, formed as the device forms them; None when the call did not report them."""
    if len(words) < TAIL_BELOW + len(TAIL_STEPS) or not words[TIGHT] or not words[TAIL_DELTA]:
        return None
    delta = bits2f(words[TAIL_DELTA])
    if not delta > 0.0:
        return None
    return [(float(t), int(words[SOFT_MISSES]))] + [(float(t) + m * delta, int(words[TAIL_BELOW + j])) for j, m in enumerate(TAIL_STEPS)]


def levels(words) -> list:
    """[(dtype, keys, candidates per query or None)] per level from a HOST copy of a call's statistics words."""
    st = [int(x) for x in words]
    if len(st) < LEVEL_WORDS or st[MAGIC] != MAGIC_VALUE:
        return []
    return [("int8" if st[IS_I8 + l] else "bf16", st[KEYS + l], st[CAND + l] / st[SAMPLED + l] if st[SAMPLED + l] else None)
            for l in range(min(st[LEVELS], MAX_LEVELS))]


def candidates_per_query(words):
    """Sampled candidates per query summed over the call's levels; None when no level sampled a query."""
    if not any(words[SAMPLED:SAMPLED + MAX_LEVELS]):
        return None
    return sum(words[CAND + l] / words[SAMPLED + l] for l in range(min(words[LEVELS], MAX_LEVELS)) if words[SAMPLED + l])
