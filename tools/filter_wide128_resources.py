#!/usr/bin/env python3
"""Compare two `-Rpass-analysis=kernel-resource-usage` build logs of csrc/topk_filter.hip and csrc/topk_filter_direct.hip:
the parent's and this tree's.  The list-carrying kernels carry the list width as their last template argument -- LW = 32 / 64 /
128 for the workgroup-per-query rescoring, the scored rescoring and the fixup scan, 64 (every k <= 64: the code as it was) / 128
for the one-wave-per-query rescoring and the repair scatter, which had no such argument in the parent; the bound selection
gained its part maxima per lane (2: the code as it was, 4: up to 256 parts for lists of 65 .. 128 keys).  Every instantiation for
LW <= 64 is matched with the parent's kernel and must report the same registers, LDS and scratch; an LW = 128 one must not use
scratch.

    make -C ragraph_amd/csrc CXXFLAGS="<the Makefile's> -Rpass-analysis=kernel-resource-usage" topk_filter.o topk_filter_direct.o 2> new.log
    (the same in a checkout of the parent commit: parent.log)
    python tools/filter_wide128_resources.py parent.log new.log > profiles/filter_wide128_resources.txt

Exit status 1 if an existing instantiation differs, one is gone, or a new one uses scratch."""
import re
import sys

from filter_wide_resources import FIELDS, parse

WIDENED = ("topk_rescore_wide_kernel", "topk_rescore_scored_kernel", "topk_overflow_fixup_kernel")   # parent: <..., LW> or <...> = 32
# parent: no such argument; the value of it that is new here (the other value is the code as it was)
GAINED = {"topk_rescore_coop_kernel": 128, "filter_repair_scatter_kernel": 128, "filter_bound_scores_kernel": 4}


def parent_name(name):
    """(the parent's name of this instantiation or None if it is new, its list width or None)"""
    m = re.match(r"(?:ragraph::)?(\w+)<(.*)>$", name)
    if not m or m.group(1) not in WIDENED + tuple(GAINED):
        return name, None
    base, args = m.group(1), m.group(2).split(", ")
    width = int(args[-1])
    if width == (GAINED[base] if base in GAINED else 128):
        return None, width
    if base in GAINED:
        rest = args[:-1]
        return (f"{base}<{', '.join(rest)}>" if rest else f"ragraph::{base}"), width
    return name, width


def main():
    parent, new = parse(sys.argv[1]), parse(sys.argv[2])
    bad, rows, seen = 0, [], set()
    for name, res in sorted(new.items()):
        pname, width = parent_name(name)
        vals = " ".join(f"{res.get(f, '?'):>6}" for f in FIELDS)
        if pname is None:
            ok = res.get("ScratchSize [bytes/lane]") == "0"
            rows.append(f"NEW   {vals}  {name}" + ("" if ok else "   <-- SCRATCH"))
            bad += not ok
            continue
        if pname not in parent and width == 32:     # (the parent spelt LW = 32 by its default in some launches)
            pname = re.sub(r", 32>$", ">", pname)
        if pname in parent:
            seen.add(pname)
            same = parent[pname] == res
            pvals = " ".join(f"{parent[pname].get(f, '?'):>6}" for f in FIELDS)
            rows.append(f"{'same ' if same else 'DIFF '} {vals}  {name}\n parent{pvals}  {pname}" if width is not None else
                        f"{'same ' if same else 'DIFF '} {vals}  {name}" + ("" if same else f"   <-- parent: {pvals}"))
            bad += not same
        else:
            rows.append(f"ADDED {vals}  {name}")
    gone = [k for k in parent if k not in seen]
    print("# kernel resources, parent against this tree (gfx950, -O3): SGPRs VGPRs AGPRs scratch[B/lane] static-LDS[B]")
    print(f"# {len(parent)} kernels in the parent, {len(new)} here; 'same': identical in every column (a list-carrying kernel for LW <= 64")
    print("# has the parent's line under its own); NEW: an LW = 128 instantiation (filter_bound_scores_kernel<4>: 256 parts)")
    print("\n".join(rows))
    for k in gone:
        print(f"GONE  {k}")
        bad += 1
    print(f"# {'all existing instantiations identical, no scratch in the new ones' if not bad else str(bad) + ' PROBLEMS'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
