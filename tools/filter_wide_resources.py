#!/usr/bin/env python3
"""Compare two `-Rpass-analysis=kernel-resource-usage` build logs of csrc/topk_filter.hip and csrc/topk_filter_direct.hip:
the parent's and this tree's.  The list-carrying kernels gained a trailing template argument LW (32: the code as it was,
64: the wide entry's); an LW = 32 instantiation is matched with the parent's kernel of the same leading arguments.

    make -C ragraph_amd/csrc CXXFLAGS="<the Makefile's> -Rpass-analysis=kernel-resource-usage" topk_filter.o topk_filter_direct.o 2> new.log
    (the same in a checkout of the parent commit: parent.log)
    python tools/filter_wide_resources.py parent.log new.log > profiles/filter_wide_resources.txt

Exit status 1 if an existing instantiation differs or a new one uses scratch."""
import re
import subprocess
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]"]
WIDENED = ("topk_rescore_wide_kernel", "topk_rescore_scored_kernel", "topk_overflow_fixup_kernel")


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = m.group(2)
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"^void ragraph::|\(.*$", "", d): out[n] for n, d in zip(names, dem)}


def main():
    parent, new = parse(sys.argv[1]), parse(sys.argv[2])
    bad = 0
    rows = []
    for name, res in sorted(new.items()):
        m = re.match(r"(\w+)<(.*)>$", name)
        key, width = name, None
        if m and m.group(1) in WIDENED:
            args = m.group(2).split(", ")
            width = int(args[-1])
            key = f"{m.group(1)}<{', '.join(args[:-1])}>"
        vals = " ".join(f"{res.get(f, '?'):>6}" for f in FIELDS)
        if width == 64:
            ok = res.get("ScratchSize [bytes/lane]") == "0"
            rows.append(f"NEW   {vals}  {name}" + ("" if ok else "   <-- SCRATCH"))
            bad += not ok
        elif key in parent:
            same = parent[key] == res
            rows.append(f"{'same ' if same else 'DIFF '} {vals}  {name}" +
                        ("" if same else "   <-- parent: " + " ".join(parent[key].get(f, "?") for f in FIELDS)))
            bad += not same
        else:
            rows.append(f"ADDED {vals}  {name}")
    gone = [k for k in parent if k not in new and not any(
        k == re.sub(r", 32>$", ">", n) for n in new)]
    print("# kernel resources, parent against this tree (gfx950, -O3): SGPRs VGPRs AGPRs scratch[B/lane] static-LDS[B]")
    print(f"# {len(parent)} kernels in the parent, {len(new)} here; 'same': identical in every column; NEW: an LW = 64 instantiation")
    print("\n".join(rows))
    for k in gone:
        print(f"GONE  {k}")
        bad += 1
    print(f"# {'all existing instantiations identical, no scratch in the new ones' if not bad else str(bad) + ' PROBLEMS'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
