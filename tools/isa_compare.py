"""Compare the gfx950 instructions of every kernel of two source trees (a refactor's proof that it changed no kernel):
  python tools/isa_compare.py OLD_TREE NEW_TREE [-j JOBS] > report.txt

For each tree every ragraph_amd/csrc/*.hip is compiled with the command its own Makefile would run (`make -n -B x.o`), turned
into a device-only assembly listing (--cuda-device-only -S).  No GPU is needed.  Comment, .file, .ident and .loc lines are
dropped and the function ordinal in block labels (.LBB<n>_) is blanked, since it only counts the functions in front of the
kernel.  Every kernel, by name, is then one of
  identical   the instruction text is the same;
  reordered   the opcode histogram is the same, and so are VGPRs, AGPRs, SGPRs, scratch and LDS (the .amdgpu_metadata block, as
              tools/kernel_regs.py reads it);
  changed     anything else (a kernel that only one tree has is `changed` too).
One line per kernel, then a summary.  Exit status 1 when a kernel is `changed`."""
import argparse
import collections
import concurrent.futures
import glob
import os
import re
import shlex
import subprocess
import sys
import tempfile

FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def assemble(csrc, src, out):
    """The Makefile's compile command for `src`, as a device-only assembly listing written to `out`."""
    obj = os.path.splitext(src)[0] + ".o"
    plan = subprocess.run(["make", "-C", csrc, "-n", "-B", "--no-print-directory", obj], capture_output=True, text=True, check=True)
    cmd = shlex.split([ln for ln in plan.stdout.splitlines() if src in ln][-1])
    keep, skip = [], False
    for a in cmd:
        if skip:
            skip = False
        elif a == "-o":
            skip = True
        elif a not in ("-c", "-MMD", "-MP"):
            keep.append(a)
    subprocess.run(keep + ["--cuda-device-only", "-S", "-o", out + ".part"], cwd=csrc, check=True, stderr=subprocess.DEVNULL)
    os.replace(out + ".part", out)


def kernels_of(path):
    """{kernel name: (instruction lines, opcode histogram, resource figures)} of one assembly file."""
    txt = open(path).read()
    meta = txt[txt.index("amdhsa.kernels:"):]
    figures = {}
    for blk in meta.split("  - .agpr_count:")[1:]:
        f = dict(re.findall(r"\.(\w+):\s+(\S+)", "  - .agpr_count:" + blk))
        figures[f["name"]] = tuple(f.get(w) for w in FIGURES)
    lines = txt[:txt.index("amdhsa.kernels:")].splitlines()
    labels = {ln.split(":")[0]: n for n, ln in enumerate(lines) if ln[:1] not in ("", "\t", " ", ".", ";") and ":" in ln}
    out = {}
    for name in figures:
        start = labels[name]
        body, ops = [], collections.Counter()
        for ln in lines[start + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            ln = ln.split(";")[0].strip()
            if not ln or re.match(r"\.(file|ident|loc)\b", ln):
                continue
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            body.append(ln)
            if not ln.endswith(":") and not ln.startswith("."):
                ops[ln.split()[0]] += 1
        out[name] = (body, ops, figures[name])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--work", help="keep the assembly listings in this directory, and reuse those it already holds")
    args = ap.parse_args()
    trees = [os.path.join(os.path.abspath(t), "ragraph_amd", "csrc") for t in (args.old, args.new)]
    srcs = [sorted(os.path.basename(p) for p in glob.glob(os.path.join(c, "*.hip"))) for c in trees]
    with tempfile.TemporaryDirectory() as tmp:
        if args.work:
            os.makedirs(args.work, exist_ok=True)
            tmp = os.path.abspath(args.work)
        jobs = [(c, s, os.path.join(tmp, f"{side}_{s}.s")) for side, (c, ss) in enumerate(zip(trees, srcs)) for s in ss]
        jobs = [j for j in jobs if not os.path.exists(j[2])]
        with concurrent.futures.ThreadPoolExecutor(args.j) as pool:
            list(pool.map(lambda j: assemble(*j), jobs))
        sides = [{s: kernels_of(os.path.join(tmp, f"{side}_{s}.s")) for s in ss} for side, ss in enumerate(srcs)]
    count = collections.Counter()
    for src in sorted(set(srcs[0]) | set(srcs[1])):
        old, new = sides[0].get(src, {}), sides[1].get(src, {})
        for name in sorted(set(old) | set(new)):
            if name not in old or name not in new:
                cls, note = "changed", "only in the %s tree" % ("old" if name in old else "new")
            elif old[name][0] == new[name][0]:
                cls, note = "identical", ""
            elif old[name][1] == new[name][1] and old[name][2] == new[name][2]:
                cls, note = "reordered", ""
            else:
                d = sum(new[name][1].values()) - sum(old[name][1].values())
                cls, note = "changed", f"instructions {d:+d}, figures {old[name][2]} -> {new[name][2]}"
            count[cls] += 1
            ins = sum(new[name][1].values()) if name in new else 0
            print(f"{cls:9s} {src:24s} {ins:6d} ins  {name}  {note}".rstrip())
    print(f"summary: {sum(count.values())} kernels of {len(srcs[1])} files: {count['identical']} identical, "
          f"{count['reordered']} reordered, {count['changed']} changed")
    return 1 if count["changed"] else 0


if __name__ == "__main__":
    sys.exit(main())
