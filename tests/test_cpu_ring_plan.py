"""The ring kernel's work plan (segment_plan.h: RingWalker, ring_plan_choose) is plain C++ shared by the kernel, the launch
and this checker: build tools/check_ring_plan.cpp with g++ and run it."""
import os
import re
import subprocess


def _build(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "check_ring_plan")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(root, "ragraph_amd", "csrc"),
                           os.path.join(root, "tools", "check_ring_plan.cpp"), "-o", exe])
    return exe


def test_ring_plan_covers_every_stage_once_and_never_loads_more_than_the_parent(tmp_path):
    """qtiles 64 .. 200 (every residue mod 8) x NS {1, 3, 8, 63, 489, 7813} x CUS {64, 128, 256} x lb_min {1, 8}: every
    (tile, stage) exactly once, no empty segment, every walk ends, the chosen plan's most loaded workgroup never above the
    XCD-groups-only plan's; at 131 x 7813 x 256 within lb_min + 1 stages of 131 * 7813 / 256 = 3998 (parent: 4151)."""
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:]
    m = re.search(r"ring plans checked: (\d+) \(split taken in (\d+) of (\d+)", out.stdout)
    assert m and int(m.group(1)) == 137 * 6 * 3 * 2 and int(m.group(2)) > 0
    m = re.search(r"bench shape 131 x 7813 x 256: mode (\d), most loaded workgroup (\d+) stages \(parent (\d+), even (\d+)\)", out.stdout)
    assert m, out.stdout[-2000:]
    mode, got, parent, even = (int(x) for x in m.groups())
    assert even == 3998 and parent == 4151
    assert mode == 2 and got <= even + 8 + 1


def test_the_gpu_parity_shapes_take_the_split_plan(tmp_path):
    """(tiles, stages) of the launches tests/test_gpu_ring_split_plan.py is about, on 256 workgroups with launch_ring's lb_min:
    all take the two-part plan; at 65 x 301 the leftover tile's pieces fall to lb_min and most workgroups get none of it.
    Below ~256 stages (and at 71 x 301) the XCD groups alone are as good and are kept."""
    exe = _build(tmp_path)
    shapes = [(65, 301), (67, 301), (71, 474), (71, 602), (65, 188), (67, 256), (71, 301)]
    out = subprocess.run([exe] + [str(v) for t, ns in shapes for v in (t, ns, 256)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:]
    got = {(int(m.group(1)), int(m.group(2))): (int(m.group(3)), int(m.group(4)), int(m.group(5)))
           for m in re.finditer(r"plan (\d+) x (\d+) x 256: mode (\d) lb_min (\d+) load \d+ idle (\d+)", out.stdout)}
    assert len(got) == len(shapes), out.stdout
    for key in shapes[:4]:
        assert got[key][0] == 2 and got[key][1] == 8, (key, got[key])
    for key in shapes[4:]:
        assert got[key][0] == 1, (key, got[key])
    assert got[(65, 301)][2] > 128
