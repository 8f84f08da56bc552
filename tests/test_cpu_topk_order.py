"""The canonical top-k order's keys (csrc/topk_order.h) are plain C++ shared by every top-k kernel and this checker: build
tools/check_topk_order.cpp with g++ and run it -- every non-NaN float through both key maps, the pair key against cand_better --
and decode the words it prints with the Python decoder of the statistics words (ragraph_amd/filter_stats.py)."""
import os
import re
import struct
import subprocess

from ragraph_amd import filter_stats as FS
from ragraph_amd import kernels as K


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _f2ord(x):
    """(tests/test_cpu_key_index_routes.py builds the statistics words with this one)"""
    b = struct.unpack("<i", struct.pack("<f", x))[0]
    return b if b >= 0 else b ^ 0x7FFFFFFF


def test_every_float_through_the_key_maps_and_the_header_words_through_the_python_decoder(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "check_topk_order")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(root, "ragraph_amd", "csrc"),
                           os.path.join(root, "tools", "check_topk_order.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:]
    assert "all checks held" in out.stdout
    m = re.search(r"floats walked: (\d+)", out.stdout)
    assert m and int(m.group(1)) == 2 ** 32 - 2 * (2 ** 23 - 1)     # every bit pattern but the NaNs
    m = re.search(r"pairs checked: (\d+) x (\d+)", out.stdout)
    assert m and int(m.group(1)) == int(m.group(2)) == 10 * 3 + 1
    words = {int(b, 16): int(w) for b, w in re.findall(r"^f2ord ([0-9a-f]{8}) (-?\d+)$", out.stdout, re.M)}
    assert len(words) == 10
    for bits, w in words.items():                                   # the header's word, decoded in Python, is the float's bits
        x = struct.unpack("<f", struct.pack("<I", bits))[0]
        assert _bits(FS.ord2f(w)) == bits and _bits(K.ord2f(w)) == bits, hex(bits)
        assert w == _f2ord(x), hex(bits)
    # (the order tests/test_cpu_key_index_routes.py expects of the words, here on the header's own)
    assert _bits(1e-45) == 1
    assert words[_bits(-1.0)] < words[_bits(-0.0)] < words[_bits(0.0)] < words[_bits(1e-45)] < words[_bits(1.0)]
    assert words[_bits(float("-inf"))] == min(words.values()) and words[_bits(float("inf"))] == max(words.values())
