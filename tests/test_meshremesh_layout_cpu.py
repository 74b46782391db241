"""The one block a remeshing handle carves its arrays from (csrc/meshremesh_layout.h), on the host: tools/meshremesh_layout_check.cpp
is a stand-alone program (its own main) that carves a host block with the handle's own code and does the memset a round does.  Here
it is built plain and with ASan + UBSan and run as a child, and its rows are compared with the arithmetic written out again in
Python from the list of arrays in the header.  No GPU; nothing loaded into Python runs under a sanitizer."""
import os
import re
import subprocess

import pytest

from surfd_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surfd_amd", "csrc")
SIZES = {"int": 4, "unsigned": 4, "int32_t": 4, "rm_u64": 8, "double": 8}
ZEROED = ["vborder", "vheavy", "vfirst", "vlast", "lfirst", "llast", "hfirst", "hlast"]


def listed():
    """[(type, name, length expression)] of RM_ARRAYS, in its order"""
    text = open(os.path.join(CSRC, "meshremesh_layout.h")).read()
    body = text[text.index("#define RM_ARRAYS(DO, V, F, H)"):text.index("struct rm_arrays")]
    return re.findall(r"DO\((\w+), (\w+), (RM_WORDS|V|F|H|3 \* \(V\)|\(H\) \+ 1)\)", body)


def slot(n, size):
    return (max(n, 1) * size + 255) & ~255


def build_check(tmp_path, *flags):
    exe = str(tmp_path / ("meshremesh_layout_check" + ("_san" if flags else "")))
    src = os.path.join(ROOT, "tools", "meshremesh_layout_check.cpp")
    r = subprocess.run([B._hipcc(), "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only", *flags, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def check_output(exe, V, F):
    r = subprocess.run([exe, str(V), str(F)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    rows = [line.split() for line in r.stdout.splitlines()]
    arrays = listed()
    assert len(arrays) == 43 and [row[0] for row in rows[:-2]] == [name for _, name, _ in arrays]
    offset = 0
    for (kind, name, expr), (_, elem, n, at) in zip(arrays, rows[:-2]):
        want_n = eval(expr, {"V": V, "F": F, "H": 3 * F, "RM_WORDS": 32})
        assert (int(elem), int(n), int(at)) == (SIZES[kind], want_n, offset), (name, elem, n, at, offset)
        offset += slot(want_n, SIZES[kind])
    assert rows[-2] == ["total", str(offset)]
    assert rows[-1] == ["zeroed", "vborder", "hlast", str(8 * slot(V, 4))]
    names = [name for _, name, _ in arrays]
    first = names.index("vborder")
    assert names[first:first + 8] == ZEROED and all(expr == "V" and kind == "int" for kind, _, expr in arrays[first:first + 8])


def test_the_handle_uses_the_checked_layout():
    hip = open(os.path.join(CSRC, "meshremesh.hip")).read()
    assert '#include "meshremesh_layout.h"' in hip and "struct rm_arrays" not in hip and "arena.get(" not in hip
    assert hip.count("rm_carve(") == 1 and hip.count("rm_block_bytes(") == 1 and "rm_round_zero_bytes(m->Vcap)" in hip
    assert "dev_slot<int>(m->Vcap)" not in hip                 # the length of the round's memset is the header's
    layout = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "meshremesh_layout.h")).read())
    assert "hip" not in layout.lower()                          # plain C++: no HIP call in the carving arithmetic


def test_the_block_is_carved_exactly(tmp_path):
    exe = build_check(tmp_path)
    for V in (0, 1, 63, 257):
        for F in (0, 1, 85, 257):
            check_output(exe, V, F)
    check_output(exe, 35_002, 70_000)


def test_the_block_under_host_sanitizers(tmp_path):
    """every array is written from its first to its last element inside a block of exactly the size the handle allocates, then the
    round's memset runs: built with ASan + UBSan, a byte outside the block is a report and a failure"""
    exe = build_check(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for V, F in ((0, 0), (1, 1), (257, 257), (257, 1), (1, 257), (5_000, 9_000)):
        check_output(exe, V, F)
