"""The host scaffold the mesh handles share (csrc/meshscene.h), without a GPU: split_units() against the four functions it
replaced (rc_splits, md_splits, mi_splits, wn_splits), restated here as they stood in raycast.hip, meshdist.hip,
meshintersect.hip and winding.hip.  The header is host C++, so a stand-alone program (tools/meshscene_split_check.cpp) prints
the function's table and this file compares it pair by pair."""
import os
import re
import subprocess

import pytest

from surfd_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surfd_amd", "csrc")
ITEMS = (1, 63, 64, 255, 256, 257, 4096, 2 ** 20, 2 ** 28)
UNITS = (1, 2, 3, 31, 64, 1000, 65535, 174763)


def ceil_div(a: int, b: int) -> int:
    return (a + b - 1) // b


def old_chunk_splits(items: int, nchunk: int, chunk: int, max_splits: int):
    """rc_splits, md_splits and mi_splits: the same text with RC_, MD_ and MI_ constants"""
    blocks = ceil_div(items, chunk)
    s = max(1, ceil_div(2048, blocks))
    s = min(s, max_splits, nchunk)
    span = ceil_div(nchunk, s)
    return ceil_div(nchunk, span), span


def old_wn_splits(Q: int, ngroup: int, one: bool, chunk: int):
    qb = ceil_div(Q, chunk)
    s = 1 if one else max(1, ceil_div(2048, qb))
    s = min(s, ngroup, 65535)
    gspan = ceil_div(ngroup, s)
    return ceil_div(ngroup, gspan), gspan


def constant(source: str, name: str) -> int:
    """`constexpr int NAME = a [* b];` of a kernel file, names resolved in the same file"""
    text = open(os.path.join(CSRC, source)).read()
    m = re.search(rf"constexpr int {name} = ([^;]+);", text)
    assert m, (source, name)
    value = 1
    for factor in m.group(1).split("*"):
        factor = factor.strip()
        value *= int(factor) if factor.isdigit() else constant(source, factor)
    return value


@pytest.fixture(scope="module")
def split_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("meshscene") / "meshscene_split_check")
    src = os.path.join(ROOT, "tools", "meshscene_split_check.cpp")
    assert '#include "../surfd_amd/csrc/meshscene.h"' in open(src).read()
    r = subprocess.run([B._hipcc(), "-std=c++17", "-O1", "-x", "hip", "--cuda-host-only", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def table(block: int, max_splits: int, target: int) -> dict:
        r = subprocess.run([exe, str(block), str(max_splits), str(target)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
        return {(i, u): (S, span) for i, u, S, span in rows}

    return table


@pytest.mark.parametrize("source,prefix", [("raycast.hip", "RC"), ("meshdist.hip", "MD"), ("meshintersect.hip", "MI")])
def test_split_units_equals_the_chunk_splits_it_replaced(split_check, source, prefix):
    chunk, cap = constant(source, f"{prefix}_CHUNK"), constant(source, f"{prefix}_MAX_SPLITS")
    assert (chunk, cap) == (256, 64)
    assert re.search(rf"split_units\([^;]*, {prefix}_CHUNK, [^;]*, {prefix}_MAX_SPLITS\);", open(os.path.join(CSRC, source)).read())
    got = split_check(chunk, cap, 2048)
    assert set(got) == {(i, u) for i in ITEMS for u in UNITS}
    for (i, u), pair in got.items():
        assert pair == old_chunk_splits(i, u, chunk, cap), (source, i, u)


@pytest.mark.parametrize("one", [False, True])
def test_split_units_equals_the_winding_splits_it_replaced(split_check, one):
    chunk = constant("winding.hip", "WN_CHUNK")
    assert chunk == 256
    text = open(os.path.join(CSRC, "winding.hip")).read()
    assert "split_units(Qs, WN_CHUNK, m->ngroup, 65535, (flags & SURFD_WINDING_ONE_SPLIT) ? 1 : 2048)" in text
    got = split_check(chunk, 65535, 1 if one else 2048)
    assert set(got) == {(i, u) for i in ITEMS for u in UNITS}
    for (i, u), pair in got.items():
        assert pair == old_wn_splits(i, u, one, chunk), (i, u, one)
        if one:
            assert pair == (1, u)
