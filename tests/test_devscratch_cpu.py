"""The scaffold the device-side mesh builds share (csrc/devscratch.h, surfd_amd/meshconn.py), without a GPU: the source text of
its three users.  What the scaffold replaced must not come back beside it: a temporary freed by hand, a hipcub call sized by
hand, a second copy of a shared helper, a second copy of the constructors' checks."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surfd_amd", "csrc")
USERS = ("meshtopo.hip", "meshsmooth.hip", "meshbvh.hip")


def code(name: str) -> str:
    """a source file without its // comments"""
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def calls(text: str, name: str):
    """the argument text of every call of ``name`` (nested parentheses followed)"""
    out = []
    for m in re.finditer(re.escape(name) + r"\s*\(", text):
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        out.append(text[m.end():i - 1])
    return out


@pytest.mark.parametrize("name", USERS)
def test_the_builds_use_the_scaffold(name):
    text = code(name)
    assert '#include "devscratch.h"' in text
    assert "DeviceScratch scratch;" in text and "CubWorkspace cub{&scratch};" in text
    # only what a handle owns is freed by hand (m->..., b->...), and only in the handle's free function
    freed = calls(text, "hipFree")
    assert freed and all(re.fullmatch(r"(m|b)->\w+(\.ptr)?", a.strip()) for a in freed), freed
    # hipcub is reached through the workspace alone: no size query with a null workspace, no call at all
    assert "hipcub::" not in text and "hipcub/hipcub.hpp" not in text
    assert "auto run = [&]" not in text


def test_the_header_has_each_shared_piece_once():
    header = code("devscratch.h")
    for piece in ("class DeviceScratch", "struct CubWorkspace", "dev_bytes(long n)", "dev_grid(long n)", "long dev_tid()", "void scan_total_kernel("):
        assert header.count(piece) == 1, piece
    assert "DeviceScratch(const DeviceScratch &) = delete" in header
    for op in ("DeviceRadixSort::SortPairs", "DeviceScan::ExclusiveSum", "DeviceScan::InclusiveScan", "DeviceReduce::Sum"):
        assert header.count("hipcub::" + op) == 1, op
    everything = "".join(code(n) for n in USERS)
    for gone in ("mt_total_kernel", "ms_total_kernel", "mt_bytes", "ms_bytes", "mt_grid", "ms_grid", "ms_tid"):
        assert gone not in everything, gone
    # the 64-bit thread index everywhere: no 32-bit product of block index and block size is left in meshtopo.hip
    assert "blockIdx.x * blockDim.x" not in code("meshtopo.hip")
    # a __global__ in a header is compiled into every code object that includes it: it must be static (or a template)
    assert re.findall(r"(\w+) __global__", header) == ["static"]


def test_the_connectivity_handles_share_one_base():
    from surfd_amd.meshconn import _MeshConnectivity
    from surfd_amd.meshsmooth import MeshSmoother
    from surfd_amd.meshtopo import MeshTopology
    for cls, abi in ((MeshTopology, "surfd_meshtopo"), (MeshSmoother, "surfd_meshsmooth")):
        assert cls.__mro__[1:] == (_MeshConnectivity, object) and cls._abi == abi
        assert "__del__" not in vars(cls) and "_check" not in vars(cls) and "_open" not in vars(cls)
        assert "no CPU fallback" in cls._no_cpu()
    assert MeshTopology._no_cpu() != MeshSmoother._no_cpu()
    for module in ("meshtopo.py", "meshsmooth.py"):
        text = open(os.path.join(ROOT, "surfd_amd", module)).read()
        assert "def _check_triangles" not in text and "def _check_vertices" not in text and "c_void_p" not in text
