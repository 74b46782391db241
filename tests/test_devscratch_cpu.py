"""The scaffold the device-side mesh builds share (csrc/devscratch.h, csrc/scratcharena.h, csrc/meshedit.h, surfd_amd/meshconn.py),
without a GPU: the source text of its five users.  What the scaffold replaced must not come back beside it: a temporary freed by
hand, a hipcub call sized by hand, a second copy of a shared helper, kernel or macro, a second copy of the constructors' checks.
The arena's carving arithmetic is host C++: a stand-alone program (tools/scratcharena_check.cpp) carves the slots of every call
site from a host block, and this file compares its offsets with the arithmetic the arena replaced."""
import os
import re
import subprocess

import pytest

from surfd_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surfd_amd", "csrc")
USERS = ("meshtopo.hip", "meshsmooth.hip", "meshbvh.hip", "meshclean.hip", "meshsimplify.hip")
HANDLELESS = ("meshclean.hip", "meshsimplify.hip")        # calls, not handles: they own nothing to free


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
    if name in HANDLELESS:
        assert not freed, freed
    else:
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
    for gone in ("mt_total_kernel", "ms_total_kernel", "mt_bytes", "ms_bytes", "mt_grid", "ms_grid", "ms_tid", "McArena", "MsArena", "MC_LAUNCH", "MS_LAUNCH",
                 "mc_slot", "ms_slot", "mc_read", "ms_read", "mc_face_mark_kernel", "ms_face_mark_kernel", "mt_heads_kernel", "mt_weld_rep_kernel", "mc_rep_kernel"):
        assert gone not in everything, gone
    # the 64-bit thread index everywhere: no 32-bit product of block index and block size is left in meshtopo.hip
    assert "blockIdx.x * blockDim.x" not in code("meshtopo.hip")
    # a __global__ in a header is compiled into every code object that includes it: it must be static (or a template)
    assert re.findall(r"(\w+) __global__", header) == ["static"]


def global_names(text: str):
    """the names of the __global__ functions a source text defines"""
    for bounds in set(calls(text, "__launch_bounds__")):
        text = text.replace(f"__launch_bounds__({bounds})", "")
    return re.findall(r"__global__\s+void\s+(\w+)\s*\(", text)


def test_the_shared_pieces_exist_once_and_nothing_beside_them():
    header, arena, shared = code("devscratch.h"), code("scratcharena.h"), code("meshedit.h")
    assert '#include "scratcharena.h"' in header and "hip" not in arena.lower()              # the carving arithmetic makes no HIP call
    for piece in ("#define DEV_LAUNCH(", "int read_words(", "int zeroed_words(", "int mesh_sizes("):
        assert header.count(piece) == 1, piece
    for piece in ("class ScratchArena", "size_t dev_slot(long n)", "void adopt(", "int open("):
        assert arena.count(piece) == 1, piece
    for piece in ("void face_mark_kernel(", "void run_heads_kernel(", "void group_rep_kernel(", "int group_representatives(", "int vertex_nonfinite("):
        assert shared.count(piece) == 1, piece
    # every kernel of meshedit.h is static or a template
    kernels = re.findall(r"(static|template <[^>]*>\n)\s*__global__ void (\w+)\(", shared)
    assert [k for _, k in kernels] == global_names(shared) == ["face_mark_kernel", "run_heads_kernel", "group_rep_kernel"]
    for name in USERS:
        text = code(name)
        # the launch macro, the read-back and the size refusal are the header's: none is written out or defined again
        assert "dim3(dev_grid(" not in text and "#define" not in text.replace("#define MT_LD(p)", ""), name
        assert "hipMemcpyDeviceToHost" not in text or name == "meshbvh.hip", name          # its visit counters are two 64-bit words
        assert "F = %d, V = %d must not be negative" not in text and "3 F must stay" not in text, name
    assert "dim3(dev_grid(" in header
    assert not re.search(r"\b(ms|MS)_\w|\bMs[A-Z]", open(os.path.join(CSRC, "meshsimplify.hip")).read())
    for name in ("meshclean.hip", "meshsimplify.hip"):
        assert '#include "meshedit.h"' in code(name) and "ScratchArena" in code(name)
    weld, cull = (re.search(rf'extern "C" int {fn}\(.*?\n}}\n', code(src), re.S).group(0)
                  for fn, src in (("surfd_meshtopo_weld", "meshtopo.hip"), ("surfd_meshclean_cull_and_merge", "meshclean.hip")))
    assert weld.count("group_representatives(") == cull.count("group_representatives(") == 1
    assert "inclusive_max" not in code("meshtopo.hip") + code("meshclean.hip")


def test_no_kernel_name_is_defined_in_two_files():
    """all of them are linked into one library in one namespace: two kernels of one signature would be one symbol"""
    seen = {}
    for name in sorted(f for f in os.listdir(CSRC) if f.endswith(".hip")):
        for kernel in global_names(code(name)):
            assert kernel not in seen, (kernel, seen[kernel], name)
            seen[kernel] = name
    assert len(seen) == sum(code(f).count("__global__") for f in os.listdir(CSRC) if f.endswith(".hip"))      # the pattern missed none
    assert seen["vc_keys_kernel"] == "meshsimplify.hip" and seen["ms_keys_kernel"] == "meshsmooth.hip"


# ---- the arena's arithmetic, on the host -------------------------------------------------------------------------------------
SITES = {"cull_and_merge": ("meshclean.hip", "surfd_meshclean_cull_and_merge", "arena"),
         "drop_duplicate_faces": ("meshclean.hip", "surfd_meshclean_drop_duplicate_faces", "arena"),
         "drop_degenerate_faces": ("meshclean.hip", "surfd_meshclean_drop_degenerate_faces", "arena"),
         "fill_small_holes": ("meshclean.hip", "surfd_meshclean_fill_small_holes", "arena"),
         "cluster_stage1": ("meshsimplify.hip", "surfd_meshsimplify_cluster", "arena"),
         "cluster_stage2": ("meshsimplify.hip", "surfd_meshsimplify_cluster", "stage")}


def old_slot(n: int, size: int) -> int:
    """mc_slot / ms_slot as they stood: dev_bytes rounded up to 256"""
    return (max(n, 1) * size + 255) & ~255


def build_arena_check(tmp_path, *flags):
    exe = str(tmp_path / ("scratcharena_check" + ("_san" if flags else "")))
    src = os.path.join(ROOT, "tools", "scratcharena_check.cpp")
    assert '#include "../surfd_amd/csrc/scratcharena.h"' in open(src).read()
    r = subprocess.run([B._hipcc(), "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only", *flags, src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def check_arena_output(exe, F, V, C, kept, live):
    r = subprocess.run([exe] + [str(x) for x in (F, V, C, kept, live)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    rows = [line.split(None, 3) for line in r.stdout.splitlines()]                          # site, slot | total | refused, ...
    for site, (src, fn, arena) in SITES.items():
        mine = [row[1:] for row in rows if row[0] == site]
        slots = [(name, int(size), *map(int, rest.split())) for name, size, rest in mine[:-2]]      # name, element bytes, elements, offset
        total, refused = mine[-2:]
        offset = 0
        for name, size, n, at in slots:
            assert at == offset and at % 256 == 0, (site, name, at, offset)
            offset += old_slot(n, size)
        assert total[0] == "total" and int(total[1]) == offset, (site, total, offset)
        who = src.split(".")[0]
        assert refused[0] == "refused" and int(refused[1]) == -2, (site, refused)           # SURFD_ERR_STATE
        assert refused[2] == f"{who}: the arena of the call is too small ({offset} + 256 > {offset} bytes)", refused
        # the program carves what the call site carves, in its order
        body = re.search(rf'extern "C" int {fn}\(.*?\n}}\n', code(src), re.S).group(0)
        carved = re.findall(rf"(?:{arena}\.get\(|zeroed_words\({arena}, )&(\w+),", body)
        assert carved == [name for name, *_ in slots], (site, carved)
    assert {row[0] for row in rows} == set(SITES)


def test_the_arena_carves_what_the_private_arenas_carved(tmp_path):
    exe = build_arena_check(tmp_path)
    for F in (0, 1, 257):
        for V in (0, 1, 257):
            check_arena_output(exe, F, V, min(V, 3 * F), F, max(F - 1, 0))
    check_arena_output(exe, 70_000, 35_002, 1, 70_000, 0)                                   # one cluster: three clusters' worth of nothing


def test_the_arena_under_host_sanitizers(tmp_path):
    """a stand-alone host program (its own main), built with ASan + UBSan and run as a child: every slot's first and last byte is
    written inside a block of exactly the size the call site opens"""
    exe = build_arena_check(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for F, V in ((0, 0), (1, 1), (257, 257), (257, 1), (1, 257)):
        check_arena_output(exe, F, V, V, F, F)


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
