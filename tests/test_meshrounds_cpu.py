"""The scaffold of rounds of independent edge operations that the edge-collapse decimation and the isotropic remeshing share
(csrc/meshrounds.h), without a GPU: the source text of the header and of its two users.  What the header replaced must not come back
beside it: a second copy of a shared device piece, kernel or rule in either file, the round's structure written out again on the
host, a function the two files both define."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surfd_amd", "csrc")
USERS = {"meshdecimate.hip": "qd_", "meshremesh.hip": "rm_"}

DEVICE_PIECES = ["fin", "mix", "load", "normal", "dot", "keeps", "keeps_side", "before", "refused_abcd", "fans_keep_side"]
STRUCTS = ["v3", "ring", "rings"]
KERNELS = ["face_mark", "compact_kept", "face_normals", "iota", "half_keys", "edge_fill", "run_bounds", "edge_info", "vertex_min", "ring_min", "rename_faces",
           "compact_live", "mark_named", "out_faces"]
HOST_PIECES = ["salt", "kept_faces", "structure", "count_named"]
# every name the two files lost to the header, under both of their prefixes (remesh keeps its rm_u64: meshremesh_layout.h has it)
REMOVED = [p + n for p in USERS.values() for n in ["fin", "mix", "salt", "v3", "load", "normal", "dot", "keeps", "keeps_side", "ring", "rings", "before", "structure",
                                                   "count_named"] + [k + "_kernel" for k in KERNELS]]


def code(name: str) -> str:
    """a source file without its // comments"""
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def functions(text: str):
    """the names of the functions and kernels a source text defines at namespace scope"""
    return re.findall(r"^(?:static |extern \"C\" |template <[^>]*>\n)*(?:__global__ |__device__ |__host__ |__forceinline__ |inline )*[\w:<>]+[ *&]+"
                      r"(?:__launch_bounds__\(\d+\) )?(\w+)\([^;{]*\) \{", text, flags=re.M)


def test_the_header_has_each_shared_piece_once():
    header = code("meshrounds.h")
    for piece in DEVICE_PIECES + HOST_PIECES:
        assert len(re.findall(rf"^[^\n]*[ *&]er_{piece}\([^;{{]*\) \{{", header, flags=re.M)) == 1, piece
    for piece in STRUCTS:
        assert header.count(f"struct er_{piece} {{") == 1, piece
    for piece in KERNELS:
        assert header.count(f"void er_{piece}_kernel(") == 1, piece
    assert sorted(functions(header)) == sorted(["er_" + p for p in DEVICE_PIECES + HOST_PIECES] + [f"er_{k}_kernel" for k in KERNELS])
    # the finaliser is the host's too, and the host salt is made from it: no third copy of the constants
    assert "__host__ __device__ __forceinline__ er_u64 er_fin(" in header and header.count("0xbf58476d1ce4e5b9") == 1
    assert re.search(r"er_salt\(uint64_t seed, uint64_t round\) \{ return er_fin\(", header)
    # a __global__ in a header is compiled into every code object that includes it: it must be static (or a template)
    assert header.count("__global__") == len(KERNELS)
    assert all(w in ("static", ">") for w in re.findall(r"(\S+)\s+__global__", header))
    # the two merged kernels take a nullable argument
    assert "if (part && k)" in header and "if (vheavy && val >= 3)" in header


def test_only_the_two_files_include_it_and_neither_keeps_a_copy():
    including = sorted(f for f in os.listdir(CSRC) if f != "meshrounds.h" and '"meshrounds.h"' in open(os.path.join(CSRC, f)).read())
    assert including == sorted(USERS)
    for name in USERS:
        text = code(name)
        assert text.index('#include "meshedit.h"') < text.index('#include "meshrounds.h"'), name
        for gone in REMOVED:
            assert not re.search(rf"\b{gone}\b", text), (name, gone)
        # the constants of the mix and the rules' loops are the header's
        for gone in ("0xbf58476d1ce4e5b9", "0x94d049bb133111eb", "0x9e3779b97f4a7c15", "++common", "rings.degree(o)", "t[0] == other"):
            assert gone not in text, (name, gone)
        # the structure of a round is made by er_structure alone: no sort of the half-edge keys that runs (the two that only make
        # room end in `true`), no heads of their runs, no edge fill
        sorts = [c for c in re.findall(r"sort_pairs\(([^;]*)\);", text) if "hkey" in c]
        assert all(c.rstrip(") ").endswith("true") for c in sorts), (name, sorts)
        assert "run_heads_kernel" not in text and "edge_fill" not in text and "32 + vbits" not in text, name
        assert "er_structure(" in text and "er_kept_faces(" in text and "er_count_named(" in text and "er_salt(" in text, name
        assert "er_refused_abcd(" in text and "er_fans_keep_side(" in text, name
    # remesh hands er_structure its arrays as they are at the call: no second struct of its pointers, stored or not
    remesh = code("meshremesh.hip")
    assert "er_structure(m->a, m->cub," in remesh and "struct rm_arrays" not in remesh and remesh.count("rm_arrays a") == 1      # the handle's member
    assert "rm_round_zero_bytes(m->Vcap)" in remesh and "7 * dev_slot<int>(V)" in code("meshdecimate.hip")      # the memsets stay with the callers


def test_no_function_is_defined_in_both_files():
    names = {}
    for name, prefix in USERS.items():
        defined = functions(code(name))
        assert len([d for d in defined if d.endswith("_kernel")]) == code(name).count("__global__"), name      # the pattern missed no kernel
        assert all(d.startswith((prefix, "surfd_")) for d in defined), (name, defined)
        names[name] = {d[len(prefix):] for d in defined if d.startswith(prefix)}
    assert len(names["meshdecimate.hip"]) >= 12 and len(names["meshremesh.hip"]) >= 20
    assert not names["meshdecimate.hip"] & names["meshremesh.hip"]
