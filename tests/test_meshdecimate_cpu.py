"""tests/meshdecimate_ref.py is the contract of the edge-collapse decimation (csrc/meshdecimate.hip equals it bit for bit): here it
is pinned itself.  Counts and stop reasons, the topology it keeps on manifold input (through tests/meshtopo_ref.py), the figures of
profiles/meshdecimate_ref_check.json, each validity rule on a mesh made for it, the cut, the hashed tie order, the integer mix, the
input rules, the seed, and the agreement of header, binding and appendix on the export.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import meshdecimate_ref as R
import meshsimplify_ref as MS
import meshtopo_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The measured distances are 0.0 (profiles/meshdecimate_ref_check.json): on flat faces and straight borders every quadric is that
# of the planes through them, and the grids' coordinates are exact.  The bound is what fp64 allows instead: a point is the solution
# of a 3 x 3 system whose kept eigenvalues span at most 1 / rank_tol = 1e3, so an error of 1e3 * 2.2e-16 * extent per collapse, over
# chains of at most some tens of rounds: below 1e-11 * extent.  Two orders of margin on that: 1e-9 * extent.
DIST_BOUND = 1e-9


def topo(v, f):
    s = T.summary(T.build(f, len(v)))
    return {k: s[k] for k in ("edge_manifold", "components_vertex", "components_edge", "euler_characteristic", "closed", "border_loops",
                              "consistently_oriented")}


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(ROOT, "profiles", "meshdecimate_ref_check.json")))


def test_target_at_or_above_the_face_count_returns_the_kept_faces():
    v, f = R.octahedron()
    for target in (8, 9, 10 ** 9):
        ov, of, vm, c = R.decimate(v, f, target)
        assert np.array_equal(ov.view(np.int64), v.view(np.int64)) and np.array_equal(of, f) and np.array_equal(vm, np.arange(6))
        assert c["rounds"] == 0 and c["collapses"] == 0 and c["stop"] == 0 and c["faces"] == 8 and c["vertices"] == 6


def test_tetrahedron_stalls_on_the_opposite_vertices():
    v, f = R.tetrahedron()
    ov, of, vm, c = R.decimate(v, f, 2)
    assert R.STOP_NAMES[c["stop"]] == "stalled" and c["faces"] == 4 and c["rounds"] == 1 and c["refused_opposite"] == 6
    assert np.array_equal(of, f) and np.array_equal(ov, v)


@pytest.mark.parametrize("name,target,faces,verts", [("octahedron", 6, 6, 5), ("octahedron", 4, 4, 4), ("cube12", 6, 6, 5), ("cube12", 8, 8, 6)])
def test_small_closed_solids(name, target, faces, verts):
    v, f = getattr(R, name)()
    ov, of, vm, c = R.decimate(v, f, target)
    assert (c["faces"], c["vertices"], c["stop"]) == (faces, verts, 0) and c["collapses"] == (len(f) - faces) // 2
    assert topo(ov, of) == topo(v, f)
    assert vm.min() >= 0 and vm.max() == verts - 1 and len(np.unique(vm)) == verts


def test_two_disjoint_spheres_stay_two():
    v, f = R.two_spheres()
    ov, of, vm, c = R.decimate(v, f, 40)
    assert c["faces"] in (39, 40) and topo(ov, of) == topo(v, f) and topo(ov, of)["components_vertex"] == 2
    left = vm[:len(v) // 2]
    assert set(left) & set(vm[len(v) // 2:]) == set()              # no vertex of one sphere ended in the other


@pytest.mark.parametrize("name", ["icosphere", "sheet", "torus"])
def test_topology_is_kept_on_manifold_input(name):
    v, f = {"icosphere": lambda: R.icosphere(3), "sheet": lambda: R.sheet_mesh(17, 17, bump=0.3), "torus": R.torus_mesh}[name]()
    target = {"icosphere": 128, "sheet": len(f) // 4, "torus": len(f) // 4}[name]
    ov, of, vm, c = R.decimate(v, f, target)
    before, after = topo(v, f), topo(ov, of)
    print(name, c, after)
    assert after == before and c["stop"] == 0
    if before["closed"]:
        assert target - 1 <= len(of) <= target
        assert c["border_collapses"] == 0 and len(f) - len(of) == 2 * c["collapses"]
    else:
        assert len(of) <= target and c["border_collapses"] > 0
    assert len(of) == c["faces"] and len(ov) == c["vertices"] and of.max() == len(ov) - 1 and len(np.unique(of)) == len(ov)
    assert np.isfinite(ov).all() and (vm >= 0).all()
    if name == "icosphere":                                     # every output face looks outward
        n = np.cross(ov[of[:, 1]] - ov[of[:, 0]], ov[of[:, 2]] - ov[of[:, 0]])
        assert ((n * ov[of].mean(axis=1)).sum(axis=1) > 0).all()


def test_cube_stays_on_its_surface_and_keeps_its_corners(recorded):
    v, f = MS.cube_mesh(24)
    ov, of, vm, c = R.decimate(v, f, len(f) // 10)
    d = float(MS.cube_distance(ov).max())
    print(f"cube: max distance {d:.3g}, {c}")
    rec = recorded["cube"]
    assert rec["target"] == len(f) // 10 and rec["counts"] == c and rec["max_distance"] == pytest.approx(d, abs=1e-12)
    assert d <= DIST_BOUND and 100 * rec["max_distance"] <= DIST_BOUND
    for corner in ((x, y, z) for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)):
        assert (np.abs(ov - corner).max(axis=1) <= DIST_BOUND).any(), corner
    assert topo(ov, of) == topo(v, f)


def test_flat_sheet_keeps_its_border_on_the_rectangle(recorded):
    v, f = R.sheet_mesh(17, 17)
    ov, of, vm, c = R.decimate(v, f, len(f) // 4)
    d = float(R.sheet_border_distance(ov[R.border_vertices(of)], 17, 17).max())
    print(f"sheet: border max distance {d:.3g}, {c}")
    rec = recorded["sheet"]
    assert rec["target"] == len(f) // 4 and rec["counts"] == c and rec["border_max_distance"] == pytest.approx(d, abs=1e-12)
    assert d <= 17 * DIST_BOUND and 100 * rec["border_max_distance"] <= 17 * DIST_BOUND
    assert np.abs(ov[:, 2]).max() <= 17 * DIST_BOUND and topo(ov, of) == topo(v, f)
    for corner in ((0.0, 0.0), (17.0, 0.0), (0.0, 17.0), (17.0, 17.0)):     # a corner vertex has no valid edge: both border edges are refused by (e) or move it
        assert (np.abs(ov[:, :2] - corner).max(axis=1) <= 17 * DIST_BOUND).any(), corner


def test_sphere_faces_look_outward(recorded):
    """the 48 x 96 sphere at the face count clustering with cell 0.1 gives: every output face looks outward.  Decimation's and
    clustering's radial error there are recorded, nothing is asserted of their size.  (With rule (e) against the standing face
    alone, three slivers near the poles ended on their side or turned over, cosine to the radius down to -0.91, and one face of the
    icosphere at 128 faces: every collapse stayed within flip_cos of the face before it, their sum did not.  Hence the input normal.)"""
    rec = recorded["sphere"]
    assert set(rec) == {"target", "decimation_radial_error", "clustering_radial_error", "counts"} and rec["counts"]["faces"] <= rec["target"]
    v, f = MS.sphere_mesh()
    ov, of, vm, c = R.decimate(v, f, rec["target"])
    assert c == rec["counts"] and rec["target"] - 1 <= len(of) <= rec["target"]
    n = np.cross(ov[of[:, 1]] - ov[of[:, 0]], ov[of[:, 2]] - ov[of[:, 0]])
    assert ((n * ov[of].mean(axis=1)).sum(axis=1) > 0).all()
    err = float(np.abs(np.sqrt((ov ** 2).sum(axis=1)) - 1.0).max())
    print(f"sphere: radial error decimation {err:.4g}, clustering {rec['clustering_radial_error']:.4g}")
    assert rec["decimation_radial_error"] == pytest.approx(err, rel=1e-6)
    assert topo(ov, of) == topo(v, f)


@pytest.mark.parametrize("rule", ["refused_valence", "refused_link", "refused_border", "refused_opposite", "refused_flip"])
def test_each_rule_refuses_the_edge_made_for_it(rule):
    v, f, (lo, hi) = R.rule_meshes()[rule]
    assert len(f) <= 12
    trace = []
    R.decimate(v, f, 0, max_rounds=1, trace=trace)
    t = trace[0]
    e = int(np.nonzero((t["elo"] == lo) & (t["ehi"] == hi))[0][0])
    column = ("refused_valence", "refused_link", "refused_border", "refused_opposite", "refused_nan", "refused_flip").index(rule)
    assert int(np.argmax(t["rules"][e])) == column and t["rules"][e, column], t["rules"][e]
    assert t["key"][e] == np.uint64(R.M64) and e not in t["chosen"]
    out = R.decimate(v, f, 0, max_rounds=1)
    assert out[3][rule] >= 1


def test_nan_cost_is_refused():
    """coordinates whose squares overflow: Inf - Inf in the cost"""
    v, f = R.sheet_mesh(2, 2)
    ov, of, vm, c = R.decimate(v * 1e200, f, 4, max_rounds=1)
    assert c["refused_nan"] > 0 and c["collapses"] == 0 and c["stop"] == 1 and np.array_equal(of, f)


def test_the_cut_keeps_the_lowest_sort_ranks():
    v, f = R.sheet_mesh(17, 17)
    trace = []
    ov, of, vm, c = R.decimate(v, f, len(f) - 3, spread=64, trace=trace)             # remaining = 2
    t = trace[0]
    assert t["candidates"] == 128 and len(t["independent"]) > 2 and t["selected"] == 2 and c["collapses"] == 2 and c["rounds"] == 1
    rank = np.empty(t["edges"], np.int64)
    rank[t["rank_order"]] = np.arange(t["edges"])
    assert sorted(rank[t["independent"]])[:2] == sorted(rank[t["chosen"]]) and len(of) == len(f) - 4
    # spread 1: as many candidates as collapses still to go
    trace = []
    R.decimate(v, f, len(f) - 3, spread=1, trace=trace)
    assert trace[0]["candidates"] == 2 and trace[0]["selected"] <= 2


def test_equal_costs_are_ordered_by_the_hash_not_by_the_edge():
    v, f = R.sheet_mesh(17, 17)                                 # flat: every cost is 0.0
    trace = []
    R.decimate(v, f, len(f) // 2, seed=3, max_rounds=1, trace=trace)
    t = trace[0]
    valid = ~t["rules"].any(axis=1)
    assert (t["cost"][valid] == 0.0).all() and valid.sum() > 500
    low = R.mix64(3, 0, t["elo"], t["ehi"]) & np.uint64(0xffffffff)
    want = np.nonzero(valid)[0][np.argsort(low[valid], kind="stable")]
    assert np.array_equal(t["rank_order"][:valid.sum()], want) and not np.array_equal(want, np.sort(want))
    assert (t["key"][valid] >> np.uint64(32) == 0).all()
    # the selected edges touch no common face: no end point of one is an end point or a neighbour of another
    ends = np.concatenate((t["elo"][t["chosen"]], t["ehi"][t["chosen"]]))
    assert len(np.unique(ends)) == len(ends)
    adjacent = set(zip(t["elo"].tolist(), t["ehi"].tolist()))
    own = set(zip(t["elo"][t["chosen"]].tolist(), t["ehi"][t["chosen"]].tolist()))
    es = sorted(ends.tolist())
    assert not [(a, b) for i, a in enumerate(es) for b in es[i + 1:] if (a, b) in adjacent and (a, b) not in own]


def _mix_by_hand(seed, rnd, lo, hi):
    m = (1 << 64) - 1

    def fin(x):
        x ^= x >> 30; x = x * 0xbf58476d1ce4e5b9 & m
        x ^= x >> 27; x = x * 0x94d049bb133111eb & m
        return x ^ (x >> 31)
    return fin(fin((seed + 0x9e3779b97f4a7c15 * (rnd + 1)) & m) ^ (lo << 32 | hi))


@pytest.mark.parametrize("args,value", [((0, 0, 0, 1), 0x9e0160293a33aaf7), ((1, 2, 3, 4), 0xb64447aaaeb323ca),
                                        ((2 ** 64 - 1, 511, 2 ** 31 - 2, 2 ** 31 - 1), 0xa5440507020b61f5)])
def test_mix_values(args, value):
    assert int(R.mix64(*args)) == value == _mix_by_hand(*args)
    assert int(R.mix64(args[0], args[1], np.array([args[2]]), np.array([args[3]]))[0]) == value


def test_input_rules():
    nan = float("nan")
    v, f = R.octahedron()
    v2 = np.concatenate((v, [[nan, 0, 0], [9.0, 9, 9], [0.5, 0.5, 0.5]]))          # 6 a NaN, 7 unreferenced, 8 named by a dropped face only
    f2 = np.concatenate(([[0, 6, 2]], f[:4], [[8, 8, 1], [3, 8, 3]], f[4:]))
    ov, of, vm, c = R.decimate(v2, f2, 100)
    assert np.array_equal(of, f) and np.array_equal(ov, v) and vm.tolist() == [0, 1, 2, 3, 4, 5, -1, -1, -1] and c["rounds"] == 0
    a, b = R.decimate(v2, f2, 4), R.decimate(v, f, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2][:6], b[2]) and (a[2][6:] == -1).all() and a[3] == b[3]
    with pytest.raises(ValueError, match="outside"):
        R.decimate(v, np.array([[0, 1, 6]]), 0)
    with pytest.raises(ValueError, match="outside"):
        R.decimate(v, np.array([[0, -1, 2]]), 0)
    for kw in (dict(target_faces=-1), dict(target_faces=4, spread=0), dict(target_faces=4, max_rounds=0), dict(target_faces=4, flip_cos=1.0),
               dict(target_faces=4, border_weight=nan), dict(target_faces=4, rank_tol=0.0), dict(target_faces=4, border_weight=-1.0)):
        with pytest.raises(ValueError):
            R.decimate(v, f, **kw)
    assert R.decimate(np.zeros((0, 3)), np.zeros((0, 3), np.int64), 0)[3]["faces"] == 0
    e = R.decimate(v, np.zeros((0, 3), np.int64), 0)
    assert len(e[0]) == 0 and (e[2] == -1).all()
    n = R.decimate(np.full((3, 3), nan), np.array([[0, 1, 2]]), 0)
    assert len(n[0]) == 0 and len(n[1]) == 0 and (n[2] == -1).all() and n[3]["rounds"] == 0


def test_max_rounds_stops_in_between():
    v, f = R.icosphere(2)
    one, two, full = (R.decimate(v, f, 32, max_rounds=k) for k in (1, 2, 512))
    assert one[3]["stop"] == 2 and two[3]["stop"] == 2 and full[3]["stop"] == 0 and one[3]["rounds"] == 1 and two[3]["rounds"] == 2
    assert len(f) > one[3]["faces"] > two[3]["faces"] > full[3]["faces"] >= 31
    assert topo(one[0], one[1]) == topo(v, f) == topo(two[0], two[1])


def test_seed_changes_the_result_and_repeats_itself():
    v, f = R.icosphere(2)
    a, b, c = R.decimate(v, f, 64, seed=1), R.decimate(v, f, 64, seed=1), R.decimate(v, f, 64, seed=2)
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert not np.array_equal(a[2], c[2])
    assert topo(c[0], c[1]) == topo(a[0], a[1]) == topo(v, f)
    big = R.decimate(v, f, 64, seed=2 ** 64 + 1)                # the seed is taken modulo 2^64
    assert np.array_equal(big[2], a[2])


def test_header_binding_and_appendix_agree():
    import ctypes as C
    from surfd_amd import _native as N
    name = "surfd_meshsimplify_decimate"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "surfd_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, "not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    kinds = ["ptr" if "*" in p else p.rsplit(" ", 1)[0] for p in params]
    assert kinds == ["ptr", "int", "ptr", "int", "int64_t", "double", "double", "double", "int", "int", "uint64_t", "ptr", "ptr", "ptr", "ptr", "surfd_stream"]
    assert [p.rsplit(" ", 1)[1].lstrip("*") for p in params] == ["vertices", "V", "faces", "F", "target_faces", "border_weight", "flip_cos", "rank_tol", "spread",
                                                                 "max_rounds", "seed", "out_vertices", "out_faces", "vertex_map", "counts", "s"]
    res, args = N._SIGS[name]
    assert res is C.c_int and name in N.EXPORTED_SYMBOLS
    as_kind = {C.c_int: "int", C.c_double: "double", C.c_int64: "int64_t", C.c_uint64: "uint64_t"}
    assert [as_kind.get(a, "ptr") for a in args[:-1]] + ["surfd_stream"] == kinds and args[-1] is C.c_void_p and args[14] is N.c_i64p
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"| `{name}` |" in doc[doc.index("## Appendix: every export"):]
    from surfd_amd import meshsimplify
    assert meshsimplify.DECIMATE_STAT_NAMES == R.COUNT_NAMES and meshsimplify.DECIMATE_STOPS == R.STOP_NAMES
    if os.path.exists(N.LIB_PATH):
        assert hasattr(C.CDLL(N.LIB_PATH), name)
    hip = open(os.path.join(ROOT, "surfd_amd", "csrc", "meshdecimate.hip")).read()
    kernels = re.findall(r"__global__ void (?:__launch_bounds__\(256\) )?(\w+)\(", hip)
    assert len(kernels) == hip.count("__global__") and all(k.startswith("qd_") and k.endswith("_kernel") for k in kernels)
    assert "hipFree" not in hip and "hipMemcpyDeviceToHost" not in hip and "DEV_LAUNCH(" in hip and "read_words(" in hip and "mesh_sizes(" in hip
    from surfd_amd import build
    assert "meshdecimate.hip" in build.SOURCES


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from surfd_amd.meshsimplify import simplify_quadric_decimation
    from surfd_amd.meshudf import get_mesh_from_udf
    v, f = torch.zeros(3, 3, dtype=torch.float64), torch.tensor([[0, 1, 2]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        simplify_quadric_decimation(v, f, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        simplify_quadric_decimation(v, f, ratio=0.5)
    kw = dict(coords_range=(-1, 1), max_dist=0.1, N=16)
    with pytest.raises(ValueError, match="simplify_faces.*differentiable"):
        get_mesh_from_udf(None, differentiable=True, device_clean=True, simplify_faces=100, **kw)
    with pytest.raises(ValueError, match="simplify_faces.*device_clean"):
        get_mesh_from_udf(None, differentiable=False, device_clean=False, simplify_faces=100, **kw)
    with pytest.raises(ValueError, match="simplify_faces and simplify_cells"):
        get_mesh_from_udf(None, differentiable=False, device_clean=True, simplify_faces=100, simplify_cells=8, **kw)
    with pytest.raises(ValueError, match="simplify_faces"):
        get_mesh_from_udf(None, differentiable=False, device_clean=True, simplify_faces=-1, **kw)


def test_example_flags_follow_the_rules_of_simplify_cells():
    import sys
    sys.path.insert(0, ROOT)
    from examples import generate, reconstruct
    for bad in (["--simplify_faces", "100"], ["--simplify_faces", "100", "--watertight"], ["--simplify_faces", "100", "--simplify_cells", "8", "--device_clean"],
                ["--simplify_faces", "-1", "--device_clean"]):
        with pytest.raises(SystemExit):
            generate.parse(["uncond"] + bad)
    assert generate.parse(["uncond", "--simplify_faces", "100", "--device_clean"]).simplify_faces == 100
    assert generate.parse(["uncond", "--simplify_faces", "100", "--watertight", "--device_mc"]).simplify_faces == 100
    assert generate.parse(["uncond"]).simplify_faces is None
    for bad in (["--simplify_faces", "100", "--watertight"], ["--simplify_faces", "100", "--simplify_cells", "8"], ["--simplify_faces", "-1"]):
        with pytest.raises(SystemExit):
            reconstruct.parse(bad)
    assert reconstruct.parse(["--simplify_faces", "100"]).simplify_faces == 100
    assert reconstruct.parse(["--simplify_faces", "100", "--watertight", "--device_mc"]).simplify_faces == 100
