"""tests/meshremesh_ref.py is the contract of the isotropic remeshing (csrc/meshremesh.hip equals it bit for bit): here it is pinned
itself.  Hand-checked cases of every stage, the topology it keeps on manifold input after every iteration (through
tests/meshtopo_ref.py), the split stage alone, the independence of what a round selects, the figures of
profiles/meshremesh_ref_check.json with the direction they must have on a marching-cubes shell, and the agreement of header,
binding and appendix on the exports.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import meshremesh_ref as R
import meshtopo_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPO = ("edge_manifold", "components_vertex", "components_edge", "euler_characteristic", "closed", "border_loops", "consistently_oriented")


def topo(v, f):
    s = T.summary(T.build(f, len(v)))
    return {k: s[k] for k in TOPO}


def normals(v, f):
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


def canon(f):
    """faces as a sorted list of rotations that start at their smallest corner: the winding is kept"""
    f = np.asarray(f)
    k = f.argmin(axis=1)
    return sorted(tuple(int(row[(s + i) % 3]) for i in range(3)) for row, s in zip(f, k))


def plane(points):
    return np.array([[x, y, 0.0] for x, y in points])


# ---- A: split -------------------------------------------------------------------------------------------------------------------
def test_two_triangles_with_one_long_shared_edge_become_four():
    v = plane([(0, 0), (2, 0), (1, .5), (1, -.5)])
    r = R.Remesher(v, [[0, 1, 2], [1, 0, 3]], low2=0.01, high2=2.56)          # the sides are sqrt(1.25) long, the shared edge 2
    assert r.split_round() == 1
    assert r.fa.tolist() == [[0, 4, 2], [4, 1, 2], [1, 4, 3], [4, 0, 3]]
    assert r.X[4].tolist() == [1.0, 0.0, 0.0] and r.origin.tolist() == [0, 1, 2, 3, -1]
    assert np.array_equal(r.n0, np.repeat(normals(v, np.array([[0, 1, 2], [1, 0, 3]])), 2, axis=0))
    assert r.split_round() == 0 and len(r.fa) == 4


@pytest.mark.parametrize("k,points", [(1, [(0, 0), (4, 0), (2, .5)]), (2, [(0, 0), (1, 0), (.5, 4)]), (2, [(0, 0), (1, 0), (.9, 4)]),
                                      (3, [(0, 0), (4, 0), (2, 3.5)])])
@pytest.mark.parametrize("rot", range(3))
def test_every_split_template_keeps_orientation_and_area(k, points, rot):
    v = np.roll(plane(points), rot, axis=0)                     # the same triangle, its long edges at every half-edge in turn
    r = R.Remesher(v, [[0, 1, 2]], low2=0.01, high2=9.0)
    parent = normals(v, np.array([[0, 1, 2]]))[0]
    assert r.split_round() == k and len(r.fa) == 1 + k and len(r.X) == 3 + k
    n = normals(r.X, r.fa)
    assert (n[:, 2] > 0).all() and (n[:, :2] == 0).all()
    assert abs(n[:, 2].sum() - parent[2]) <= 4 * np.finfo(float).eps * parent[2]      # exact up to the rounding of 1 + k cross products
    assert np.array_equal(r.n0, np.repeat(parent[None], 1 + k, axis=0))
    # conforming: every new vertex lies on its edge's midpoint, and every half-edge inside the parent has its twin
    elo, ehi, val, _ = R._edges(r.fa)
    inner = [(a, b) for a, b, n_ in zip(elo, ehi, val) if n_ == 2]
    assert len(inner) == {1: 1, 2: 2, 3: 3}[k] and (val <= 2).all()


def test_the_k2_diagonal_is_the_shorter_one_and_ties_go_to_the_lower_index():
    tie = plane([(0, 0), (1, 0), (.5, 4)])                     # the apex over the middle: both diagonals have the same bits
    r = R.Remesher(tie, [[0, 1, 2]], 0.01, 9.0)
    r.split_round()
    assert r.X[3].tolist() == [.25, 2, 0] and r.X[4].tolist() == [.75, 2, 0]      # edge (0, 2) comes before edge (1, 2)
    assert r.fa.tolist() == [[4, 2, 3], [0, 1, 4], [0, 4, 3]]                       # a = 0 < b = 1: the diagonal a - m1
    r = R.Remesher(tie[[1, 0, 2]], [[1, 0, 2]], 0.01, 9.0)     # the same triangle, a = 1 and b = 0
    r.split_round()
    assert r.fa.tolist() == [[3, 2, 4], [1, 0, 4], [0, 3, 4]]                       # the diagonal b - m2 starts at the lower index
    skew = plane([(0, 0), (1, 0), (.9, 4)])                    # |a m1|^2 = 4.9025, |b m2|^2 = 4.3025
    r = R.Remesher(skew, [[0, 1, 2]], 0.01, 9.0)
    r.split_round()
    assert r.fa.tolist() == [[4, 2, 3], [0, 1, 3], [1, 4, 3]]


def test_split_alone_leaves_no_long_edge():
    v, f = R.icosphere(1)
    L = np.sqrt(R._len2(v[f[:1, 0]], v[f[:1, 1]]))[0] / 4
    ov, of, origin, stats = R.remesh(v, f, L, iterations=1, split_rounds=16, collapse_rounds=0, flip_rounds=0, relax_sweeps=0)
    _, high2 = R.bounds2(L)
    elo, ehi, _, _ = R._edges(of)
    c = stats[0]
    assert (R._len2(ov[elo], ov[ehi]) <= high2).all() and c["split_marked"] == 0 and 2 <= c["split_rounds"] <= 16
    assert len(ov) == len(v) + c["splits"] and len(of) == len(f) + 2 * c["splits"] and len(of) >= 16 * len(f)
    assert topo(ov, of) == topo(v, f) and (origin[:len(v)] == np.arange(len(v))).all() and (origin[len(v):] == -1).all()
    assert c["collapse_rounds"] == c["flip_rounds"] == c["collapses"] == c["flips"] == c["relaxed"] == 0


# ---- B: collapse ----------------------------------------------------------------------------------------------------------------
def pulled_sheet():
    """the flat 4 x 4 sheet with its middle vertex 12 pulled to (1.3, 1.3), 0.42 from vertex 6 and 2.4 from vertex 18"""
    v, f = R.sheet_mesh(4, 4)
    v = v.copy()
    v[12] = [1.3, 1.3, 0.0]
    return v, f


def test_a_collapse_that_would_make_a_long_edge_is_refused_by_rule_f_alone():
    v, f = pulled_sheet()
    for high2, taken in ((4.0, 0), (9.0, 1)):                   # from the midpoint (1.15, 1.15) vertex 18 is sqrt(6.845) away
        r = R.Remesher(v, f, low2=0.25, high2=high2)
        r.trace = []
        c = dict.fromkeys(R.COUNT_NAMES, 0)
        assert r.collapse_round(c) == taken
        t = r.trace[0]
        e = np.nonzero(t["short"])[0]
        assert len(e) == 1 and (t["elo"][e[0]], t["ehi"][e[0]]) == (6, 12)
        # the rules of the decimation (a) (b) (c) (d) and (e) allow it at either bound; (f) is what refuses it at the lower one
        assert t["rules"][e[0]].tolist() == [False, False, False, False, not taken, False]
        assert c["collapse_refused_long"] == 1 - taken and c["collapses"] == taken
        assert sum(c[k] for k in R.COUNT_NAMES[12:18]) == 1 - taken
        if taken:
            assert r.X[6].tolist() == [1.15, 1.15, 0.0] and r.origin[6] == -1 and len(r.fa) == len(f) - 2 and not (r.fa == 12).any()
        else:
            assert np.array_equal(r.X, v) and np.array_equal(r.fa, f) and (r.origin == np.arange(25)).all()


def test_a_collapse_next_to_the_border_goes_to_the_border_vertex():
    v, f = R.sheet_mesh(4, 4)
    v = v.copy()
    v[6] = [0.25, 1.0, 0.0]                                     # interior vertex 6 = (1, 1) pulled towards border vertex 1 = (0, 1)
    r = R.Remesher(v, f, low2=0.09, high2=9.0)
    assert r.collapse_round(dict.fromkeys(R.COUNT_NAMES, 0)) == 1
    assert np.array_equal(r.X[1].view(np.int64), v[1].view(np.int64)) and r.origin[1] == 1 and not (r.fa == 6).any()


# ---- C: flip --------------------------------------------------------------------------------------------------------------------
def test_a_flip_that_lowers_the_valence_deviation_is_taken_and_others_are_left():
    v, f = R.sheet_mesh(6, 6)
    r = R.Remesher(v, f, 0.01, 4.0)
    r.trace = []
    c = dict.fromkeys(R.COUNT_NAMES, 0)
    assert r.flip_round(c) == 0 and not r.trace[0]["looked"].any()      # every interior vertex has six edges: nothing to gain
    assert sum(c[k] for k in R.COUNT_NAMES[18:]) == 0 and np.array_equal(r.fa, f)
    # the quad of cell (2, 2) cut the other way: its corners now have 5, 7, 5, 7 edges
    a, b, cc, d = 2 * 7 + 2, 3 * 7 + 2, 3 * 7 + 3, 2 * 7 + 3
    g = f.copy()
    k = [i for i, t in enumerate(f.tolist()) if t in ([a, b, cc], [a, cc, d])]
    g[k[0]], g[k[1]] = [a, b, d], [b, cc, d]
    r = R.Remesher(v, g, 0.01, 4.0)
    r.trace = []
    assert r.flip_round(c) == 1 and c["flips"] == 1
    t = r.trace[0]
    assert t["looked"].sum() == 1 and (t["a"][t["chosen"]], t["b"][t["chosen"]]) == (d, b)
    assert canon(r.fa) == canon(f) and np.array_equal(r.n0[k[0]], r.n0[k[1]]) and r.n0[k[0]].tolist() == [0, 0, 2]
    assert r.flip_round(c) == 0


def flip_rules(v, f, high2=100.0):
    r = R.Remesher(np.asarray(v, float), f, 0.01, high2)
    r.trace = []
    r.flip_round(dict.fromkeys(R.COUNT_NAMES, 0))
    t = r.trace[0]
    return {(int(a), int(b)): rule.tolist() for a, b, rule in zip(t["a"], t["b"], t["rules"])}, t, r


def test_each_flip_refusal():
    # (same, edge, degree, long, fold) of the edge named
    rules, t, _ = flip_rules(*R.tetrahedron())                   # c - d is an edge already, and every vertex has three edges
    assert len(rules) == 6 and all(rule == [False, True, True, False, True] or rule[:3] == [False, True, True] for rule in rules.values())
    rules, _, _ = flip_rules(*R.octahedron())                    # four edges everywhere, c and d are opposite poles: only the fold can refuse
    assert len(rules) == 12 and all(rule[:4] == [False, False, False, False] for rule in rules.values())
    fan = plane([(0, 0), (3, 0), (0, 3), (1, 1)])               # a triangle cut at an inner point: vertex 3 has three edges
    rules, _, _ = flip_rules(fan, [[0, 1, 3], [1, 2, 3], [2, 0, 3]])
    assert rules[(0, 3)][2] and rules[(1, 3)][2] and rules[(2, 3)][2]
    kite = plane([(0, 0), (2, 0), (-1, 1), (-1, -1)])          # reflex at vertex 0: the diagonal 2 - 3 runs outside the quad
    rules, _, r = flip_rules(kite, [[0, 1, 2], [1, 0, 3]])
    assert rules == {(0, 1): [False, False, False, False, True]} and np.array_equal(r.fa, [[0, 1, 2], [1, 0, 3]])
    tall = plane([(0, 0), (1, 0), (.5, 3), (.5, -3)])          # convex, but its other diagonal is 6 long
    for high2, long in ((25.0, True), (49.0, False)):
        rules, _, _ = flip_rules(tall, [[0, 1, 2], [1, 0, 3]], high2)
        assert rules == {(0, 1): [False, False, False, long, False]}
    # two faces that run the same way along their edge, and two that are each other's reverse
    _, t, _ = flip_rules(tall, [[0, 1, 2], [0, 1, 3]])
    assert t["orient"].tolist() == [True] and not t["looked"].any()
    rules, t, _ = flip_rules(tall, [[0, 1, 2], [1, 0, 2]])
    assert all(rule[0] for rule in rules.values()) and not t["orient"].any()


# ---- D: relax -------------------------------------------------------------------------------------------------------------------
def test_a_relax_move_that_folds_a_face_is_refused():
    # a fan over an L-shaped ring: the vertex sees every ring edge from within [0, 1]^2 only, the mean of the ring is (5/3, 5/3)
    v = plane([(0, 0), (4, 0), (4, 1), (1, 1), (1, 4), (0, 4), (.5, .5)])
    f = [[6, i, (i + 1) % 6] for i in range(6)]
    r = R.Remesher(v, f, 0.01, 100.0)
    c = dict.fromkeys(R.COUNT_NAMES, 0)
    r.relax_stage(1, 1.0, c)
    assert c["relax_refused"] == 1 and c["relaxed"] == 0 and np.array_equal(r.X, v) and r.origin[6] == 6
    r.relax_stage(1, 0.25, c)                                   # a quarter of the way stays inside
    assert c["relaxed"] == 1 and r.origin[6] == -1 and np.allclose(r.X[6], [.5 + .25 * (5 / 3 - .5)] * 2 + [0]) and np.array_equal(r.X[:6], v[:6])
    assert (normals(r.X, r.fa)[:, 2] > 0).all()


def test_border_vertices_and_vertices_with_an_origin_keep_their_bits():
    v, f = R.bumped_sheet()
    L = R.mean_edge_length(v, f)
    for scale in (1.0, 0.5, 1.7):
        ov, of, origin, stats = R.remesh(v, f, L * scale, iterations=3)
        kept = origin >= 0
        assert kept.any() and np.array_equal(ov[kept].view(np.int64), v[origin[kept]].view(np.int64))
        assert len(np.unique(origin[kept])) == kept.sum()
    # without collapses every border vertex of the input is still there, where it was
    ov, of, origin, _ = R.remesh(v, f, L, iterations=3, collapse_rounds=0)
    border = R.border_vertices(f)
    assert set(border) <= set(origin[origin >= 0])
    # a flat sheet at its own edge length has nothing to do: the first iteration turns the -0.0 that sheet_mesh leaves in z into 0.0
    # (a change of bits, so those vertices count as relaxed), the second finds nothing and the call stops
    fv, ff = R.sheet_mesh(17, 17)
    ov, of, origin, stats = R.remesh(fv, ff, R.mean_edge_length(fv, ff))
    assert len(stats) == 2 and np.array_equal(ov, fv) and np.array_equal(of, ff)
    inner = np.setdiff1d(np.arange(len(fv)), R.border_vertices(ff))
    assert stats[0]["relaxed"] == int(np.signbit(fv[inner, 2]).sum()) == int((origin < 0).sum()) and stats[1]["relaxed"] == 0
    assert all(s[k] == 0 for s in stats for k in ("splits", "collapses", "flips", "relax_refused"))
    az, _, _, one = R.remesh(np.abs(fv), ff, R.mean_edge_length(fv, ff))
    assert len(one) == 1 and np.array_equal(az.view(np.int64), np.abs(fv).view(np.int64))


# ---- invariants -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere", "torus", "bumped_sheet", "two_spheres", "cube24"])
@pytest.mark.parametrize("scale", [1.0, 0.6])
def test_topology_and_orientation_are_kept_after_every_iteration(name, scale):
    v, f = R.named_meshes()[name]
    before = topo(v, f)
    seen = []

    def each(it, r):
        ov, of, _ = r.emit()
        assert topo(ov, of) == before, (name, it)
        fa = r.fa
        assert ((fa[:, 0] != fa[:, 1]) & (fa[:, 1] != fa[:, 2]) & (fa[:, 0] != fa[:, 2])).all()
        assert ((normals(r.X, fa) * r.n0).sum(axis=1) > 0).all(), (name, it)
        seen.append(it)

    ov, of, origin, stats = R.remesh(v, f, R.mean_edge_length(v, f) * scale, iterations=3, each=each)
    assert seen == list(range(len(stats))) and stats[-1]["faces"] == len(of) and stats[-1]["vertices"] == len(ov) == len(origin)
    assert of.max() == len(ov) - 1 and len(np.unique(of)) == len(ov)


def test_selected_collapses_and_flips_are_independent():
    for name in ("torus", "icosphere", "bumped_sheet"):
        v, f = R.named_meshes()[name]
        trace = []
        R.remesh(v, f, R.mean_edge_length(v, f) * 1.5, iterations=2, trace=trace)
        made = {"collapse": 0, "flip": 0}
        for t in trace:
            if t["stage"] == "collapse":
                lo, hi = t["elo"][t["chosen"]], t["ehi"][t["chosen"]]
                ends = np.concatenate((lo, hi))
                assert len(np.unique(ends)) == len(ends)
                owner = np.full(len(v) * 8, -1)
                owner[lo] = owner[hi] = np.arange(len(lo))
                a, b = owner[t["elo"]], owner[t["ehi"]]
                assert not ((a >= 0) & (b >= 0) & (a != b)).any()          # no edge joins the end points of two selected edges
                made["collapse"] += len(lo)
            else:
                four = np.concatenate([t[k][t["chosen"]] for k in "abcd"])
                assert len(np.unique(four)) == len(four)
                made["flip"] += int(t["chosen"].sum())
        assert made["collapse"] > 0 and made["flip"] > 0, name
        assert [t["rnd"] for t in trace] == list(range(len(trace)))         # one tick per collapse or flip round of the handle's life


def test_seed_knobs_and_refusals():
    v, f = R.torus_mesh()
    L = R.mean_edge_length(v, f)
    a, b, c = (R.remesh(v, f, L, iterations=2, seed=s) for s in (1, 1 + 2 ** 64, 2))
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.array_equal(a[1], b[1]) and a[3] == b[3]
    assert not (a[1].shape == c[1].shape and np.array_equal(a[1], c[1]))
    assert R.bounds2(0.3) == ((0.8 * 0.3) * (0.8 * 0.3), (4.0 / 3.0 * 0.3) * (4.0 / 3.0 * 0.3))
    for kw in (dict(target_edge_length=0.0), dict(target_edge_length=float("nan")), dict(target_edge_length=L, low=1.5), dict(target_edge_length=L, relax=0.0),
               dict(target_edge_length=L, relax=1.5), dict(target_edge_length=L, flip_cos=1.0)):
        with pytest.raises(ValueError):
            R.remesh(v, f, **kw)
    with pytest.raises(ValueError):
        R.remesh(v, np.array([[0, 1, len(v)]]), L)
    nan = float("nan")
    ov, of, origin, stats = R.remesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [nan, 0, 0.]]), [[0, 1, 2], [0, 1, 3], [2, 2, 1]], 10.0)
    assert of.tolist() == [[0, 1, 2]] and len(ov) == 3 and len(stats) == 1
    ov, of, origin, stats = R.remesh(np.zeros((0, 3)), np.zeros((0, 3), int), 1.0)
    assert len(ov) == len(of) == len(origin) == 0 and stats[0]["split_rounds"] == stats[0]["collapse_rounds"] == stats[0]["flip_rounds"] == 1


# ---- what it reaches -------------------------------------------------------------------------------------------------------------
def close(a, b, path=""):
    """the recorded figures against a fresh run: counts and texts exactly, the measures (means, square roots and arc cosines of
    another numpy or libm, all outside the contract) to 1e-6 of their size"""
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            close(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, float):
        assert abs(a - b) <= 1e-6 * max(abs(a), abs(b), 1e-300), (path, a, b)
    else:
        assert a == b, (path, a, b)


def test_reference_check_improves_the_marching_cubes_shell():
    """profiles/meshremesh_ref_check.json is what this run gives (python tests/meshremesh_ref.py rewrites it).  On the marching-cubes
    shell the direction is asserted, and only the direction: more edges within [low L, high L], a larger mean smallest angle, a
    smaller mean |deg - t|."""
    recorded = json.load(open(os.path.join(ROOT, "profiles", "meshremesh_ref_check.json")))
    fresh = R.reference_check(R.mc_shell())
    close(json.loads(json.dumps(fresh)), recorded)
    shell = fresh["mc_shell"]
    print(json.dumps(shell, indent=1))
    assert shell["after"]["edges_in_range"] > shell["before"]["edges_in_range"]
    assert shell["after"]["min_angle_mean"] > shell["before"]["min_angle_mean"]
    assert shell["after"]["valence_deviation_mean"] < shell["before"]["valence_deviation_mean"]


def test_the_numpy_and_torch_measures_agree():
    import torch
    from surfd_amd.meshremesh import mean_edge_length, triangle_quality
    v, f = R.bumped_sheet()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    L = R.mean_edge_length(v, f)
    assert abs(mean_edge_length(tv, tf) - L) <= 1e-12 * L
    a, b = R.triangle_quality(v, f, L), triangle_quality(tv, tf, L)
    assert a.keys() == b.keys() and all(abs(a[k] - b[k]) <= 1e-9 * max(1.0, abs(a[k])) for k in a)


# ---- the exports -----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_appendix_agree():
    import ctypes as C
    from surfd_amd import _native as N
    from surfd_amd import build, meshremesh
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "surfd_hip.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    as_kind = {C.c_int: "int", C.c_double: "double", C.c_int64: "int64_t", C.c_uint64: "uint64_t"}
    want = {"create": ["ptr", "int", "ptr", "int", "double", "double", "double", "uint64_t", "surfd_stream", "ptr"], "destroy": ["ptr"],
            "iterate": ["ptr", "int", "int", "int", "int", "double", "ptr", "surfd_stream"], "sizes": ["ptr", "ptr", "ptr"],
            "get_positions": ["ptr", "ptr", "ptr", "surfd_stream"], "set_positions": ["ptr", "ptr", "surfd_stream"],
            "emit": ["ptr", "ptr", "ptr", "ptr", "ptr", "surfd_stream"]}
    for short, kinds in want.items():
        name = "surfd_meshremesh_" + short
        m = re.search(r"\b(int|void)\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(2).split(",")]
        assert ["ptr" if "*" in p else p.rsplit(" ", 1)[0] for p in params] == kinds, name
        res, args = N._SIGS[name]
        assert res is (None if m.group(1) == "void" else C.c_int) and name in N.EXPORTED_SYMBOLS
        assert [("surfd_stream" if k == "surfd_stream" else as_kind.get(a, "ptr")) for a, k in zip(args, kinds)] == kinds, name
        assert f"| `{name}` |" in doc[doc.index("## Appendix: every export"):]
        if os.path.exists(N.LIB_PATH):
            assert hasattr(C.CDLL(N.LIB_PATH), name)
    assert meshremesh.STAT_NAMES == R.COUNT_NAMES and len(R.COUNT_NAMES) == 24
    hip = open(os.path.join(ROOT, "surfd_amd", "csrc", "meshremesh.hip")).read()
    kernels = re.findall(r"__global__ void (?:__launch_bounds__\(256\) )?(\w+)\(", hip)
    assert len(kernels) == hip.count("__global__") and all(k.startswith("rm_") and k.endswith("_kernel") for k in kernels)
    assert "hipcub::" not in hip and "atomicAdd(float" not in hip and "DEV_LAUNCH(" in hip and "read_words(" in hip and "mesh_sizes(" in hip
    assert "meshremesh.hip" in build.SOURCES
    # the header comment of the kernels carries the text of the restatement's contract
    ref = open(os.path.join(ROOT, "tests", "meshremesh_ref.py")).read()
    for line in ("A split      up to split_rounds rounds.", "B collapse   up to collapse_rounds rounds, rnd = tick, tick += 1.", "C flip       up to flip_rounds rounds",
                 "D relax      relax_sweeps Jacobi sweeps", "(f) for every w of N(lo), then of N(hi), other than lo and hi: len2(x_w, point) <= high2;"):
        assert line in ref and line in hip, line
    regs = open(os.path.join(ROOT, "profiles", "meshremesh_regs.txt")).read().splitlines()[2:]
    assert {k for k in kernels} <= {row.split()[0] for row in regs} and all(row.split()[-3] == "0" for row in regs)      # no scratch


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from surfd_amd.meshremesh import remesh_isotropic
    v, f = torch.zeros(3, 3, dtype=torch.float64), torch.tensor([[0, 1, 2]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        remesh_isotropic(v, f, 1.0)
    with pytest.raises(TypeError):
        remesh_isotropic(v, f)


def test_the_consumers_refuse_before_they_mesh():
    from surfd_amd.meshudf import get_mesh_from_udf
    kw = dict(coords_range=(-1, 1), max_dist=0.1, N=16)
    with pytest.raises(ValueError, match="remesh_edge.*differentiable"):
        get_mesh_from_udf(None, differentiable=True, device_clean=True, remesh_edge=0.1, **kw)
    with pytest.raises(ValueError, match="remesh_edge.*device_clean"):
        get_mesh_from_udf(None, differentiable=False, device_clean=False, remesh_edge=0.1, **kw)
    for bad in (dict(remesh_edge=-1.0), dict(remesh_edge=float("nan")), dict(remesh_edge=0.0), dict(remesh_edge=0.1, remesh_iterations=-1)):
        with pytest.raises(ValueError, match="remesh_"):
            get_mesh_from_udf(None, differentiable=False, device_clean=True, **bad, **kw)
    import inspect
    assert [p for p in inspect.signature(get_mesh_from_udf).parameters if p.startswith("remesh")] == ["remesh_edge", "remesh_iterations"]


def test_example_flags_follow_the_rules_of_simplify_faces():
    import sys
    sys.path.insert(0, ROOT)
    from examples import generate, reconstruct
    for bad in (["--remesh_edge", "0.1"], ["--remesh_edge", "0.1", "--watertight"], ["--remesh_edge", "0.1", "--remesh_edge_mean", "1", "--device_clean"],
                ["--remesh_edge", "-1", "--device_clean"], ["--remesh_edge_mean", "0", "--device_clean"], ["--remesh_project", "--device_clean"],
                ["--remesh_iterations", "3", "--device_clean"], ["--remesh_edge", "0.1", "--remesh_iterations", "-1", "--device_clean"]):
        with pytest.raises(SystemExit):
            generate.parse(["uncond"] + bad)
    a = generate.parse(["uncond", "--remesh_edge", "0.1", "--device_clean", "--simplify_faces", "100", "--remesh_project"])
    assert (a.remesh_edge, a.remesh_edge_mean, a.remesh_iterations, a.remesh_project, a.simplify_faces) == (0.1, None, 5, True, 100)
    assert generate.parse(["uncond", "--remesh_edge_mean", "1.5", "--remesh_iterations", "2", "--watertight", "--device_mc"]).remesh_edge_mean == 1.5
    a = generate.parse(["uncond"])
    assert a.remesh_edge is None and a.remesh_edge_mean is None and not a.remesh_project
    for bad in (["--remesh_edge", "0.1", "--watertight"], ["--remesh_edge", "0.1", "--remesh_edge_mean", "1"], ["--remesh_edge", "0"], ["--remesh_project"]):
        with pytest.raises(SystemExit):
            reconstruct.parse(bad)
    assert reconstruct.parse(["--remesh_edge", "0.1", "--simplify_cells", "32"]).remesh_edge == 0.1
    assert reconstruct.parse(["--remesh_edge_mean", "1", "--watertight", "--device_mc", "--metrics", "--mesh_quality"]).mesh_quality
