"""Pins tests/meshsimplify_ref.py, the numpy restatement that the device simplification (csrc/meshsimplify.hip) must equal bit for
bit: hand-checked clusters, sums and face rules, the cube and sphere figures of profiles/meshsimplify_ref_check.json, the key range,
and the agreement of header, binding and appendix on the export.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import meshsimplify_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = (0.071, 0.1, 0.13, 0.21)
SURFACE_BOUND = 1e-12          # the issue's: four orders above the restatement's own error, ten below the mean's
MEAN_OFF = 1e-2                # the issue's: the mean leaves the cube by more than this at each of the four cells
# the points of solve_jacobi and solve_eigh differ by at most 7.6e-15 on the cube and the sphere (profiles/meshsimplify_ref_check.json:
# "jacobi_vs_eigh"); the bound is that measurement with a margin of two orders
EIGH_BOUND = 1e-12


@pytest.fixture(scope="module")
def cube():
    return R.cube_mesh(24)


@pytest.fixture(scope="module")
def sphere():
    return R.sphere_mesh()


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(ROOT, "profiles", "meshsimplify_ref_check.json")))


@pytest.mark.parametrize("rep", ["mean", "quadric"])
def test_face_rules_by_hand(rep):
    v, f = R.hand_mesh()
    ov, of, vmap, c = R.simplify(v, f, 1.0, origin=(0.0, 0.0, 0.0), representative=rep)
    # clusters in key order: a = 0, c = 1, b = 2, d = 3; face 0 -> (0, 2, 1), face 1 -> (1, 2, 0): the lowest stays with its winding
    assert of.tolist() == [[0, 2, 1]]
    assert c == {"vertices": 3, "faces": 1, "clusters": 4, "collapsed_faces": 2, "duplicate_faces": 1, "fallbacks": 0}
    assert vmap.tolist() == [0, 2, 1, 0, 2, 1, -1, -1, -1, -1, -1]
    if rep == "mean":
        assert ov.tolist() == [[0.375, 0.375, 0.375], [0.375, 1.375, 0.375], [1.375, 0.375, 0.375]]
    # the default origin is the minimum over the REFERENCED vertices: (0.25, 0.25, 0.25), not the unreferenced (-3, -3, -3)
    ov2, of2, vmap2, c2 = R.simplify(v, f, 1.0, representative=rep)
    assert c2["clusters"] == 4 and of2.tolist() == [[0, 2, 1]] and vmap2.tolist() == vmap.tolist()


@pytest.mark.parametrize("rep", ["mean", "quadric"])
def test_small_cell_returns_the_input(cube, rep):
    """every vertex alone in its cell: the vertices in ascending key order, the faces in the duplicate rule's order"""
    v, f = cube
    cell = 0.04                                              # below the spacing 1 / 24
    ov, of, vmap, c = R.simplify(v, f, cell, representative=rep)
    assert c == {"vertices": len(v), "faces": len(f), "clusters": len(v), "collapsed_faces": 0, "duplicate_faces": 0, "fallbacks": 0}
    k = np.floor(v / cell).astype(np.int64)
    order = np.lexsort((k[:, 2], k[:, 1], k[:, 0]))
    assert (vmap[order] == np.arange(len(v))).all()
    if rep == "mean":
        assert (ov.view(np.int64) == v[order].view(np.int64)).all()
    else:
        assert np.abs(ov - v[order]).max() < 1e-15
    renamed = vmap[f]
    s = np.sort(renamed, axis=1)
    expect = renamed[np.lexsort((s[:, 0], s[:, 1], s[:, 2]))]
    assert (of == expect).all()


@pytest.mark.parametrize("rep", ["mean", "quadric"])
def test_large_cell_gives_one_cluster_and_no_faces(cube, rep):
    v, f = cube
    ov, of, vmap, c = R.simplify(v, f, 4.0, representative=rep)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and (vmap == -1).all()
    assert c["clusters"] == 1 and c["collapsed_faces"] == len(f) and c["vertices"] == 0 and c["faces"] == 0


def test_mean_is_the_sequential_sum_in_member_order():
    big = 1e16
    # (1e16 + 1) - 1e16 = 0 (the 1 is lost to the rounding), (1e16 - 1e16) + 1 = 1, (1 + 1e16) - 1e16 = 0
    orders = (([big, 1.0, -big], 0.0), ([big, -big, 1.0], 1.0), ([1.0, big, -big], 0.0))
    for xs, total in orders:
        assert R._sequential_sums(np.array(xs)[:, None], np.array([0]), np.array([3]))[0, 0] == total
    # through simplify: the three share the cell (0, 0, 0) of a grid of 4e16 from (-2e16, 0, 0); the other two corners lie in the
    # cells (0, 1, 0) and (0, 0, 1), so the keys ascend as (0,0,0) < (0,0,1) < (0,1,0) and the three faces become one
    for xs, total in orders:
        v, f = R.order_mesh(xs)
        ov, of, vmap, c = R.simplify(v, f, 4e16, origin=(-2e16, 0.0, 0.0), representative="mean")
        assert c["clusters"] == 3 and c["duplicate_faces"] == 2 and of.tolist() == [[0, 2, 1]] and vmap.tolist() == [0, 0, 0, 2, 1]
        assert ov[0].tolist() == [total / 3.0, 0.25, 0.25]


@pytest.mark.parametrize("cell", CELLS)
def test_cube_quadric_stays_on_the_surface_and_mean_does_not(cube, recorded, cell):
    v, f = cube
    ov, of, _, c = R.simplify(v, f, cell, representative="quadric")
    dq = float(R.cube_distance(ov).max())
    om, _, _, cm = R.simplify(v, f, cell, representative="mean")
    dm = float(R.cube_distance(om).max())
    print(f"cell {cell}: quadric {dq:.3g}, mean {dm:.3g}, {c}")
    assert c["fallbacks"] == 0
    assert dq <= SURFACE_BOUND
    assert dm > MEAN_OFF
    corners = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    corner = max(float(np.sqrt(((ov - k) ** 2).sum(axis=1)).min()) for k in corners)
    assert corner <= SURFACE_BOUND                          # a vertex at every corner
    rec = recorded["cube"][str(cell)]
    assert rec["quadric_max_distance"] == dq and rec["mean_max_distance"] == dm and rec["counts"] == c and rec["quadric_corner_distance"] == corner


def test_sphere_quadric_and_mean_agree_to_three_digits(sphere, recorded):
    v, f = sphere
    oq, fq, _, cq = R.simplify(v, f, 0.1, representative="quadric")
    om, fm, _, cm = R.simplify(v, f, 0.1, representative="mean")
    assert (fq == fm).all() and cq["fallbacks"] == 0
    rq, rm = np.abs(np.sqrt((oq ** 2).sum(axis=1)) - 1.0).max(), np.abs(np.sqrt((om ** 2).sum(axis=1)) - 1.0).max()
    print(f"sphere: radial error quadric {rq:.4g}, mean {rm:.4g}")
    assert rq < 2e-3 and rm < 2e-3 and abs(rq - rm) < 1e-4
    # the sphere's vertices come from sin and cos, which may differ in the last place between C libraries: no bit-level comparison
    assert recorded["sphere"]["quadric_radial_error"] == pytest.approx(rq, rel=1e-6) and recorded["sphere"]["mean_radial_error"] == pytest.approx(rm, rel=1e-6)


@pytest.mark.parametrize("which", ["cube", "sphere"])
def test_jacobi_solve_agrees_with_eigh(cube, sphere, recorded, which):
    worst = 0.0
    for cell in CELLS if which == "cube" else (0.1, 0.2):
        v, f = cube if which == "cube" else sphere
        A, b, m, c = R.quadric_system(v, f, cell)
        pj, fj = R.solve_jacobi(A, b, m, c, cell)
        pe, fe = R.solve_eigh(A, b, m, c, cell)
        assert not fj.any() and not fe.any()
        worst = max(worst, float(np.abs(pj - pe).max()))
    print(f"{which}: jacobi against eigh {worst:.3g}")
    assert worst <= EIGH_BOUND
    assert 100 * recorded["jacobi_vs_eigh"][which] <= EIGH_BOUND      # the recorded measurement (LAPACK builds differ in the last places) and its margin


def test_key_range():
    top = float(2 ** 21)
    tri = R.edge_triangle
    v, f = tri(top - 0.5)                                    # k = 2^21 - 1
    ov, of, vmap, c = R.simplify(v, f, 1.0, origin=(0.0, 0.0, 0.0), representative="mean")
    assert c["clusters"] == 3 and of.tolist() == [[0, 2, 1]] and vmap.tolist() == [0, 2, 1]      # kx is the most significant field
    v, f = tri(top + 0.5)                                    # k = 2^21
    with pytest.raises(ValueError, match="2\\^21"):
        R.simplify(v, f, 1.0, origin=(0.0, 0.0, 0.0))
    v, f = tri(2.5)
    with pytest.raises(ValueError, match="2\\^21"):
        R.simplify(v, f, 1.0, origin=(1.0, 0.0, 0.0))        # k = -1 at the first vertex
    R.simplify(v, f, 1.0, origin=(0.5, 0.5, 0.5))            # k = 0 exactly


def test_empty_inputs():
    for v, f in ((np.zeros((0, 3)), np.zeros((0, 3), np.int64)), (np.ones((4, 3)), np.zeros((0, 3), np.int64))):
        ov, of, vmap, c = R.simplify(v, f, 1.0)
        assert ov.shape == (0, 3) and of.shape == (0, 3) and vmap.tolist() == [-1] * len(v) and not any(c.values())
    nan = np.full((3, 3), np.nan)
    ov, of, vmap, c = R.simplify(nan, np.array([[0, 1, 2]]), 1.0)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and vmap.tolist() == [-1, -1, -1] and not any(c.values())


def test_degenerate_faces_add_nothing_and_the_fallback_is_the_mean():
    """a cell whose only faces have no area has A = 0: no eigenpair is kept, the point is c + (mean - c), no fall-back; a quadric
    whose minimiser leaves the cell by more than a cell falls back to the mean's own bits"""
    (v, f), par = R.flat_and_parallel_meshes()
    A, b, m, c = R.quadric_system(v, f, 1.0, origin=(0.0, 0.0, 0.0))
    ov, of, vmap, cnt = R.simplify(v, f, 1.0, origin=(0.0, 0.0, 0.0))
    assert cnt["fallbacks"] == 0 and cnt["collapsed_faces"] == 1 and of.tolist() == [[0, 2, 1]]
    # two nearly parallel planes through one cell meet far outside it: rank_tol tiny keeps the weak direction, the point leaves
    v, f = par
    om, _, _, _ = R.simplify(v, f, 1.0, origin=(0.0, 0.0, 0.0), representative="mean")
    oq, _, _, cq = R.simplify(v, f, 1.0, origin=(0.0, 0.0, 0.0), representative="quadric", rank_tol=1e-12)
    fell = [i for i in range(len(oq)) if (oq[i].view(np.int64) == om[i].view(np.int64)).all()]
    assert cq["fallbacks"] == len(fell) >= 1


def test_header_binding_and_appendix_agree_on_the_export():
    import ctypes as C
    from surfd_amd import _native as N
    name = "surfd_meshsimplify_cluster"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "surfd_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, "not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    kinds = []
    for p in params:
        if "*" in p:
            kinds.append("ptr")
        else:
            kinds.append(p.rsplit(" ", 1)[0])
    assert kinds == ["ptr", "int", "ptr", "int", "ptr", "double", "int", "double", "ptr", "ptr", "ptr", "ptr", "surfd_stream"]
    res, args = N._SIGS[name]
    assert res is C.c_int and name in N.EXPORTED_SYMBOLS
    as_kind = {C.c_int: "int", C.c_double: "double"}
    got = [as_kind.get(a, "ptr") for a in args[:-1]] + ["surfd_stream"]
    assert got == kinds and args[-1] is C.c_void_p
    assert args[4] is C.POINTER(C.c_double) and args[11] is N.c_i64p
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"| `{name}` |" in doc[doc.index("## Appendix: every export"):]
    assert "SURFD_SIMPLIFY_MEAN = 0" in text and "SURFD_SIMPLIFY_QUADRIC = 1" in text
    from surfd_amd import meshsimplify
    assert meshsimplify.REPRESENTATIVES == {"mean": 0, "quadric": 1} and meshsimplify.STAT_NAMES == R.COUNT_NAMES
    if os.path.exists(N.LIB_PATH):
        assert hasattr(C.CDLL(N.LIB_PATH), name)


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from surfd_amd.meshsimplify import simplify_vertex_clustering
    from surfd_amd.meshudf import get_mesh_from_udf
    v, f = torch.zeros(3, 3, dtype=torch.float64), torch.tensor([[0, 1, 2]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        simplify_vertex_clustering(v, f, 0.1)
    with pytest.raises(ValueError, match="simplify_cells"):
        get_mesh_from_udf(None, (-1, 1), 0.1, N=16, differentiable=True, device_clean=True, simplify_cells=8)
    with pytest.raises(ValueError, match="simplify_cells"):
        get_mesh_from_udf(None, (-1, 1), 0.1, N=16, differentiable=False, device_clean=False, simplify_cells=8)
