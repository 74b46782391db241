"""tests/meshtopo_ref.py, the sequential restatement of the mesh-topology contract, pinned without a GPU:
hand-checkable meshes, the three marching-cubes fixtures against numbers obtained independently (scipy's connected_components
on the face arrays, recorded in the table of DESIGN.md section 8.12 and taken here as given), its keep_components_with_at_least
against meshproc's, and the product module's refusal of CPU tensors."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshtopo_ref as mt  # noqa: E402
import raycast_ref as rr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_marching_cubes.npz")

# mesh: F, V, E, chi, border, non-manifold, components (vertex, edge, manifold), border loops, same-direction manifold edges
FIXTURE_TABLE = {
    "two_spheres_48": (7424, 3686, 11136, -26, 0, 0, (1, 1, 1), 0, 0),
    "open_sheet_48": (2414, 1288, 3701, 1, 160, 0, (1, 1, 1), 1, 0),
    "noisy_blob_48": (21851, 11430, 33260, 21, 967, 0, (19, 19, 19), 15, 0),
}


def fixture_mesh(name):
    z = np.load(GOLDEN, allow_pickle=False)
    return z[name + "_verts"], z[name + "_faces"].astype(np.int64)


def test_one_triangle():
    topo = mt.build([[0, 1, 2]])
    assert topo["edges"].tolist() == [[0, 1], [0, 2], [1, 2]]
    assert topo["valence"].tolist() == [1, 1, 1]
    assert topo["edge_halfedges"].tolist() == [0, 2, 1]                 # 0 -> 1, 2 -> 0, 1 -> 2
    assert topo["face_edges"].tolist() == [[0, 2, 1]]
    assert topo["face_neighbors"].tolist() == [[-1, -1, -1]]
    s = mt.summary(topo)
    assert (s["euler_characteristic"], s["border_loops"], s["largest_border_loop"], s["closed"], s["consistently_oriented"]) == (1, 1, 3, False, True)
    assert s["patches"] == [{"faces": 1, "closed": False, "orientable": True, "genus": None}]


def test_empty():
    topo = mt.build(np.zeros((0, 3), dtype=np.int64))
    assert topo["E"] == 0 and topo["edge_offsets"].tolist() == [0]
    s = mt.summary(topo)
    assert s["faces"] == 0 and s["components_vertex"] == 0 and s["closed"] and s["patches"] == []


def test_tetrahedron_and_octahedron():
    tet = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    for f, (V, E) in ((tet, (4, 6)), (rr.octahedron()[1], (6, 12))):
        s = mt.summary(mt.build(f))
        assert (s["referenced_vertices"], s["edges"], s["manifold_edges"], s["euler_characteristic"]) == (V, E, E, 2)
        assert s["closed"] and s["edge_manifold"] and s["consistently_oriented"]
        assert s["patches"] == [{"faces": len(f), "closed": True, "orientable": True, "genus": 0}]
    assert mt.build(tet)["face_neighbors"].tolist() == [[3, 2, 1], [0, 2, 3], [0, 3, 1], [0, 1, 2]]


def test_cube_and_flipped_cube():
    v, f = rr.cube()
    topo = mt.build(f)
    assert topo["E"] == 18 and (topo["valence"] == 2).all()
    assert not mt.orientation(topo)[0].any()
    vf, ff = rr.cube_flipped()
    flip, po = mt.orientation(mt.build(ff))
    turned = np.zeros(12, dtype=bool)
    turned[::2] = True
    assert po.all() and np.array_equal(flip, turned ^ turned[0])        # relative to face 0, which keeps its winding
    assert mt.same_direction_manifold_edges(ff) > 0 and mt.same_direction_manifold_edges(mt.oriented(ff, flip)) == 0
    # outward: face 0 of cube_flipped is turned, so the consistent mesh is inside out and everything is turned once more
    flip_out, _ = mt.orientation(mt.build(ff), vf)
    assert np.array_equal(flip_out, turned)
    assert np.array_equal(mt.oriented(ff, flip_out), f)


def test_two_cubes():
    v, f = mt.two_cubes("edge")
    topo = mt.build(f)
    assert len(v) == 14 and sorted(topo["valence"].tolist())[-2:] == [2, 4]
    s = mt.summary(topo)
    assert (s["components_vertex"], s["components_edge"], s["components_manifold"], s["non_manifold_edges"]) == (1, 1, 2, 1)
    assert not s["closed"] and not s["edge_manifold"] and (topo["face_neighbors"] == -2).sum() == 4
    assert [p["closed"] for p in s["patches"]] == [False, False]          # a patch with a valence-4 edge is not closed
    v, f = mt.two_cubes("vertex")
    s = mt.summary(mt.build(f))
    assert len(v) == 15 and (s["components_vertex"], s["components_edge"], s["components_manifold"]) == (1, 2, 2)
    assert s["closed"] and [p["genus"] for p in s["patches"]] == [0, 0]
    assert mt.components(mt.build(f), "edge")[0].tolist() == [0] * 12 + [1] * 12


def test_duplicated_and_degenerate_faces():
    topo = mt.build([[0, 1, 2], [0, 1, 2]])
    assert topo["valence"].tolist() == [2, 2, 2] and topo["face_neighbors"].tolist() == [[1, 1, 1], [0, 0, 0]]
    flip, po = mt.orientation(topo)
    assert po.all() and flip.tolist() == [False, True]                   # the copy runs the same way along all three edges
    topo = mt.build([[0, 1, 2], [2, 2, 3], [2, 1, 3]], 4)
    assert topo["degenerate"].tolist() == [False, True, False]
    assert topo["face_edges"][1].tolist() == [-1, -1, -1] and topo["face_neighbors"][1].tolist() == [-1, -1, -1]
    assert topo["edge_halfedges"].tolist() == [0, 2, 1, 6, 7, 8]
    for c in ("vertex", "edge", "manifold"):
        labels, sizes = mt.components(topo, c)
        assert labels.tolist() == [0, -1, 0] and sizes.tolist() == [2]
    s = mt.summary(topo)
    assert s["degenerate_faces"] == 1 and not s["closed"] and s["euler_characteristic"] == 4 - 5 + 2


def test_moebius_band_and_annulus():
    v, f = mt.band(16, twist=True)
    topo = mt.build(f)
    flip, po = mt.orientation(topo)
    assert po.tolist() == [False] and not flip.any()
    labels, sizes, simple = mt.border_loops(topo)
    assert sizes.tolist() == [32] and simple.tolist() == [True] and labels.tolist() == [0] * 32
    assert mt.summary(topo)["euler_characteristic"] == 0 and not mt.summary(topo)["orientable"]
    v, f = mt.band(16, twist=False)
    topo = mt.build(f)
    flip, po = mt.orientation(topo)
    assert po.tolist() == [True] and not flip.any()
    assert mt.border_loops(topo)[1].tolist() == [16, 16]
    ft, perm, turned = mt.turned_and_shuffled(f, 0.4, seed=3)
    flip, po = mt.orientation(mt.build(ft))
    assert po.all() and np.array_equal(flip, turned ^ turned[0])


def test_bow_tie_border_loop_is_not_simple():
    topo = mt.build([[0, 1, 2], [0, 3, 4]])
    labels, sizes, simple = mt.border_loops(topo)
    assert sizes.tolist() == [6] and simple.tolist() == [False]


def test_torus_and_strip():
    v, f = rr.torus()
    s = mt.summary(mt.build(f))
    assert s["closed"] and s["euler_characteristic"] == 0 and s["patches"][0]["genus"] == 1 and s["consistently_oriented"]
    v, f = mt.strip(2001)
    topo = mt.build(f)
    assert mt.border_loops(topo)[1].tolist() == [2003] and not mt.orientation(topo)[0].any()
    ft, perm, turned = mt.turned_and_shuffled(f, 0.4, seed=1)
    flip, po = mt.orientation(mt.build(ft))
    assert po.all() and np.array_equal(flip, turned ^ turned[0])
    assert mt.same_direction_manifold_edges(mt.oriented(ft, flip)) == 0


def test_outward_and_volume_terms():
    v, f = rr.icosphere(3)
    inverted = f[:, [0, 2, 1]]
    terms = mt.signed_volume_terms(v, f)
    sphere6 = 6 * 4 / 3 * np.pi * 0.75 ** 3           # M = 1: the sum is 6 x the volume in units of 2^-30; the inscribed polyhedron
    assert 0.98 * sphere6 < sum(terms) / 2.0 ** 30 < sphere6      # lacks the caps over its 1 280 faces (sagitta / radius about 0.4 %)
    assert sum(mt.signed_volume_terms(v, inverted)) == -sum(terms)
    assert mt.orientation(mt.build(inverted), v)[0].all() and not mt.orientation(mt.build(f), v)[0].any()
    sv, sf = fixture_mesh("open_sheet_48")
    assert not mt.orientation(mt.build(sf), sv)[0].any()                           # an open patch is left alone


def test_weld():
    v, f = rr.icosphere(1)
    ev, ef = mt.exploded(v, f)
    wv, wf, vmap = mt.weld(ev, ef)
    assert len(wv) == len(v) and mt.summary(mt.build(wf))["closed"]
    assert np.array_equal(wv[wf], v[f])
    pts = np.array([[0.0, 1, 2], [-0.0, 1, 2], [np.nan, 0, 0], [np.nan, 0, 0], [5, 5, 5], [0, 1, 2]], dtype=np.float32)
    wv, wf, vmap = mt.weld(pts, [[0, 1, 4], [2, 3, 5]])
    assert vmap.tolist() == [0, 0, 1, 2, 3, 0] and len(wv) == 4 and wf.tolist() == [[0, 0, 3], [1, 2, 0]]


@pytest.mark.parametrize("name", sorted(FIXTURE_TABLE))
def test_fixtures_reproduce_the_table(name):
    F, V, E, chi, border, nonmanifold, comps, loops, same_dir = FIXTURE_TABLE[name]
    v, f = fixture_mesh(name)
    s = mt.summary(mt.build(f, len(v)))
    assert (s["faces"], s["referenced_vertices"], s["edges"], s["euler_characteristic"]) == (F, V, E, chi)
    assert (s["border_edges"], s["non_manifold_edges"]) == (border, nonmanifold)
    assert (s["components_vertex"], s["components_edge"], s["components_manifold"]) == comps
    assert s["border_loops"] == loops and s["degenerate_faces"] == 0
    assert mt.same_direction_manifold_edges(f) == same_dir
    assert s["consistently_oriented"]                                               # the mesher's raw output needs no flip


def test_keep_components_matches_meshproc():
    from surfd_amd import meshproc
    v, f = fixture_mesh("noisy_blob_48")
    sizes = mt.components(mt.build(f, len(v)), "vertex")[1]
    assert len(sizes) == 19
    min_faces = int(np.sort(sizes)[len(sizes) // 2])                                # some go, some stay
    assert 0 < (sizes < min_faces).sum() < len(sizes)
    kv, kf = mt.keep_components_with_at_least(v, f, min_faces)
    pv, pf = meshproc.keep_components_with_at_least(v, f, min_faces)
    assert np.array_equal(kf, pf) and np.array_equal(kv.astype(np.float64), pv)
    labels = mt.components(mt.build(f, len(v)), "vertex")[0]
    ours, theirs = labels, meshproc.face_components(f, len(v))
    assert len(np.unique(np.stack([ours, theirs], 1), axis=0)) == 19                 # the same partition


def test_product_module_refuses_cpu_tensors():
    from surfd_amd import meshtopo
    v, f = rr.cube()
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshtopo.MeshTopology(tf)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshtopo.weld_vertices(tv, tf)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshtopo.orient_faces(tv, tf)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshtopo.keep_components_with_at_least(tv, tf, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshtopo.is_closed(tf)
    with pytest.raises(ValueError):
        meshtopo.MeshTopology(tf[:, :2])
    with pytest.raises(TypeError):
        meshtopo.MeshTopology(tf.float())
