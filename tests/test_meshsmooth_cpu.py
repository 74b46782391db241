"""tests/meshsmooth_ref.py, the sequential restatement of the contract of csrc/meshsmooth.hip, pinned
without a GPU: against surfd_amd.meshproc (equal where meshproc's own arithmetic has one order, within a measured bound where
it goes through einsum / linalg.norm) and on meshes small enough to check by hand."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshsmooth_ref as R  # noqa: E402

from surfd_amd import meshproc as mp  # noqa: E402

SHAPES = R.shapes()

# The largest |meshsmooth_ref.laplacian - meshproc.laplacian_smooth| over the well-conditioned meshes (R.WELL_CONDITIONED, 3 steps,
# cotangent weights, boundary on and off), in units of 2^-52 max |coordinate|: 4.87, on the 40 x 40 sheet with boundary=False
# (measured on the CPU; DESIGN.md section 8.14 has the table).  The tests assert 8 x that: the margin covers meshes other than
# those measured.  The bound is against meshproc and was not taken from any device result.
LAPLACIAN_MEASURED_UNITS = 4.87
LAPLACIAN_BOUND_UNITS = 8 * LAPLACIAN_MEASURED_UNITS


def laplacian_bound(vertices):
    return LAPLACIAN_BOUND_UNITS * 2.0 ** -52 * np.abs(vertices).max()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_smooth_borders_equals_meshproc(name):
    v, f = SHAPES[name]
    assert np.array_equal(R.smooth_borders(v, f), mp.smooth_borders(v, f))
    assert np.array_equal(R.smooth_borders(v, f, 0.5, 3), mp.smooth_borders(v, f, 0.5, 3))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_vertex_normals_equal_meshproc(name):
    v, f = SHAPES[name]
    unit, raw = R.vertex_normals(v, f, "angle")
    assert np.array_equal(unit, mp.vertex_normals_by_angle(v, f))
    assert np.isfinite(raw).all()


@pytest.mark.parametrize("name", R.WELL_CONDITIONED)
@pytest.mark.parametrize("boundary", [True, False])
def test_laplacian_within_the_measured_bound_of_meshproc(name, boundary):
    v, f = SHAPES[name]
    got, want = R.laplacian(v, f, 3, True, boundary), mp.laplacian_smooth(v, f, 3, True, boundary)
    err = np.abs(got - want).max()
    print(f"{name} boundary={boundary}: {err / (2.0 ** -52 * np.abs(v).max()):.3f} units")
    assert err <= laplacian_bound(v)
    assert err > 0 or name == "sheet5"                  # the einsum of meshproc does round differently: the bound is not idle


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_uniform_laplacian_equals_meshproc(name):
    """without cotangents meshproc has no einsum and no norm: one order of operations, equal bits"""
    v, f = SHAPES[name]
    for boundary in (True, False):
        assert np.array_equal(R.laplacian(v, f, 3, False, boundary), mp.laplacian_smooth(v, f, 3, False, boundary))


def test_border_count_rule():
    assert R.counts(SHAPES["empty"][1]) == (0, 0)
    assert R.counts(SHAPES["one_triangle"][1]) == (3, 3)
    assert R.counts(SHAPES["two_triangles"][1]) == (4, 4)
    assert R.counts(SHAPES["tetrahedron"][1]) == (0, 0)
    assert R.counts(SHAPES["sheet5"][1]) == (16, 16)
    assert R.counts(SHAPES["sheet40"][1]) == (156, 156)
    assert R.counts(SHAPES["fan70"][1]) == (72, 72)
    # the edge (0, 1) carries three half-edges: inner; the six others are border
    f = SHAPES["three_on_an_edge"][1]
    assert R.border_halfedges(f).tolist() == [False, True, True, False, True, True, False, True, True]
    # the face (1, 1, 3) counts: its pair (1, 1) occurs once (border), its pairs (1, 3) and (3, 1) make (1, 3) occur four times
    f = SHAPES["repeated_index"][1]
    b = R.border_halfedges(f)
    assert b[3] and not b[4] and not b[5]
    assert sorted(map(tuple, np.stack(R.border_records(f), 1).tolist())).count((1, 1)) == 2
    for name, (v, f) in SHAPES.items():
        assert np.array_equal(np.nonzero(R.border_halfedges(f))[0], np.sort(mp.border_edge_rows(f)) if len(f) else np.zeros(0, dtype=np.int64)), name


def test_one_triangle_by_hand():
    v, f = SHAPES["one_triangle"]
    # every vertex is a border vertex: (2 p + n1 + n2) / 4, added as ((p + n_out) + n_in), then p + that, then / (3 + 1)
    want = np.stack([(v[i] + ((v[i] + v[(i + 1) % 3]) + v[(i + 2) % 3])) / 4.0 for i in range(3)])
    assert np.array_equal(R.laplacian(v, f, 1, True, True), want)
    # without the border rule and without cotangents: the two neighbours, once per half-edge
    want = np.stack([(v[i] + (v[(i + 1) % 3] + v[(i + 2) % 3])) / 3.0 for i in range(3)])
    assert np.array_equal(R.laplacian(v, f, 1, False, False), want)
    # the umbrella over the border: neighbours above the vertex ascending, then those below
    order = {0: (1, 2), 1: (2, 0), 2: (0, 1)}
    want = np.stack([v[i] + 0.3 * ((v[order[i][0]] + v[order[i][1]]) / 2.0 - v[i]) for i in range(3)])
    assert np.array_equal(R.smooth_borders(v, f, 0.3, 1), want)
    # normals: one face, every corner carries its unit normal times its angle; the angles sum to pi
    unit, raw = R.vertex_normals(v, f, "angle")
    n = np.cross(v[1] - v[0], v[2] - v[0])
    assert np.allclose(unit, n / np.linalg.norm(n), atol=1e-15)
    assert abs(np.linalg.norm(raw, axis=1).sum() - np.pi) < 1e-14
    unit, raw = R.vertex_normals(v, f, "area")
    assert np.array_equal(raw, R.cross3((v[1] - v[0])[None], (v[2] - v[0])[None]).repeat(3, 0))


def test_closed_and_unreferenced_and_empty():
    v, f = SHAPES["tetrahedron"]
    assert np.array_equal(R.smooth_borders(v, f), v)                        # closed: no border, nothing moves
    assert np.array_equal(R.laplacian(v, f, 2, True, True), R.laplacian(v, f, 2, True, False))
    v, f = SHAPES["unreferenced"]
    for out in (R.laplacian(v, f), R.smooth_borders(v, f), R.taubin(v, f, 2), R.umbrella(v, f, 0.5)):
        assert np.array_equal(out[4], v[4]) and not np.array_equal(out[:4], v[:4])
    assert np.array_equal(R.vertex_normals(v, f)[0][4], np.zeros(3))
    v, f = SHAPES["empty"]
    assert np.array_equal(R.laplacian(v, f), v) and np.array_equal(R.taubin(v, f), v) and np.array_equal(R.vertex_normals(v, f)[0], np.zeros((3, 3)))


def test_zero_area_face_weighs_nothing():
    v, f = SHAPES["zero_area"]
    v0, v1, v2 = R.halfedges(f)
    w = R.cot_weights(v, v0, v1, v2)
    assert np.array_equal(w[6:9], np.zeros(3)) and (w[:6] != 0).all() and np.isfinite(w).all()
    assert np.isfinite(R.laplacian(v, f, 3, True, False)).all()
    assert np.array_equal(R.vertex_normals(v, f, "area")[1][4], R.vertex_normals(v, f[[0, 1, 3]], "area")[1][4])


def test_sweeps_are_jacobi():
    """an in-place sweep (each vertex reading the positions already moved) differs from the contract on the 40 x 40 sheet"""
    v, f = SHAPES["sheet40"]
    v0, v1, _ = R.halfedges(f)
    p = v.copy()
    for _ in range(2):
        for i in range(len(p)):
            nb = np.concatenate([v1[v0 == i], v0[v1 == i]])
            p[i] = p[i] + 0.5 * (p[nb].sum(axis=0) / len(nb) - p[i])
    assert not np.allclose(p, R.umbrella(v, f, 0.5, 0.5, 2), atol=1e-3)


def test_taubin_shrinks_less_than_the_umbrella():
    v, f = R.icosphere(2, 0.02, seed=4)
    radius = lambda p: np.sqrt((p * p).sum(axis=1)).mean()                  # noqa: E731
    assert abs(radius(R.taubin(v, f, 10)) - 1.0) < abs(radius(R.umbrella(v, f, 0.5, 0.5, 10)) - 1.0)


def test_product_module_refuses_cpu_tensors_shapes_and_dtypes():
    from surfd_amd import meshsmooth
    v, f = SHAPES["two_triangles"]
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshsmooth.MeshSmoother(tf)
    for fn in (meshsmooth.laplacian_smooth, meshsmooth.smooth_borders, meshsmooth.taubin_smooth, meshsmooth.vertex_normals_by_angle):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(tv, tf)
        with pytest.raises(ValueError):
            fn(tv[:, :2], tf)
        with pytest.raises(ValueError):
            fn(tv, tf[:, :2])
        with pytest.raises(TypeError):
            fn(tv.half(), tf)
        with pytest.raises(TypeError):
            fn(tv, tf.float())
