"""The restatement tests/meshfill_ref.py against what defines it: exhaustive enumeration of all triangulations, the counts and
incidences a cap must have, hand-worked rows, and the meshes on which loops stay open.  No GPU: tests/test_gpu_meshfill.py pins
the device to the restatement."""
import math

import numpy as np
import pytest

import meshfill_ref as R
import meshtopo_ref as T
from meshclean_ref import fill_small_holes


def _caps(v, f, **kw):
    out, loop, st = R.fill_holes(v, f, **kw)
    assert (out[:len(f)] == f).all() and len(out) - len(f) == st["caps"] == len(loop)
    return out[len(f):], loop, st


@pytest.mark.parametrize("n", range(3, 10))
def test_dp_total_equals_exhaustive_enumeration(n):
    rng = np.random.default_rng(n)
    for _ in range(3):
        P = rng.standard_normal((n, 3))
        total, rows = R.triangulate(P)
        best = R.best_total_exhaustive(P)
        assert abs(total - best) <= 1e-12 * best
        assert len(rows) == n - 2
        assert abs(sum(R.area(P[i], P[k], P[j]) for i, k, j in rows) - total) <= 1e-12 * total


@pytest.mark.parametrize("n", [3, 4, 5, 8, 17, 33, 64])
def test_spans_at_once_equal_the_plain_loops(n):
    rng = np.random.default_rng(100 + n)
    P = rng.standard_normal((n, 3))
    assert R.triangulate_spans(P) == R.triangulate(P)
    Q = P.copy()
    Q[n // 2] = np.nan
    assert R.triangulate_spans(Q)[1] == R.triangulate(Q)[1]
    Q = P.copy()
    Q[0, 0], Q[n - 1, 1] = 1e200, np.inf
    assert R.triangulate_spans(Q)[1] == R.triangulate(Q)[1]
    Z = np.round(P)                                          # small integers: many exact ties
    assert R.triangulate_spans(Z) == R.triangulate(Z)


@pytest.mark.parametrize("n", [3, 4, 7, 32, 33, 100])
def test_every_loop_edge_is_matched_once_against_the_border(n):
    v, f = R.ring(n, seed=n, rotate=n // 3)
    caps, loop, st = _caps(v, f, max_edges=128)
    assert len(caps) == n - 2 and st["loops_filled"] == 1 and st["longest_filled"] == n and (loop == 0).all()
    border = {(int(t[c]), int(t[(c + 1) % 3])) for t in f for c in range(3)} - {(int(t[(c + 1) % 3]), int(t[c])) for t in f for c in range(3)}
    assert len(border) == n
    cap_half = [(int(t[c]), int(t[(c + 1) % 3])) for t in caps for c in range(3)]
    for u, w in border:
        assert cap_half.count((w, u)) == 1 and cap_half.count((u, w)) == 0
    s = T.summary(T.build(np.vstack([f, caps]), len(v)))
    assert s["closed"] and s["consistently_oriented"] and s["euler_characteristic"] == 2


def test_preorder_on_a_hand_worked_hexagon():
    """even corners low, odd corners high: the three ears (0,1,2), (2,3,4), (4,5,0) and the middle (0,2,4) are the least area.  The
    recursion meets them as (0,4,5) [root: the triangle on the chord 0-5], then everything of (0,4): (0,2,4), its left (0,1,2), its
    right (2,3,4); (4,5) has nothing.  The right child of (0,2,4) at slot 1 lies at 1 + 1 + (2 - 0 - 1) = 3."""
    P = [[0, 0, 0], [2, -1, 3], [4, 0, 0], [5, 2, 3], [2, 3, 0], [-1, 2, 3]]
    total, rows = R.triangulate(P)
    assert rows == [(0, 4, 5), (0, 2, 4), (0, 1, 2), (2, 3, 4)]
    assert total == R.best_total_exhaustive(P)


def test_ties_go_to_the_smaller_k():
    """flat and convex: every triangulation has the same area in exact arithmetic, so k = i + 1 wins everywhere: a fan at the last
    vertex of the reversed listing"""
    v, f = R.flat_hexagon()
    caps, _, _ = _caps(v, f)
    assert caps.tolist() == [[0, 5, 1], [5, 4, 1], [4, 3, 1], [3, 2, 1]]             # r = 0 5 4 3 2 1
    v, f = R.flat_grid_hole()                                 # integer coordinates: every area is exact
    caps, loop, st = _caps(v, f)
    outer = [0, 6, 12, 18, 24, 30, 31, 32, 33, 34, 35, 29, 23, 17, 11, 5, 4, 3, 2, 1]           # r of the outer border, from vertex 0
    inner = [7, 8, 9, 10, 16, 22, 28, 27, 26, 25, 19, 13]                                        # r of the hole, from vertex 7
    want = [[r[i], r[i + 1], r[-1]] for r in (outer, inner) for i in range(len(r) - 2)]
    assert caps.tolist() == want and loop.tolist() == [0] * 18 + [1] * 10
    assert st == {"loops_filled": 2, "caps": 28, "loops_too_long": 0, "loops_nonfinite": 0, "irregular_border_edges": 0, "border_edges": 32,
                  "longest_filled": 20}


def test_three_and_four_edges_against_fill_small_holes():
    for n in (3, 4):
        v, f = R.ring(n, seed=2)
        caps, _, _ = _caps(v, f)
        small = fill_small_holes(v, f)[len(f):]
        assert len(caps) == len(small) == n - 2
        if n == 3:                                           # a rotation of the same cap
            c, s = caps[0].tolist(), small[0].tolist()
            assert any(c == s[r:] + s[:r] for r in range(3))
        else:                                                # the same quad, whichever diagonal: both close the mesh with its orientation
            for got in (caps, small):
                s = T.summary(T.build(np.vstack([f, got]), len(v)))
                assert s["closed"] and s["consistently_oriented"]


def test_punched_icosphere_closes():
    v, f, stars = R.punched_icosphere()
    assert stars == 42 and set(R.hole_sizes(f)) == {5, 6}
    out, loop, st = R.fill_holes(v, f)
    assert st["loops_filled"] == stars and st["irregular_border_edges"] == 0 and st["caps"] == st["border_edges"] - 2 * stars
    s = T.summary(T.build(out, len(v)))
    assert s["closed"] and s["edge_manifold"] and s["euler_characteristic"] == 2 and s["consistently_oriented"]


def test_bow_tie_stays_open():
    """two faces of an octahedron that share only vertex 4 go: their borders touch there, out(4) = in(4) = 2"""
    from meshclean_ref import _OCTA_F, _OCTA_V
    v = np.array(_OCTA_V, dtype=np.float64)
    f = np.array([t for n, t in enumerate(_OCTA_F) if n not in (0, 2)], dtype=np.int64)
    caps, _, st = _caps(v, f)
    assert len(caps) == 0 and st["loops_filled"] == 0 and st["border_edges"] == 6 and st["irregular_border_edges"] == 6


def test_misoriented_face_on_a_border_stays_open():
    v, f = R.ring(8, seed=3)
    g = f.copy()
    g[2] = g[2][[1, 0, 2]]                                   # its border half-edge now runs against its neighbours'
    caps, _, st = _caps(v, g)
    assert len(caps) == 0 and st["loops_filled"] == 0 and st["irregular_border_edges"] == st["border_edges"] > 0


def test_nan_vertex_on_a_loop():
    v, f = R.ring(9, seed=4)
    v[5, 1] = math.nan
    caps, _, st = _caps(v, f)
    assert len(caps) == 0 and st["loops_nonfinite"] == 1 and st["loops_filled"] == 0 and st["longest_filled"] == 0
    v, f = R.ring(9, seed=4)
    v[:9] *= 1e200                                           # finite vertices, areas that overflow
    assert _caps(v, f)[2]["loops_nonfinite"] == 1


def test_loop_longer_than_max_edges_stays_open():
    v, f = R.ring(13, seed=5)
    caps, _, st = _caps(v, f, max_edges=12)
    assert len(caps) == 0 and st["loops_too_long"] == 1 and st["irregular_border_edges"] == 0
    assert _caps(v, f, max_edges=13)[2]["loops_filled"] == 1
    for bad in (2, 1025):
        with pytest.raises(ValueError):
            R.fill_holes(v, f, max_edges=bad)


def test_sheet_has_every_kind_of_border():
    v, f = R.bumped_sheet()
    sizes = R.hole_sizes(f)
    assert sizes[-3:] == [36, 48, 160] and sizes[0] == 3 and any(4 < s <= 32 for s in sizes)
    _, loop, st = _caps(v, f, max_edges=128)
    assert st["loops_too_long"] == 1 and st["irregular_border_edges"] == 112 and st["longest_filled"] == 48
    assert (np.diff(loop) >= 0).all()                        # caps in ascending loop number
    assert _caps(v, f, max_edges=1024)[2]["longest_filled"] == 160
