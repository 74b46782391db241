"""tests/meshclean_ref.py (the order-free restatement that csrc/meshclean.hip builds) against
surfd_amd.meshproc on the CPU, bit for bit and in the same order; and the fixtures against the paths they are there to take,
checked on meshproc itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshclean_ref as R  # noqa: E402

from surfd_amd import meshproc as mp  # noqa: E402

SHAPES = R.shapes()
NAMES = sorted(SHAPES)


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.float64:
        assert np.array_equal(got.view(np.int64), want.view(np.int64))          # the bits: -0.0 is not 0.0 here
    else:
        assert np.array_equal(got, want)


def check_all(v, f):
    """every function of the restatement against meshproc on one mesh, each step on meshproc's own intermediate result"""
    v1, f1 = mp.cull_and_merge(v, f)
    g1 = R.cull_and_merge(v, f)
    same(g1[0], v1); same(g1[1], f1)
    f2 = mp.drop_duplicate_faces(f1)
    same(R.drop_duplicate_faces(f1), f2)
    same(R.drop_duplicate_faces(f), mp.drop_duplicate_faces(f))
    with np.errstate(all="ignore"):
        f3 = mp.drop_degenerate_faces(v1, f2)
        raw = mp.drop_degenerate_faces(v, f)                 # the raw mesh too: NaN and Inf coordinates, repeated indices
    same(R.drop_degenerate_faces(v1, f2), f3)
    same(R.drop_degenerate_faces(v, f), raw)
    same(R.fill_small_holes(v1, f3), mp.fill_small_holes(v1, f3))
    same(R.fill_small_holes(v, f), mp.fill_small_holes(v, f))
    with np.errstate(all="ignore"):
        want = mp.clean_until_stable(v, f)
    got = R.clean_until_stable(v, f)
    same(got[0], want[0]); same(got[1], want[1])
    return got[2]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_meshproc(name):
    check_all(*SHAPES[name])


def test_restatement_equals_meshproc_on_random_soups():
    rng = np.random.default_rng(7)
    capped = merged = 0
    for _ in range(1500):
        st = check_all(*R.random_soup(rng))
        capped += st["caps3"] + st["caps4"] > 0
        merged += st["merged_vertices"] > 0
    assert capped > 20 and merged > 100, (capped, merged)


def test_degenerate_arithmetic_on_random_triangles():
    """the operation order of the height test, on triangles of every scale down to the thresholds"""
    rng = np.random.default_rng(11)
    v = rng.standard_normal((3000, 3)) * 10.0 ** rng.integers(-9, 3, size=(3000, 1))
    f = rng.integers(0, len(v), size=(4000, 3))
    thin = np.arange(0, 3000 - 3, 3)                          # slivers: the third corner almost on the line of the other two
    v[thin + 2] = v[thin] + (v[thin + 1] - v[thin]) * rng.random((len(thin), 1)) + rng.standard_normal((len(thin), 3)) * 1e-8
    f = np.vstack([f, np.stack([thin, thin + 1, thin + 2], axis=1)])
    want = mp.drop_degenerate_faces(v, f)
    assert 0 < len(want) < len(f)
    same(R.drop_degenerate_faces(v, f), want)


def test_duplicate_order_across_the_packing_boundary():
    """_pack_rows changes its method where an index reaches 2^20 - 1 (three 21-bit fields); the order must not"""
    for top in (2 ** 20 - 3, 2 ** 20 - 2, 2 ** 20 - 1, 2 ** 20, 2 ** 21 - 1, 2 ** 21 + 5):
        f = np.array([[top, 3, 7], [7, top, 3], [2, top - 1, top], [top, top - 1, 2], [0, 1, 2], [top - 1, 5, 6], [5, 6, top - 1], [1, 0, 2]], dtype=np.int64)
        same(R.drop_duplicate_faces(f), mp.drop_duplicate_faces(f))


def test_key_range_is_refused():
    v, f = SHAPES["tetrahedron"]
    v = v.copy(); v[1, 0] = 2.0 ** 62 / 1e8
    with pytest.raises(ValueError):
        R.cull_and_merge(v, f)
    v[1, 0] = np.nextafter(2.0 ** 62 / 1e8, 0) / 2
    R.cull_and_merge(v, f)


# ---- the fixtures take the paths they are there for, on meshproc itself -----------------------------------------------------------
def _sequence(name):
    """meshproc's own first pass on a fixture: (v, f0 after the cull, f after the duplicate pass, after the height test, after the caps)"""
    v, f = SHAPES[name]
    v1, f0 = mp.cull_and_merge(v, f)
    fd = mp.drop_duplicate_faces(f0)
    fg = mp.drop_degenerate_faces(v1, fd)
    return v1, f0, fd, fg, mp.fill_small_holes(v1, fg)


def _fast_return(name):
    _, f0, fd, fg, fh = _sequence(name)
    return len(f0) == len(fd) == len(fg) == len(fh)


def _meshproc_rounds(name):
    """the duplicate / degenerate passes meshproc.clean_until_stable runs, the first included: its calls of drop_duplicate_faces"""
    calls, inner = [0], mp.drop_duplicate_faces

    def counting(faces):
        calls[0] += 1
        return inner(faces)
    mp.drop_duplicate_faces = counting
    try:
        mp.clean_until_stable(*SHAPES[name])
    finally:
        mp.drop_duplicate_faces = inner
    return calls[0]


def test_fixtures_cover_every_path():
    assert _fast_return("tetrahedron") and _meshproc_rounds("tetrahedron") == 1
    _, _, _, fg, fh = _sequence("octahedron_minus_one")
    assert len(fh) == len(fg) + 1                                             # a 3-cap
    _, _, _, fg, fh = _sequence("cube_minus_quad")
    assert len(fh) == len(fg) + 2                                             # a 4-cap
    for name in ("pentagon_hole", "octahedron_minus_two"):                    # holes left open
        _, _, _, fg, fh = _sequence(name)
        assert len(fh) == len(fg) and len(mp.border_edge_rows(fg)) >= 5
    _, _, _, fg, _ = _sequence("octahedron_minus_two")
    edges = mp.edges_of_faces(fg)[0][mp.border_edge_rows(fg)]
    assert np.bincount(edges[:, 0]).max() == 2                                # a vertex that two border half-edges leave
    assert _meshproc_rounds("tetrahedron_and_triangle") >= 2 and _meshproc_rounds("tetrahedron_and_two_triangles") >= 2
    # soup: a merged pair, a tie in each direction, a duplicate and a degenerate face removed, a NaN vertex, an unreferenced one
    v, f = SHAPES["soup"]
    v1, f0, fd, fg, _ = _sequence("soup")
    finite = np.isfinite(v).all(axis=1)
    referenced = np.zeros(len(v), dtype=bool); referenced[f[finite[f].all(axis=1)]] = True
    assert (~finite).sum() == 1 and len(f0) == len(f) - 1 and (finite & ~referenced).sum() == 1
    assert len(v1) < (referenced & finite).sum()
    x = v[finite, 0] * 1e8
    ties = x[(x - np.floor(x) == 0.5)]
    assert (np.round(ties) < ties).any() and (np.round(ties) > ties).any()
    assert (v[finite] == 0).all(axis=1).sum() == 2 and np.signbit(v[finite]).any()          # -0.0 against 0.0
    assert len(fd) < len(f0) and len(fg) < len(fd)
    st = R.clean_until_stable(v, f)[2]
    assert st["merged_vertices"] >= 4 and st["duplicate_faces"] >= 2 and st["degenerate_faces"] >= 2 and st["rounds"] == _meshproc_rounds("soup") >= 2
    # sheet64: many of every kind
    v, f = SHAPES["sheet64"]
    st = R.clean_until_stable(v, f)[2]
    assert 7500 < len(f) < 8000 and st["caps3"] > 50 and st["caps4"] > 5, (len(f), st)
