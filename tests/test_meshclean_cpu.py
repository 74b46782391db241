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


# ---- the meshes at size and the families: restatement == meshproc, and each takes the path it is there for ----------------------
BIG = R.big_shapes()


def _rounds_of(v, f):
    """as _meshproc_rounds, of any mesh"""
    calls, inner = [0], mp.drop_duplicate_faces

    def counting(faces):
        calls[0] += 1
        return inner(faces)
    mp.drop_duplicate_faces = counting
    try:
        with np.errstate(all="ignore"):
            mp.clean_until_stable(v, f)
    finally:
        mp.drop_duplicate_faces = inner
    return calls[0]


def _classes(v, f):
    """(size, span) per class of meshproc's keys over the vertices that take part: members, highest - lowest index"""
    finite = np.isfinite(v).all(axis=1)
    part = np.zeros(len(v), dtype=bool)
    part[f[finite[f].all(axis=1)]] = True
    idx = np.nonzero(part)[0]
    _, inv = np.unique(np.round(v[idx] * (1.0 / mp.MERGE_TOL)).astype(np.int64), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    lo, hi = np.full(inv.max() + 1, len(v)), np.full(inv.max() + 1, -1)
    np.minimum.at(lo, inv, idx); np.maximum.at(hi, inv, idx)
    return np.bincount(inv), hi - lo


@pytest.mark.parametrize("name", sorted(BIG))
def test_restatement_equals_meshproc_at_size(name):
    check_all(*BIG[name])


def test_torus_soup_takes_its_path():
    v, f = BIG["torus_soup"]
    assert v.shape == (3 * R.TORUS_FACES, 3) and f.shape == (R.TORUS_FACES, 3)
    st = R.new_stats()
    gv, gf = R.cull_and_merge(v, f, stats=st)
    wv, wf = mp.cull_and_merge(v, f)
    negative = float((np.round(v * 1e8) < 0).mean())
    size, span = _classes(v, f)
    print(f"\ntorus_soup: V {len(v)} F {len(f)} -> V {len(wv)} F {len(wf)}, merged {st['merged_vertices']}, negative keys {negative:.3f}, "
          f"largest class {size.max()}, median class span {int(np.median(span))}, rounds {_rounds_of(v, f)}")
    assert st["merged_vertices"] == 3 * len(f) - R.TORUS_VERTICES and st["nonfinite_vertices"] == 0 and st["unreferenced_vertices"] == 0
    assert wv.shape == gv.shape == (R.TORUS_VERTICES, 3) and wf.shape == gf.shape == (R.TORUS_FACES, 3)
    assert negative >= 0.6 and np.median(span) > 10000 and size.max() >= 6
    cv, cf = mp.clean_until_stable(v, f)
    assert cv.shape == wv.shape and cf.shape == wf.shape


def test_jittered_soup_takes_its_path():
    v, f = BIG["torus_soup_jitter"]
    gv, gf, st = R.clean_until_stable(v, f)
    rounds = _rounds_of(v, f)
    print(f"\ntorus_soup_jitter: V {len(v)} F {len(f)} -> V {len(gv)} F {len(gf)}, first cull leaves {len(mp.cull_and_merge(v, f)[0])} vertices, {st}")
    assert st["duplicate_faces"] >= 100 and st["caps3"] >= 100 and st["caps4"] >= 1 and st["rounds"] == rounds >= 2


def test_fan_takes_its_path():
    v, f = BIG["fan"]
    st = R.new_stats()
    R.cull_and_merge(v, f, stats=st)
    wv, wf = mp.cull_and_merge(v, f)
    size, span = _classes(v, f)
    print(f"\nfan: V {len(v)} F {len(f)} -> V {len(wv)} F {len(wf)}, {st}, largest class {size.max()} spanning {span[np.argmax(size)]}, classes of two {int((size == 2).sum())}")
    assert len(v) == 15000 + R.FAN_EXTRA + R.FAN_NAN and len(f) == 5000 + R.FAN_NAN_FACES
    assert size.max() == 5000 and (size == 5000).sum() == 1 and (size == 2).sum() == 5000 and len(size) == 5001 and span[np.argmax(size)] > 15000
    assert st["nonfinite_vertices"] == R.FAN_NAN and st["unreferenced_vertices"] == R.FAN_EXTRA and st["merged_vertices"] == 15000 - 5001
    assert len(f) - len(wf) == R.FAN_NAN_FACES and len(wv) == 5001
    # the keys of x have both signs, and a vertex that takes no part coincides with the class of the lowest x and has the highest
    # label of those that take no part
    finite = np.isfinite(v).all(axis=1)
    part = np.zeros(len(v), dtype=bool); part[f[finite[f].all(axis=1)]] = True
    x = np.round(v[part, 0] * 1e8)
    assert (x < 0).any() and (x > 0).any()
    last = np.nonzero(~part)[0].max()
    lowest = np.nonzero(part)[0][np.argmin(v[part, 0])]
    assert finite[last] and np.array_equal(v[last], v[lowest])


def test_doubled_sheet_takes_its_path():
    v, f = BIG["doubled_sheet"]
    sheet_f = R.sheet(64)[1]
    want = mp.drop_duplicate_faces(f)
    print(f"\ndoubled_sheet: V {len(v)} F {len(f)} -> {len(want)} faces, {len(f) - len(want)} duplicates removed")
    assert len(f) - len(want) > len(f) / 2 and len(want) == len(sheet_f)
    key = lambda t: sorted(map(tuple, np.sort(t, axis=1).tolist()))      # noqa: E731
    assert key(want) == key(sheet_f)
    twice = np.unique(np.sort(f, axis=1), axis=0, return_counts=True)[1]
    assert set(twice.tolist()) == {2, 3}


def test_relabellings_take_every_rotation():
    seen = {}
    for name, seed, v, f in R.relabellings():
        seen.setdefault(name, set()).add(R.loop_pattern(f))
        check_all(v, f)
    print(f"\nrelabellings: {({k: sorted(s) for k, s in seen.items()})}")
    assert len(seen["cube_minus_quad"]) == 6 and len(seen["octahedron_minus_one"]) == 2
    meshes = [(v, f) for _, _, v, f in R.relabellings()]
    for seed in (None, 0):
        v, f = R.side_by_side(meshes, seed)
        st = check_all(v, f)
        assert st["caps3"] == 16 and st["caps4"] == 64 and st["merged_vertices"] == 0, st


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("V", R.PAD_SIZES)
@pytest.mark.parametrize("name", R.PAD_NAMES)
def test_padded_solids_give_the_solid_s_caps(name, V, split):
    v0, f0 = SHAPES[name]
    v, f, new = R.padded(name, V, split=split)
    loop = R.loop_vertices(f0)
    assert len(v) == V and sorted(new[loop].tolist()) == list(range(V - len(loop), V)) and len(set(new.tolist())) == len(new)
    assert not v[np.setdiff1d(np.arange(V), new)].any()
    want = mp.fill_small_holes(v, f)
    caps = mp.fill_small_holes(v0, f0)[len(f0):]
    same(want, np.vstack([f, new[caps]]))
    assert len(caps) == (1 if name == "octahedron_minus_one" else 2) and sorted(map(sorted, f.tolist())) == sorted(map(sorted, new[f0].tolist()))
    same(R.fill_small_holes(v, f), want)
    cv, cf = mp.clean_until_stable(v, f)
    gv, gf, _ = R.clean_until_stable(v, f)
    same(gv, cv); same(gf, cf)
    assert len(cv) == len(v0)
    if split:                                                # two edges whose sort keys differ in the highest bit alone
        bits = 1
        while (1 << bits) < V:
            bits += 1
        e = {(max(a, b), min(a, b)) for t in f.tolist() for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
        assert (V - 1 == 1 << (bits - 1)) or any((hi - (1 << (bits - 1)), lo) in e for hi, lo in e)
    v, f, new = R.padded(name, V, top=False)
    same(mp.fill_small_holes(v, f), new[mp.fill_small_holes(v0, f0)])


def test_first_400_soups_take_every_path():
    n = dict.fromkeys(("cap", "merge", "duplicate", "flat", "nonfinite", "rounds>1"), 0)
    for v, f in R.first_soups(400):
        st = R.clean_until_stable(v, f)[2]
        n["cap"] += st["caps3"] + st["caps4"] > 0
        n["merge"] += st["merged_vertices"] > 0
        n["duplicate"] += st["duplicate_faces"] > 0
        n["flat"] += st["degenerate_faces"] > 0
        n["nonfinite"] += st["nonfinite_vertices"] > 0
        n["rounds>1"] += st["rounds"] > 1
    print(f"\nfirst 400 soups of seed 7: {n}")
    assert n["cap"] >= 15 and n["merge"] >= 40 and n["duplicate"] >= 150 and n["flat"] >= 150 and n["nonfinite"] >= 50, n
    rng = np.random.default_rng(7)
    for v, f in R.first_soups(3):                            # the soups of the 1 500-soup test above, in its order
        w, g = R.random_soup(rng)
        same(v, w); same(f, g)
