"""The pair contract of the mesh intersection tests on the CPU: a zoo of hand-written ties on the numpy
restatement tests/meshintersect_ref.py, the restatement against its second form in Python integers, against an independent
ray-casting yardstick, the numbers of the issue's table, lattice_for, and the drivers' argument errors.  No GPU."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshintersect_ref as mr  # noqa: E402
import raycast_ref as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE = ((0, 0, 0), (8, 0, 0), (0, 8, 0))             # the zoo's triangle A unless stated: the half square below x + y = 8 in z = 0

# (name, A, B, verdict inside one mesh, verdict between two meshes)
ZOO = [
    # B's first corner (2, 2, 0) lies strictly inside A, the rest of B above the plane: one common point
    ("vertex touches a face interior", BASE, ((2, 2, 0), (2, 2, 5), (5, 2, 5)), True, True),
    # a hexagram: no corner of one inside the other, every edge of A crosses two edges of B in the plane
    ("coplanar edges crossing", ((0, 0, 0), (6, 0, 0), (3, 6, 0)), ((0, 4, 0), (6, 4, 0), (3, -2, 0)), True, True),
    # B's nearest corner (5, 5) has x + y = 10 > 8: beyond A's long edge, though the boxes overlap
    ("coplanar and disjoint", BASE, ((5, 5, 0), (9, 5, 0), (5, 9, 0)), False, False),
    # no edge of one meets an edge of the other; B's corners lie in A
    ("coplanar, one inside the other", ((0, 0, 0), (12, 0, 0), (0, 12, 0)), ((2, 2, 0), (5, 2, 0), (2, 5, 0)), True, True),
    ("parallel planes", BASE, ((0, 0, 1), (8, 0, 1), (0, 8, 1)), False, False),
    # B leaves the shared corner towards negative x and y and upwards: the corner is the only common point, which one mesh
    # forgives and two meshes do not
    ("one shared vertex, otherwise apart", BASE, ((0, 0, 0), (-8, 0, 3), (0, -8, 3)), False, True),
    # B's edge opposite the shared corner runs from (2, 2, -3) to (2, 2, 3): through A's interior at (2, 2, 0)
    ("one shared vertex, the opposite edge piercing", BASE, ((0, 0, 0), (2, 2, -3), (2, 2, 3)), True, True),
    # both wedges open into the first quadrant; A's long edge x + y = 8 crosses B's two sides
    ("one shared vertex, coplanar wedges overlapping", BASE, ((0, 0, 0), (10, 2, 0), (2, 10, 0)), True, True),
    # B's wedge opens below the x axis: only the corner is common
    ("one shared vertex, coplanar wedges not overlapping", BASE, ((0, 0, 0), (8, -1, 0), (3, -8, 0)), False, True),
    # B shares A's corner (8, 0, 0) and has the corner (4, 0, 0) in the middle of A's edge from (0, 0, 0) to (8, 0, 0)
    ("a T-junction at a shared vertex", BASE, ((4, 0, 0), (8, 0, 0), (6, -5, 2)), True, True),
    # the same without a shared point: B's corner (4, 0, 0) on A's edge, touching
    ("a T-junction, nothing shared", BASE, ((4, 0, 0), (2, -5, 1), (6, -5, 1)), True, True),
    # proper neighbours over the edge (0, 0, 0) - (8, 0, 0): B rises out of the plane
    ("a shared edge, not coplanar", BASE, ((0, 0, 0), (8, 0, 0), (3, 3, 5)), False, True),
    # B lies in the plane below the x axis, A above it
    ("a shared edge, coplanar on opposite sides", BASE, ((8, 0, 0), (0, 0, 0), (3, -6, 0)), False, True),
    # B's third corner (3, 5, 0) lies on A's side of the shared edge: a fold laid flat
    ("a shared edge, folded flat", BASE, ((0, 0, 0), (8, 0, 0), (3, 5, 0)), True, True),
    ("a duplicate, same winding", BASE, ((8, 0, 0), (0, 8, 0), (0, 0, 0)), True, True),
    ("a duplicate, opposite winding", BASE, ((0, 0, 0), (0, 8, 0), (8, 0, 0)), True, True),
    # three points in a line inside A: no area, intersects nothing
    ("a degenerate partner (collinear)", BASE, ((1, 1, 0), (2, 2, 0), (3, 3, 0)), False, False),
    ("a degenerate partner (repeated corner)", BASE, ((2, 2, 0), (2, 2, 0), (2, 2, 5)), False, False),
    # B stands on the diagonal x = y, from z = -3 to z = 3: it cuts A along a segment
    ("a proper crossing", BASE, ((2, 2, -3), (2, 2, 3), (9, 9, 3)), True, True),
    # the same plane x = y, but beyond A's long edge
    ("crossing planes, triangles apart", BASE, ((9, 9, -3), (9, 9, 3), (12, 12, 0)), False, False),
    # B's corner (4, 4, 0) is the midpoint of A's long edge, its other corners lie beyond that edge
    ("a vertex touches an edge from outside", BASE, ((4, 4, 0), (9, 9, 2), (9, 9, -2)), True, True),
]


def _variants(A, B):
    """every rotation of both triangles' corners, both windings of B, both roles, the three cyclic renamings of the axes"""
    A, B = np.array(A, np.int64), np.array(B, np.int64)
    for ra, rb, flip, swap, axes in itertools.product(range(3), range(3), (False, True), (False, True), range(3)):
        a, b = np.roll(A, ra, 0), np.roll(B, rb, 0)
        if flip:
            b = b[::-1]
        a, b = np.roll(a, axes, 1), np.roll(b, axes, 1)
        yield (b, a) if swap else (a, b)


# ---- 1. the tie zoo ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ZOO, ids=[z[0] for z in ZOO])
def test_zoo_verdicts(case):
    name, A, B, inside, between = case
    pairs = list(_variants(A, B))
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    assert len(pairs) == 108
    got = mr.verdicts(a, b, True)
    assert (got == inside).all(), (name, "one mesh", np.flatnonzero(got != inside)[:5])
    got = mr.verdicts(a, b, False)
    assert (got == between).all(), (name, "two meshes", np.flatnonzero(got != between)[:5])
    # a larger lattice changes nothing: the same shapes scaled by 2^15 and moved to the lattice's corner
    big = (1 << 15, np.array([-(1 << 19), 1 << 18, -(1 << 19) + 7]))
    for same in (True, False):
        assert (mr.verdicts(a * big[0] + big[1], b * big[0] + big[1], same) == (inside if same else between)).all()


# ---- 2. the restatement against its second form -----------------------------------------------------------------------------------
def _both(A, B, same):
    fast = mr.verdicts(A, B, same)
    slow = np.array([mr.verdict_big(a, b, same) for a, b in zip(A, B)], bool)
    assert np.array_equal(fast, slow), np.flatnonzero(fast != slow)[:5]
    return fast


def test_second_form_on_the_zoo():
    for name, A, B, inside, between in ZOO:
        pairs = list(_variants(A, B))
        a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        assert (_both(a, b, True) == inside).all() and (_both(a, b, False) == between).all(), name


@pytest.mark.parametrize("name", sorted(mr.TABLE))
def test_second_form_on_the_meshes(name):
    v, f = mr.TABLE[name][0]()
    tri = mr.snap_mesh(v, f, mr.LATTICE)
    lo, hi = mr.boxes(tri)
    i, j = mr.candidates(lo, hi, lo, hi)                        # every pair whose boxes meet (all that can intersect) ...
    keep = i < j
    i, j = i[keep], j[keep]
    rng = np.random.default_rng(11)
    if len(i) > 6000:
        pick = rng.choice(len(i), 6000, replace=False)
        hit = np.flatnonzero(mr.verdicts(tri[i], tri[j], True))  # ... sampled where they are many, every intersecting pair kept
        pick = np.union1d(pick, hit)
        i, j = i[pick], j[pick]
    ri, rj = rng.integers(0, len(tri), 1000), rng.integers(0, len(tri), 1000)     # ... and pairs at random
    i, j = np.concatenate([i, ri[ri != rj]]), np.concatenate([j, rj[ri != rj]])
    _both(tri[i], tri[j], True)
    _both(tri[i], tri[j], False)


def test_second_form_at_the_corners_of_the_lattice():
    """triangles whose corners lie at +-2^19 (and at 0): the largest differences and products the contract allows"""
    rng = np.random.default_rng(12)
    n = 6000
    A = rng.choice([-mr.SNAP_MAX, 0, mr.SNAP_MAX], (n, 3, 3))
    B = rng.choice([-mr.SNAP_MAX, 0, mr.SNAP_MAX], (n, 3, 3))
    B[: n // 3, 0] = A[: n // 3, 1]                              # a third share a point, a sixth an edge
    B[: n // 6, 1] = A[: n // 6, 2]
    B[n // 2: n // 2 + 500] = rng.integers(-mr.SNAP_MAX, mr.SNAP_MAX + 1, (500, 3, 3))
    for same in (True, False):
        got = _both(A, B, same)
        assert 0.05 < got.mean() < 0.95                         # both verdicts occur
    M = mr.SNAP_MAX
    flat = np.array([[[-M, -M, 0], [M, -M, 0], [0, M, 0]]])     # holds the origin in its interior
    stab = np.array([[[0, 0, -M], [0, 0, M], [M, M, M]]])       # its first edge runs along the z axis through the origin
    wall = np.array([[[M, M, -M], [M, M, M], [M, 0, M]]])       # in the plane x = M, which flat meets at (M, -M, 0) only
    assert _both(flat, stab, True).all() and not _both(flat, wall, True).any()


# ---- 3. an independent yardstick: the edges of one cast as rays at the other ---------------------------------------------------------
def test_closed_test_equals_ray_casting_where_no_predicate_is_zero():
    rng = np.random.default_rng(7)
    tri = rng.integers(-700, 701, (160, 1, 3)) + rng.integers(-300, 301, (160, 3, 3))
    L = 11
    v = (tri.reshape(-1, 3) / 2.0 ** L).astype(np.float32)
    f = np.arange(480).reshape(160, 3)
    assert np.array_equal(mr.snap_mesh(v, f, L), tri)
    i, j = np.triu_indices(160, 1)
    assert len(i) == 12720
    A, B = tri[i], tri[j]
    closed = mr.verdicts(A, B, False)
    # zero predicates: a corner of one in the plane of the other, or an edge of one coplanar with an edge of the other
    zero = np.zeros(len(i), bool)
    for k in range(3):
        zero |= mr._o3(A[:, 0], A[:, 1], A[:, 2], B[:, k]) == 0
        zero |= mr._o3(B[:, 0], B[:, 1], B[:, 2], A[:, k]) == 0
        for m in range(3):
            zero |= mr._o3(A[:, k], A[:, (k + 1) % 3], B[:, m], B[:, (m + 1) % 3]) == 0
    # every edge of every triangle as a ray with 0 <= t < 1 against every triangle, through the ray caster's own pair test
    origin = tri.astype(np.float64) / 2.0 ** L
    rays = np.concatenate([origin, np.roll(origin, -1, 1) - origin], -1).reshape(-1, 6).astype(np.float32)     # ray 3 t + e = edge e of t
    hit = rr.pair(v, f, rays, 0.0, 1.0)[0].reshape(160, 3, 160).any(1)                                      # [triangle of the edge, target]
    cast = hit[i, j] | hit[j, i]
    print(f"{len(i)} pairs, {int(closed.sum())} intersecting, {int(zero.sum())} with a zero predicate, "
          f"{int((closed != cast)[~zero].sum())} disagreements")
    assert zero.mean() <= 0.01
    assert np.array_equal(closed[~zero], cast[~zero])
    assert closed.sum() > 50


# ---- 4. the numbers of the table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mr.TABLE))
def test_table(name):
    make, pairs, degenerate = mr.TABLE[name]
    v, f = make()
    r = mr.result(v, f, mr.LATTICE)
    assert (r["count"], int(r["degenerate"].sum())) == (pairs, degenerate)
    assert r["hits"].sum() == 2 * pairs and r["hits"].dtype == np.int32
    if len(f) <= 700:                                           # culling by boxes changes nothing
        brute = mr.result(v, f, mr.LATTICE, cull=False)
        assert np.array_equal(brute["pairs"], r["pairs"]) and np.array_equal(brute["hits"], r["hits"])
    if name == "spliced_sheet":
        assert r["pairs"].tolist() == [[16, 155], [54, 221]]
    if name == "two_cubes":
        assert r["pairs"].tolist() == [[10, 21], [11, 20]]        # the coincident faces of the touching side
    if name == "two_spheres":
        assert (r["pairs"][:, 0] < 320).all() and (r["pairs"][:, 1] >= 320).all()      # every one between the two spheres
        b = mr.result_between(v, f[:320], v, f[320:], mr.LATTICE)
        assert np.array_equal(b["pairs"] + [0, 320], r["pairs"])


def test_two_spheres_do_not_depend_on_order_or_rotation():
    v, f = mr.two_spheres()
    base = mr.result(v, f, mr.LATTICE)["pairs"]
    rng = np.random.default_rng(13)
    perm = rng.permutation(len(f))
    g = np.stack([np.roll(f[p], rng.integers(0, 3)) for p in perm])
    got = perm[mr.result(v, g, mr.LATTICE)["pairs"]]
    got = np.sort(got, 1)
    got = got[np.lexsort((got[:, 1], got[:, 0]))]
    assert np.array_equal(got, base)


def test_refusals_of_the_restatement():
    v, f = rr.cube()
    for bad in (np.nan, 2.5, -np.inf):                          # 2.5 * 2^18 > 2^19
        w = v.copy()
        w[3, 1] = bad
        with pytest.raises(ValueError, match="1 vertices"):
            mr.snap_mesh(w, f, mr.LATTICE)
    g = f.copy()
    g[5, 2] = len(v)
    with pytest.raises(ValueError):
        mr.snap_mesh(v, g, mr.LATTICE)
    assert mr.snap_mesh(v * 4, f, mr.LATTICE).max() == mr.SNAP_MAX      # exactly 2^19 is inside


# ---- 5. lattice_for ---------------------------------------------------------------------------------------------------------------
def test_lattice_for():
    from surfd_amd.meshintersect import lattice_for
    t = torch.tensor
    assert lattice_for(t([[0.3, -1.0, 0.5]])) == 19 and lattice_for(t([[0.3, -0.99, 0.5]])) == 19
    assert lattice_for(t([[0.5, 0.0, 0.0]])) == 20 and lattice_for(t([[0.5000001, 0.0, 0.0]])) == 19
    assert lattice_for(t([[1.0000001, 0.0, 0.0]])) == 18 and lattice_for(t([[1.25, 0.0, 0.0]])) == 18
    assert lattice_for(t([[0.1, 0.0, 0.0]]), t([[0.0, -300.0, 0.0]])) == 10          # over all tensors given: 300 * 2^10 <= 2^19 < 300 * 2^11
    assert lattice_for(t([[0.0, 0.0, 0.0]])) == 19
    assert lattice_for(t([[2.0 ** -30, 0.0, 0.0]])) == 49
    with pytest.raises(ValueError):
        lattice_for(t([[float("nan"), 0.0, 0.0]]))
    with pytest.raises(ValueError):
        lattice_for()
    rng = np.random.default_rng(14)
    for scale in (1e-3, 0.7, 1.0, 3.0, 1e4):
        x = (rng.uniform(-1, 1, (50, 3)) * scale).astype(np.float32)
        L = lattice_for(torch.from_numpy(x))
        assert L == mr.lattice_for(x)
        m = float(np.abs(x).max())
        assert m * 2.0 ** L <= 2 ** 19 < m * 2.0 ** (L + 1)
        assert mr.snap(x, L)[1].all() and not mr.snap(x, L + 1)[1].all()


def test_wrapper_refuses_cpu_tensors():
    from surfd_amd import meshintersect
    v, f = (torch.from_numpy(x) for x in rr.cube())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshintersect.IntersectionScene(v, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshintersect.self_intersections(v, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshintersect.mesh_intersections(v, f, v, f)
    with pytest.raises(ValueError):
        meshintersect.IntersectionScene(v, f[:0])
    with pytest.raises(TypeError):
        meshintersect.IntersectionScene(v.double(), f)


# ---- 6. the drivers' argument errors ------------------------------------------------------------------------------------------------
def test_driver_argument_errors(tmp_path):
    from examples import evaluate, reconstruct
    base = ["--generated", str(tmp_path), "--reference", str(tmp_path)]
    for flag in ("--self_intersections", "--collisions"):
        with pytest.raises(SystemExit, match="--paired"):
            evaluate.run(evaluate.parse(base + [flag]))
    a = evaluate.parse(base + ["--paired", "--self_intersections", "--collisions"])
    assert a.self_intersections and a.collisions
    d = evaluate.parse(base)
    assert not d.self_intersections and not d.collisions
    with pytest.raises(SystemExit, match="--metrics"):
        reconstruct.run(reconstruct.parse(["--synthetic", "--mesh_quality", "--output_dir", str(tmp_path / "out")]))
    assert not (tmp_path / "out").exists()                      # refused before anything is written
    assert reconstruct.parse(["--metrics", "--mesh_quality"]).mesh_quality and not reconstruct.parse([]).mesh_quality
