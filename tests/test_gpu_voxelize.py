"""GPU tests of the voxeliser (surfd_amd/voxelize.py, csrc/voxel.hip) against tests/voxel_ref.py.  Every buffer — packed words,
counters, intersection / union counts and the IoU — is required EQUAL to the numpy restatement: nothing but the specified snap is
floating point, so there is no tolerance.  Meshes have at most 2 000 triangles, R is 8, 32 or 40 (40: a word boundary and 24
padding bits per column, where the XOR masks of the fill could go wrong).  Every test fails on a tree without
surfd_amd/voxelize.py.  Out-of-range indices are covered by the restatement's CPU test and by reading the guard in vx_load();
no test here feeds them to the GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu
RES = (8, 32, 40)


@pytest.fixture(scope="module")
def VZ():
    from surfd_amd import voxelize
    return voxelize


def dev(v, f=None):
    vt = torch.as_tensor(np.asarray(v, np.float32).reshape(-1, 3)).cuda()
    return vt if f is None else (vt, torch.as_tensor(np.asarray(f, np.int32).reshape(-1, 3)).cuda())


def words_of(grid):
    return grid.packed.cpu().numpy().view(np.uint32)


_cache = {}


def cached(key, fn):
    """a restatement computed once for the module and left unchanged"""
    if key not in _cache:
        _cache[key] = fn()
        for a in _cache[key].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _cache[key]


MESHES = {"sheet": X.sheet, "box": lambda: X.box_mesh((-0.61, -0.4, -0.77), (0.52, 0.83, 0.3)), "sphere": X.icosphere}


def surface_of(name, R):
    return cached(("surface", name, R), lambda: X.surface_ref(*MESHES[name](), R))


def solid_of(name, R, include_surface):
    return cached(("solid", name, R, include_surface), lambda: X.solid_ref(*MESHES[name](), R, include_surface=include_surface))


# ---- surface ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [None, "small", "large"])
def test_surface_rule_cases(VZ, path):
    R, U = 8, X.VOXEL_UNITS(8)
    for tri in (X.PLANE_TRIANGLE, X.CORNER_TRIANGLE, X.SLANTED_TRIANGLE):
        g, c = VZ.voxelize_surface(*dev(tri, [[0, 1, 2]]), R, U, path=path, return_counts=True)
        assert np.array_equal(words_of(g), X.surface_ref(tri, [[0, 1, 2]], R, U)["bits"]) and c == {"dropped": 0, "degenerate": 0}
    d = VZ.voxelize_surface(*dev(X.PLANE_TRIANGLE, [[0, 1, 2]]), R, U, path=path).dense().cpu().numpy()
    assert d[:, :, 2].any() and np.array_equal(d[:, :, 2], d[:, :, 3]) and d.sum() == 2 * d[:, :, 2].sum()       # both layers
    d = VZ.voxelize_surface(*dev(X.CORNER_TRIANGLE, [[0, 1, 2]]), R, U, path=path).dense().cpu().numpy()
    assert d.sum() == 8 and d[3:5, 3:5, 3:5].all()                                                                # all 8 voxels
    d = VZ.voxelize_surface(*dev(X.SLANTED_TRIANGLE, [[0, 1, 2]]), R, U, path=path).dense().cpu().numpy()
    assert not d[X.SLANTED_CLEAR] and d.any()                                                                     # edge x axis only


@pytest.mark.parametrize("R", RES)
@pytest.mark.parametrize("path", [None, "small", "large"])
def test_triangle_spanning_partly_and_wholly_outside(VZ, R, path):
    # inside; partly outside on either side; the bounding box overlaps the grid but the triangle passes it by; wholly outside
    for shift, some in ((0.0, True), (0.5, True), (-0.25, True), (-0.75, False), (1.5, False)):
        tri = X.SPANNING_TRIANGLE + np.float32(shift)
        want = X.surface_ref(tri, [[0, 1, 2]], R, (0.0, 1.0))
        g, c = VZ.voxelize_surface(*dev(tri, [[0, 1, 2]]), R, (0.0, 1.0), path=path, return_counts=True)
        assert np.array_equal(words_of(g), want["bits"]) and bool(want["dense"].any()) == some, shift
        assert c == {"dropped": 0, "degenerate": 0} and g.count() == int(want["dense"].sum())


@pytest.mark.parametrize("R", RES)
@pytest.mark.parametrize("name", ["sheet", "box"])
def test_surface_paths_are_bit_identical_and_equal_the_restatement(VZ, name, R):
    v, f = dev(*MESHES[name]())
    want = surface_of(name, R)
    grids = [words_of(VZ.voxelize_surface(v, f, R, path=p)) for p in (None, "small", "large")]
    assert np.array_equal(grids[0], want["bits"]) and want["dense"].any()
    assert np.array_equal(grids[1], grids[0]) and np.array_equal(grids[2], grids[0])
    if R % 32:
        assert not (grids[0][:, :, -1] >> np.uint32(R % 32)).any()                 # padding bits


def test_surface_invariances(VZ):
    R = 40
    v, f = MESHES["sheet"]()
    want = surface_of("sheet", R)["bits"]
    rng = np.random.default_rng(1)
    vt = dev(v)
    for faces in (f[rng.permutation(len(f))], f[:, ::-1], np.concatenate([f, f[::3]])):       # order, winding, duplicates
        assert np.array_equal(words_of(VZ.voxelize_surface(vt, torch.as_tensor(np.ascontiguousarray(faces)).cuda(), R)), want)
    ft = torch.as_tensor(f).cuda()
    for _ in range(10):                                                                      # repetition
        assert np.array_equal(words_of(VZ.voxelize_surface(vt, ft, R)), want)
    # two meshes accumulated into one grid = the OR of their grids
    vb, fb = dev(*MESHES["box"]())
    g = VZ.voxelize_surface(vt, ft, R)
    assert VZ.voxelize_surface(vb, fb, R, out=g) is g
    assert np.array_equal(words_of(g), want | surface_of("box", R)["bits"])
    assert np.array_equal(words_of(VZ.voxelize_surface(vt, ft.long(), R)), want)              # int64 faces are converted


def test_counters_agree_with_the_restatement(VZ):
    R = 8
    v = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [1, 1, 1], [np.nan, 0, 0], [3e5, 0, 0], [0.25, 0, 0], [np.inf, 0, 0]], np.float32)
    f = [[0, 1, 2], [0, 1, 6], [3, 3, 3], [0, 0, 1], [0, 1, 4], [0, 5, 2], [7, 1, 2]]          # every index inside [0, V)
    want = X.surface_ref(v, f, R)
    assert (want["dropped"], want["degenerate"]) == (3, 3)
    for path in (None, "small", "large"):
        g, c = VZ.voxelize_surface(*dev(v, f), R, path=path, return_counts=True)
        assert c == {"dropped": 3, "degenerate": 3} and np.array_equal(words_of(g), want["bits"])
        g, c = VZ.voxelize_solid(*dev(v, f), R, path=path, return_counts=True)
        s = X.solid_ref(v, f, R)
        assert c == {"dropped": 3, "odd_columns": s["odd_columns"]} and np.array_equal(words_of(g), s["bits"])
    g, c = VZ.voxelize_surface(dev(v), torch.zeros(0, 3, dtype=torch.int32).cuda(), R, return_counts=True)     # an empty mesh
    assert c == {"dropped": 0, "degenerate": 0} and g.count() == 0


# ---- solid ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [None, "small", "large"])
def test_solid_rule_cases(VZ, path):
    R, U = 8, X.VOXEL_UNITS(8)
    g, odd = VZ.voxelize_solid(*dev(*X.box_mesh((1, 2, 3), (4, 4, 7))), R, U, include_surface=False, path=path)
    d = g.dense().cpu().numpy()
    assert odd == 0 and d.sum() == 3 * 2 * 4 and d[1:4, 2:4, 3:7].all()                       # faces on voxel boundaries: w h d
    g, odd = VZ.voxelize_solid(*dev(*X.box_mesh((1.5, 1.5, 1.5), (4.5, 4.5, 4.5))), R, U, include_surface=False, path=path)
    d = g.dense().cpu().numpy()
    assert odd == 0 and d.sum() == 27 and d[1:4, 1:4, 2:5].all()                              # faces through voxel centres: strictness
    v, f = X.octahedron((4.5, 4.5, 4.0), 3.0)                                                 # apex and edges through column centres
    want = X.solid_ref(v, f, R, U, include_surface=False)
    g, odd = VZ.voxelize_solid(*dev(v, f), R, U, include_surface=False, path=path)
    assert odd == 0 and want["odd_columns"] == 0 and np.array_equal(words_of(g), want["bits"]) and want["fill"][4, 4, 1:7].all()
    vo, fo = X.box_mesh((1, 1, 1), (7, 7, 7))                                                 # nested boxes: a hollow interior
    vi, fi = X.box_mesh((3, 3, 3), (5, 5, 5))
    g, odd = VZ.voxelize_solid(*dev(np.concatenate([vo, vi]), np.concatenate([fo, fi + 8])), R, U, include_surface=False, path=path)
    d = g.dense().cpu().numpy()
    assert odd == 0 and d.sum() == 6 ** 3 - 2 ** 3 and not d[3:5, 3:5, 3:5].any()


@pytest.mark.parametrize("R", RES)
@pytest.mark.parametrize("include_surface", [False, True])
def test_solid_sphere_equals_the_restatement_on_every_path(VZ, R, include_surface):
    v, f = dev(*MESHES["sphere"]())
    want = solid_of("sphere", R, include_surface)
    assert want["odd_columns"] == 0 and want["fill"].any()
    for path in (None, "small", "large"):
        g, c = VZ.voxelize_solid(v, f, R, include_surface=include_surface, path=path, return_counts=True)
        assert c == {"odd_columns": 0, "dropped": 0} and np.array_equal(words_of(g), want["bits"]), path
    if include_surface:                                                                       # fill | surface is a superset of fill
        fill = solid_of("sphere", R, False)["bits"]
        assert np.array_equal(want["bits"] & fill, fill) and (want["bits"] != fill).any()
        assert np.array_equal(want["bits"], fill | surface_of("sphere", R)["bits"])
    assert VZ.is_closed(v, f, R) is True


@pytest.mark.parametrize("R", [32, 40])
def test_open_sphere_has_odd_columns(VZ, R):
    v, f = MESHES["sphere"]()
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    gone = int(np.argmax(np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])))                  # the triangle with the largest xy projection
    fo = np.delete(f, gone, 0)
    want = X.solid_ref(v, fo, R)
    g, odd = VZ.voxelize_solid(*dev(v, fo), R)
    assert odd == want["odd_columns"] and odd > 0 and np.array_equal(words_of(g), want["bits"])
    assert VZ.is_closed(*dev(v, fo), R) is False
    # face order, winding, duplicates-in-pairs and accumulation do not change the fill
    rng = np.random.default_rng(2)
    for faces in (f[rng.permutation(len(f))], f[:, ::-1], np.concatenate([f, f[:100], f[:100]])):
        g, odd = VZ.voxelize_solid(*dev(v, np.ascontiguousarray(faces)), R)
        assert odd == 0 and np.array_equal(words_of(g), solid_of("sphere", R, True)["bits"])
    g = VZ.voxelize_surface(*dev(*MESHES["box"]()), R)
    VZ.voxelize_solid(*dev(v, f), R, out=g)
    assert np.array_equal(words_of(g), solid_of("sphere", R, True)["bits"] | surface_of("box", R)["bits"])


# ---- points -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RES)
def test_points(VZ, R):
    U = X.VOXEL_UNITS(R)
    rng = np.random.default_rng(R)
    hand = np.array([[1.0, 2.0, 3.0], [0, 0, 0], [R, R, R], [R, 0.5, 0.5], [R + 1 / 64, 1, 1], [-1 / 64, 1, 1], [np.nan, 1, 1],
                     [2.99, 3.0, 3.01], [1, np.inf, 1], [1, 1, -3e6], [R - 1 / 1024, R - 1, R / 2]], np.float32)      # faces, upper face, outside, NaN
    pts = np.concatenate([hand, rng.uniform(-0.1 * R, 1.1 * R, (3000, 3)).astype(np.float32), rng.integers(0, R + 1, (300, 3)).astype(np.float32)])
    want = X.points_ref(pts, R, U)
    g, c = VZ.voxelize_points(dev(pts), R, U, return_counts=True)
    assert np.array_equal(words_of(g), want["bits"]) and c == {"outside": want["outside"]} and want["outside"] > 5
    d = g.dense().cpu().numpy()
    assert d[1, 2, 3] and d[0, 0, 0] and d[R - 1, R - 1, R - 1] and d[R - 1, 0, 0] and d[2, 3, 3]
    g2 = VZ.voxelize_points(dev(pts[:1000]), R, U)
    VZ.voxelize_points(dev(pts[1000:]), R, U, out=g2)                                          # accumulation
    assert np.array_equal(words_of(g2), want["bits"])
    want = X.points_ref(pts / R * 2 - 1, R)                                                   # the default bounds: a non-trivial scale
    assert np.array_equal(words_of(VZ.voxelize_points(dev(pts / R * 2 - 1), R)), want["bits"])


# ---- iou --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RES)
def test_iou(VZ, R):
    rng = np.random.default_rng(R)
    dense = rng.random((5, R, R, R)) < np.array([0.0, 0.1, 0.5, 0.9, 0.5])[:, None, None, None]
    dense[4] = ~dense[2]                                                                     # disjoint from 2
    grids = [VZ.VoxelGrid.from_dense(torch.from_numpy(d).cuda()) for d in dense]
    packed = X.pack(dense)
    for g, w, d in zip(grids, packed, dense):
        assert np.array_equal(words_of(g), w) and g.count() == int(d.sum()) and np.array_equal(g.dense().cpu().numpy(), d)
    inter, union, iou = X.iou_ref(packed, packed)
    gi, gn, gu = VZ.voxel_iou_matrix(grids, grids, return_counts=True)
    assert gi.dtype == torch.float32 and gn.dtype == torch.int32 and tuple(gi.shape) == (5, 5)
    assert np.array_equal(gn.cpu().numpy(), inter) and np.array_equal(gu.cpu().numpy(), union)
    assert np.array_equal(gi.cpu().numpy().view(np.uint32), iou.view(np.uint32))
    assert gi[0, 0] == 1.0 and gi[2, 2] == 1.0 and gi[2, 4] == 0.0 and gi[0, 1] == 0.0          # empty / identical / disjoint
    # counts equal the dense sums computed in torch
    dt = torch.from_numpy(dense).cuda()
    assert torch.equal(gn, (dt[:, None] & dt[None]).sum((2, 3, 4)).int()) and torch.equal(gu, (dt[:, None] | dt[None]).sum((2, 3, 4)).int())
    # paired against the matrix diagonal, on grids and on packed batches
    batch = torch.stack([g.packed for g in grids])
    pi, pn, pu = VZ.voxel_iou(batch, batch.flip(0), return_counts=True)
    mi, mn, mu = VZ.voxel_iou_matrix(batch, batch.flip(0), return_counts=True)
    assert torch.equal(pi, mi.diagonal()) and torch.equal(pn, mn.diagonal()) and torch.equal(pu, mu.diagonal())
    single = VZ.voxel_iou(grids[1], grids[2])
    assert single.dim() == 0 and single == gi[1, 2]
    # entries do not depend on M and N
    sub = VZ.voxel_iou_matrix(grids[1:3], grids[2:])
    assert torch.equal(sub, gi[1:3, 2:])
    with pytest.raises(ValueError, match="resolutions differ"):
        VZ.voxel_iou(grids[0], VZ.VoxelGrid.empty(R + 1))
    with pytest.raises(ValueError, match="as many"):
        VZ.voxel_iou(batch, batch[:2])
    other = [VZ.VoxelGrid(g.packed, R, (0.0, 1.0)) for g in grids[:2]]
    with pytest.raises(ValueError, match="bounds differ"):                                      # lists of grids carry their bounds too
        VZ.voxel_iou_matrix(grids[:2], other)


def test_iou_matrix_beyond_65535_pairs_and_wide_indices(VZ):
    """the pair index rides on gridDim.x: a 260 x 260 matrix (67 600 pairs) is one call; and int64 face indices that do not fit
    int32 are dropped and counted instead of wrapping into [0, V)"""
    R = 8
    rng = np.random.default_rng(7)
    dense = rng.random((260, R, R, R)) < 0.3
    packed = X.pack(dense)
    batch = torch.from_numpy(packed.view(np.int32)).cuda()
    iou, inter, union = VZ.voxel_iou_matrix(batch, batch, return_counts=True)
    wi, wu, wq = X.iou_ref(packed, packed)
    assert np.array_equal(inter.cpu().numpy(), wi) and np.array_equal(union.cpu().numpy(), wu)
    assert np.array_equal(iou.cpu().numpy().view(np.uint32), wq.view(np.uint32))
    v, f = X.box_mesh((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    wide = np.concatenate([f.astype(np.int64), [[0, 1, 2 ** 32 + 2], [2 ** 31, 1, 2], [-2 ** 32 + 1, 1, 2]]])
    g, c = VZ.voxelize_surface(dev(v), torch.from_numpy(wide).cuda(), R, return_counts=True)
    assert c == {"dropped": 3, "degenerate": 0} and np.array_equal(words_of(g), X.surface_ref(v, f, R)["bits"])


def test_mesh_iou_end_to_end(VZ):
    """a sphere against itself shifted: surface, solid and points grids of the same frame, IoU from the library = IoU of dense()"""
    v, f = MESHES["sphere"]()
    a, _ = VZ.voxelize_solid(*dev(v, f), 32)
    b, _ = VZ.voxelize_solid(*dev(v + np.float32(0.1), f), 32)
    iou, inter, union = VZ.voxel_iou(a, b, return_counts=True)
    da, db = a.dense(), b.dense()
    assert int(inter) == int((da & db).sum()) and int(union) == int((da | db).sum()) and 0.5 < float(iou) < 0.95
    assert float(VZ.voxel_iou(a, a)) == 1.0
    p = VZ.voxelize_points(dev(v), 32)
    s = VZ.voxelize_surface(*dev(v, f), 32)
    assert bool((p.dense() & ~s.dense()).sum() == 0)                                          # a vertex's voxel is a surface voxel


# ---- the example driver -----------------------------------------------------------------------------------------------------------
def _write_obj(path, v, f):
    with open(path, "w") as fh:
        fh.writelines(f"v {x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in v)
        fh.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f)


@pytest.mark.parametrize("mode", ["surface", "solid", "points"])
def test_evaluate_driver_voxel_iou(VZ, tmp_path, mode):
    """examples/evaluate.py --paired --voxel_iou (in process): both items in the reference item's frame, .npz clouds scored in
    points mode only, odd_columns recorded in solid mode, and without the flag the output carries no voxel key"""
    import json
    from examples import evaluate as E
    from surfd_amd import meshprep
    gen, ref = tmp_path / "gen", tmp_path / "ref"
    gen.mkdir(), ref.mkdir()
    v, f = X.icosphere(2, 3.0, (5.0, 5.0, 5.0))                                               # far from [-1, 1]^3 before normalisation
    _write_obj(ref / "ball.obj", v, f)
    _write_obj(gen / "ball.obj", v + np.float32(0.06), f)                                     # 0.02 in the reference frame: a third of a voxel
    pts = np.random.default_rng(0).uniform(-1, 1, (4096, 3)).astype(np.float32)
    np.savez(ref / "cloud.npz", points=pts)
    np.savez(gen / "cloud.npz", points=pts[::-1] * np.float32(0.5))
    base = ["--generated", str(gen), "--reference", str(ref), "--paired", "--num_points", "512", "--output", str(tmp_path / "m.json")]
    plain = E.run(E.parse(base))
    assert "voxel_iou" not in plain["mean"] and "skipped" not in plain and all("voxel_iou" not in i for i in plain["items"].values())
    out = E.run(E.parse(base + ["--voxel_iou", "32", "--voxel_mode", mode]))
    assert out == json.load(open(tmp_path / "m.json"))
    assert {k: out["items"]["ball"][k] for k in ("cd", "fscore")} == {k: plain["items"]["ball"][k] for k in ("cd", "fscore")}
    assert out["skipped"] == ([] if mode == "points" else ["cloud"])
    rv, rf = (torch.as_tensor(np.asarray(a)) for a in meshprep.read_mesh(str(ref / "ball.obj")))
    gv, _ = (torch.as_tensor(np.asarray(a)) for a in meshprep.read_mesh(str(gen / "ball.obj")))
    c, r = E.reference_frame(rv.float(), "bbox")
    a_, b_ = (((x.float() - c) / r).contiguous().cuda() for x in (gv, rv))
    ft = rf.int().cuda()
    if mode == "surface":
        want = VZ.voxel_iou(VZ.voxelize_surface(a_, ft, 32), VZ.voxelize_surface(b_, ft, 32))
    elif mode == "solid":
        want = VZ.voxel_iou(VZ.voxelize_solid(a_, ft, 32)[0], VZ.voxelize_solid(b_, ft, 32)[0])
        assert out["items"]["ball"]["odd_columns_generated"] == 0 and out["items"]["ball"]["odd_columns_reference"] == 0
    else:
        want = VZ.voxel_iou(VZ.voxelize_points(a_, 32), VZ.voxelize_points(b_, 32))
        assert 0.0 < out["items"]["cloud"]["voxel_iou"] < 0.5                                  # the half-size cloud fills an eighth of the cube
    assert out["items"]["ball"]["voxel_iou"] == float(want) and 0.0 < float(want) < 1.0
    scored = [i["voxel_iou"] for i in out["items"].values() if "voxel_iou" in i]
    assert out["mean"]["voxel_iou"] == pytest.approx(float(np.mean(scored)), abs=1e-12)
