"""csrc/winding.hip on the GPU against the numpy restatement tests/winding_ref.py: values within
F 2^-50 through the raw ABI and through WindingScene on every mesh of the case makers and on each side of the chunk (256) and
group (4 096) boundaries, bit identity of a query's value across batches, positions, repeats and splits, face permutation and
corner rotation, occupancy / is_inside / the sign of the signed distance, voxelize_winding, refusals, and the two drivers."""
import functools
import os
import sys

import ctypes as C
import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raycast_ref as rr  # noqa: E402
import winding_ref as wr  # noqa: E402
import mesh_udf_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = (1, 2, 255, 256, 257, 4095, 4096, 4097)          # each side of a chunk and of a group
QS = (1, 63, 64, 65, 255, 256, 257)                   # each side of a wave and of a workgroup


def cu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


class RawWinding:
    """the C ABI as it is"""

    def __init__(self, v, f):
        from surfd_amd import _native as N
        self.N = N
        self.v, self.f = cu(v), cu(f, torch.int32)
        self.h = C.c_void_p()
        N.check(N.lib().surfd_winding_create(N.ptr(self.v), len(v), N.ptr(self.f), len(f), N.stream(), C.byref(self.h)))
        assert N.lib().surfd_winding_num_triangles(self.h) == len(f)

    def eval(self, points, flags=0):
        N, Q = self.N, len(points)
        p = cu(np.asarray(points, dtype=np.float32))
        w = torch.full((Q,), -7.0, device="cuda", dtype=torch.float64)
        N.check(N.lib().surfd_winding_eval(self.h, N.ptr(p), Q, flags, N.ptr(w), N.stream()))
        torch.cuda.synchronize()
        return w.cpu().numpy()

    def __del__(self):
        self.N.lib().surfd_winding_destroy(self.h)


# ---- the cases: name -> (mesh, queries); reference values are computed once -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def holed():
    v, f, holes = wr.holed_sphere()
    return v, f, holes


@functools.lru_cache(maxsize=None)
def big_torus():
    v, f = rr.torus(132, 64)
    assert len(f) == 16896                                               # 66 chunks, five groups, the last one of two chunks
    return v, f


def uniform_queries(n, seed=1):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32)


def _cases():
    out = {}
    meshes = {name: make() for name, make in rr.MESHES.items()}
    meshes["holed_sphere"] = holed()[:2]
    for name, mesh in meshes.items():
        out[f"mesh-{name}"] = (mesh, uniform_queries(2000))
    for F in FS:
        out[f"F-{F}"] = (rr.first_faces(big_torus(), F), uniform_queries(max(QS), 200 + F))
    out["F-16896"] = (big_torus(), uniform_queries(300, 300))
    return out


CASES = _cases()
MESH_CASES = sorted(k for k in CASES if k.startswith("mesh-"))


@functools.lru_cache(maxsize=None)
def reference(name):
    (v, f), q = CASES[name]
    w = wr.winding_number(v, f, q)
    w.setflags(write=False)
    return w


def close(got, ref, F, what):
    err = float(np.abs(got - ref).max())
    print(f"{what}: F = {F}, Q = {len(ref)}, max |w - w_ref| = {err:.3e}, bound {wr.tolerance(F):.3e}")
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert err <= wr.tolerance(F), (what, err, wr.tolerance(F))


# ---- 1. values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESH_CASES + ["F-16896"])
def test_values_against_the_restatement(name):
    from surfd_amd.winding import WindingScene, winding_number
    (v, f), q = CASES[name]
    ref = reference(name)
    close(RawWinding(v, f).eval(q), ref, len(f), f"{name} raw")
    scene = WindingScene(cu(v), cu(f))
    w = scene.winding_number(cu(q))
    assert w.dtype == torch.float64 and w.is_cuda
    close(w.cpu().numpy(), ref, len(f), f"{name} scene")
    if name == "mesh-cube":
        assert torch.equal(winding_number(cu(v), cu(f, torch.int32), cu(q)), w)


@pytest.mark.parametrize("F", FS)
def test_values_at_the_chunk_and_group_boundaries(F):
    from surfd_amd.winding import WindingScene
    (v, f), q = CASES[f"F-{F}"]
    ref = reference(f"F-{F}")
    raw, scene = RawWinding(v, f), WindingScene(cu(v), cu(f))
    full = raw.eval(q)
    for Q in QS:
        got = raw.eval(q[:Q])
        close(got, ref[:Q], F, f"F-{F} Q-{Q} raw")
        assert np.array_equal(got.view(np.uint64), full[:Q].view(np.uint64))            # the batch does not reach the bits
        close(scene.winding_number(cu(q[:Q])).cpu().numpy(), ref[:Q], F, f"F-{F} Q-{Q} scene")


# ---- 2. bit identity -------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_batch_position_repeat_or_splits():
    from surfd_amd.winding import WindingScene
    (v, f), q = CASES["F-16896"]
    scene = WindingScene(cu(v), cu(f))
    qd = cu(q)
    among = scene.winding_number(qd)                                     # 300 queries: two blocks of queries
    again = scene.winding_number(qd)
    alone = scene.winding_number(qd[:5].contiguous())                    # 5 queries: the five groups go to five splits
    rev = scene.winding_number(qd.flip(0).contiguous()).flip(0)
    single = scene.winding_number(qd, one_split=True)                    # one workgroup per block of queries walks all groups
    assert among.dtype == torch.float64
    assert torch.equal(among, again)
    assert torch.equal(alone, among[:5])
    assert torch.equal(rev, among)
    assert torch.equal(single, among)
    assert torch.equal(scene.winding_number(qd[:5].contiguous(), one_split=True), alone)
    one_by_one = torch.cat([scene.winding_number(qd[i:i + 1].contiguous()) for i in (0, 7, 299)])
    assert torch.equal(one_by_one, among[[0, 7, 299]])


@pytest.mark.parametrize("name", ["cube", "sheet", "F-16896"])
def test_workspace_regrowth_changes_nothing(name):
    """One handle: 64 queries, then 5000, then the first 64 again, each also with ``one_split``.  The handle's arena
    (csrc/meshscene.h) holds ngroup * Q partial sums, so the second round has to free and allocate it and the third runs in an
    arena larger than it needs.  Every call equals the same call on a fresh handle.  cube: 12 triangles; sheet: 450; both are
    one group, so S = 1 either way.  F-16896: five groups, S = 5, and 1 with ``one_split``."""
    from surfd_amd.winding import WindingScene
    v, f = {"cube": rr.cube, "sheet": lambda: rr.wavy_sheet(16), "F-16896": big_torus}[name]()
    assert len(f) == {"cube": 12, "sheet": 450, "F-16896": 16896}[name]
    vd, fd = cu(v), cu(f)
    q = cu(uniform_queries(5000, 31))
    small = q[:64].contiguous()
    scene = WindingScene(vd, fd)
    for points in (small, q, small):
        w = scene.winding_number(points)
        single = scene.winding_number(points, one_split=True)
        assert torch.equal(w, WindingScene(vd, fd).winding_number(points))
        assert torch.equal(single, w)
        assert not bool(torch.isnan(w).any())


# ---- 3. face permutation and corner rotation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mesh-torus", "mesh-spliced_sheet", "F-16896"])
def test_face_order_and_corner_rotation_stay_within_the_bound(name):
    (v, f), q = CASES[name]
    ref = reference(name)
    rng = np.random.default_rng(11)
    close(RawWinding(v, f[rng.permutation(len(f))]).eval(q), ref, len(f), f"{name} permuted")
    close(RawWinding(v, f[:, [1, 2, 0]]).eval(q), ref, len(f), f"{name} rotated")
    close(RawWinding(v, f[:, [0, 2, 1]]).eval(q), -ref, len(f), f"{name} reversed")


# ---- 4. occupancy, is_inside and the sign of the signed distance -----------------------------------------------------------------
@pytest.mark.parametrize("name", MESH_CASES)
def test_occupancy_is_inside_and_sign(name):
    from surfd_amd import meshprep
    from surfd_amd.winding import WindingScene
    (v, f), q = CASES[name]
    ref = reference(name)
    decided = wr.decided(ref, len(f))
    assert int((~decided).sum()) == 0                                    # no query of these inputs sits on the threshold
    want = wr.occupancy(ref)
    scene = WindingScene(cu(v), cu(f))
    qd = cu(q)
    occ, w = scene.compute_occupancy(qd, return_winding=True)
    assert occ.dtype == torch.float32 and torch.equal(w, scene.winding_number(qd))
    assert np.array_equal(occ.cpu().numpy(), want.astype(np.float32))
    assert torch.equal(scene.compute_occupancy(qd), occ)
    inside = meshprep.is_inside(cu(v), cu(f), qd, method="winding")
    assert inside.dtype == torch.bool and np.array_equal(inside.cpu().numpy(), want)
    assert torch.equal(meshprep.is_inside(scene, None, qd, method="winding"), inside)
    sdf = scene.compute_signed_distance(qd)
    dist = scene.mesh_distance().closest(qd)[0]
    assert sdf.dtype == torch.float32 and torch.equal(sdf.abs(), dist)
    assert np.array_equal(torch.signbit(sdf).cpu().numpy(), want)
    s2, grad = meshprep.compute_sdf_and_gradients(scene, None, qd, sign="winding")
    assert torch.equal(s2, sdf) and grad.shape == (len(q), 3)
    s3, _ = meshprep.compute_sdf_and_gradients(cu(v), cu(f), qd, sign="winding")
    assert torch.equal(s3, sdf)
    # another threshold moves the rule, nothing else
    lo = scene.compute_occupancy(qd, threshold=0.25)
    assert np.array_equal(lo.cpu().numpy(), (np.abs(w.cpu().numpy()) >= 0.25).astype(np.float32))


def test_a_scene_of_the_other_kind_is_refused():
    from surfd_amd import meshprep
    from surfd_amd.raycast import RaycastingScene
    from surfd_amd.winding import WindingScene
    v, f = (cu(x) for x in rr.cube())
    q = cu(uniform_queries(8))
    with pytest.raises(TypeError, match="WindingScene"):
        meshprep.is_inside(RaycastingScene(v, f), None, q, method="winding")
    with pytest.raises(TypeError, match="RaycastingScene"):
        meshprep.compute_sdf_and_gradients(WindingScene(v, f), None, q)


def test_holed_sphere_is_answered_where_parity_is_not():
    from surfd_amd import meshprep
    from surfd_amd.winding import WindingScene
    v, f, holes = holed()
    q, kept, inside = wr.holed_sphere_queries(holes)
    qd = cu(q[kept])
    truth = inside[kept]
    scene = WindingScene(cu(v), cu(f))
    assert np.array_equal(scene.compute_occupancy(qd).cpu().numpy() > 0, truth)
    assert np.array_equal(meshprep.is_inside(scene, None, qd, method="winding").cpu().numpy(), truth)
    assert np.array_equal(torch.signbit(scene.compute_signed_distance(qd)).cpu().numpy(), truth)
    parity = meshprep.is_inside(cu(v), cu(f), qd).cpu().numpy()          # the default: what the feature is for
    assert int((parity != truth).sum()) >= 300


# ---- 5. voxelize_winding ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere", "holed_sphere"])
def test_voxelize_winding(name):
    from surfd_amd import voxelize
    v, f = rr.icosphere() if name == "icosphere" else holed()[:2]
    R, lo, hi = 16, -1.0, 1.0
    c = np.float32(lo) + (np.arange(R, dtype=np.float32) + np.float32(0.5)) * np.float32((hi - lo) / R)
    centres = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    ref = wr.winding_number(v, f, centres)
    assert int((~wr.decided(ref, len(f))).sum()) == 0
    want = wr.occupancy(ref).reshape(R, R, R)
    grid = voxelize.voxelize_winding(cu(v), cu(f), R, (lo, hi))
    assert isinstance(grid, voxelize.VoxelGrid) and grid.resolution == R and grid.bounds == (lo, hi)
    assert np.array_equal(grid.dense().cpu().numpy(), want)
    assert grid.count() == int(want.sum()) > 0
    closed = voxelize.voxelize_winding(cu(rr.icosphere()[0]), cu(rr.icosphere()[1]), R, (lo, hi))
    if name == "holed_sphere":                                           # the holes cost a few voxels next to them, not columns
        assert float(voxelize.voxel_iou(grid, closed)) > 0.9
        solid = voxelize.voxelize_solid(cu(v), cu(f), R, (lo, hi))[0]
        assert float(voxelize.voxel_iou(solid, closed)) < float(voxelize.voxel_iou(grid, closed))
    else:
        assert torch.equal(grid.packed, closed.packed)
    half = voxelize.voxelize_winding(cu(v), cu(f), R, (lo, hi), threshold=0.9)
    assert np.array_equal(half.dense().cpu().numpy(), (np.abs(ref) >= 0.9).reshape(R, R, R))


# ---- 6. refusals and special values ----------------------------------------------------------------------------------------------
def test_refusals():
    from surfd_amd import _native as N
    from surfd_amd.winding import WindingScene
    v, f = rr.cube()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        WindingScene(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(TypeError):
        WindingScene(cu(v).double(), cu(f))
    scene = WindingScene(cu(v), cu(f))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.winding_number(torch.zeros(3, 3))
    with pytest.raises(TypeError):
        scene.winding_number(torch.zeros(3, 3, device="cuda", dtype=torch.float64))
    bad_f = f.copy()
    bad_f[5, 1] = len(v)
    with pytest.raises(ValueError, match="outside"):
        WindingScene(cu(v), cu(bad_f))
    bad_v = v.copy()
    bad_v[3, 2] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        WindingScene(cu(bad_v), cu(f))
    # the library finds both on the device and answers with SURFD_ERR_ARG, never with a fault
    h = C.c_void_p()
    for vv, ff, text in ((v, bad_f, b"outside"), (bad_v, f, b"NaN"), (np.where(np.isnan(bad_v), np.float32(np.inf), bad_v), f, b"Inf")):
        vd, fd = cu(vv), cu(ff, torch.int32)
        assert N.lib().surfd_winding_create(N.ptr(vd), len(vv), N.ptr(fd), len(ff), N.stream(), C.byref(h)) == -1
        assert text in N.lib().surfd_last_error() and h.value is None
    neg = f.copy()
    neg[0, 0] = -1
    vd, fd = cu(v), cu(neg, torch.int32)
    assert N.lib().surfd_winding_create(N.ptr(vd), len(v), N.ptr(fd), len(f), N.stream(), C.byref(h)) == -1
    raw = RawWinding(v, f)
    p = cu(uniform_queries(4))
    w = torch.zeros(4, device="cuda", dtype=torch.float64)
    assert N.lib().surfd_winding_eval(raw.h, N.ptr(p), 4, 2, N.ptr(w), N.stream()) == -1          # an unknown flag
    assert N.lib().surfd_winding_eval(raw.h, N.ptr(p), -1, 0, N.ptr(w), N.stream()) == -1
    assert N.lib().surfd_winding_eval(raw.h, N.ptr(p), 2 ** 31, 0, N.ptr(w), N.stream()) == -1
    assert N.lib().surfd_winding_eval(raw.h, None, 4, 0, N.ptr(w), N.stream()) == -1
    assert N.lib().surfd_winding_eval(raw.h, N.ptr(p), 4, 0, None, N.stream()) == -1
    assert N.lib().surfd_winding_eval(raw.h, None, 0, 0, None, N.stream()) == 0                    # Q = 0 is a no-op
    torch.cuda.synchronize()
    assert not w.any()


def test_empty_and_non_finite_queries():
    from surfd_amd.winding import WindingScene
    v, f = rr.octahedron()
    scene = WindingScene(cu(v), cu(f))
    empty = scene.winding_number(torch.zeros(0, 3, device="cuda"))
    assert empty.shape == (0,) and empty.dtype == torch.float64
    assert scene.compute_occupancy(torch.zeros(0, 3, device="cuda")).shape == (0,)
    q = np.array([(0.1, 0.1, 0.1), (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (2, 2, 2), (0.1, 0.1, 0.1)], dtype=np.float32)
    w = scene.winding_number(cu(q)).cpu().numpy()
    ref = wr.winding_number(v, f, q)
    assert np.isnan(w[1:4]).all() and np.isnan(ref[1:4]).all()
    ok = [0, 4, 5]
    assert np.abs(w[ok] - ref[ok]).max() <= wr.tolerance(len(f)) and w[0].view(np.uint64) == w[5].view(np.uint64)
    assert scene.compute_occupancy(cu(q)).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    assert torch.signbit(scene.compute_signed_distance(cu(q)[[0, 4]].contiguous())).tolist() == [True, False]
    # a query on a vertex, on an edge and in a face's plane: finite, and what the restatement gives within the bound
    v, f = rr.cube()
    on = np.array([(0.5, 0.5, 0.5), (0.5, 0.5, 0.0), (0.5, 0.25, 0.125), (0.5, 2.0, 3.0)], dtype=np.float32)
    got = RawWinding(v, f).eval(on)
    assert np.isfinite(got).all() and np.abs(got - wr.winding_number(v, f, on)).max() <= wr.tolerance(len(f))


# ---- 7. the drivers --------------------------------------------------------------------------------------------------------------
def test_evaluate_driver_voxel_mode_winding(tmp_path):
    import json
    from examples import evaluate as E
    from surfd_amd import voxelize
    gen, ref = tmp_path / "gen", tmp_path / "ref"
    gen.mkdir(), ref.mkdir()
    hv, hf, _ = holed()
    cv, cf = rr.icosphere(3)
    mesh_udf_ref.write_obj(gen / "ball.obj", hv, hf)                     # the generated item has the holes
    mesh_udf_ref.write_obj(ref / "ball.obj", cv, cf)
    base = ["--generated", str(gen), "--reference", str(ref), "--paired", "--num_points", "256", "--normalize", "none",
            "--output", str(tmp_path / "m.json")]
    plain = E.run(E.parse(base))
    assert "voxel_iou" not in plain["mean"] and "voxel_mode" not in plain["options"]
    out = E.run(E.parse(base + ["--voxel_iou", "16", "--voxel_mode", "winding"]))
    assert out == json.load(open(tmp_path / "m.json"))
    assert out["options"]["voxel_mode"] == "winding" and out["skipped"] == []
    assert {k: out["items"]["ball"][k] for k in ("cd", "fscore")} == {k: plain["items"]["ball"][k] for k in ("cd", "fscore")}
    want = voxelize.voxel_iou(voxelize.voxelize_winding(cu(hv), cu(hf), 16), voxelize.voxelize_winding(cu(cv), cu(cf), 16))
    assert out["items"]["ball"]["voxel_iou"] == float(want) and float(want) > 0.9
    solid = E.run(E.parse(base + ["--voxel_iou", "16", "--voxel_mode", "solid"]))
    assert solid["items"]["ball"]["odd_columns_generated"] > 0 and solid["items"]["ball"]["voxel_iou"] < float(want)


def test_preprocess_udfs_sign_winding(tmp_path):
    from examples import preprocess_udfs as P
    v, f, holes = holed()
    mesh_udf_ref.write_obj(tmp_path / "ball.obj", v, f)
    counts = [1500, 1000, 250, 2000]
    base = [str(tmp_path / "ball.obj"), "--num_surface_points", "3000", "--num_queries_per_std", *map(str, counts), "--seed", "5",
            "--signed", "--num_queries_on_surface", "200"]
    items = {}
    for tag, extra in (("default", []), ("parity", ["--sign", "parity"]), ("winding", ["--sign", "winding"])):
        P.run(P.parse(base + ["--output_dir", str(tmp_path / tag)] + extra))
        items[tag] = dict(np.load(tmp_path / tag / "ball.npz"))
    for k in items["default"]:                                           # naming the default changes nothing
        assert np.array_equal(items["default"][k], items["parity"][k]), k
    z, p = items["winding"], items["default"]
    assert sorted(z) == ["coords", "gradients", "labels", "pcd", "triangles", "vertices"]
    for k in ("coords", "pcd", "vertices", "triangles"):                 # the same random numbers either way
        assert np.array_equal(z[k], p[k]), k
    assert np.array_equal(np.abs(z["labels"]), np.abs(p["labels"]))
    assert not z["labels"][:200].any() and not z["gradients"][:200].any()
    q = z["coords"][200:].astype(np.float64)
    radius = np.linalg.norm(q, axis=1)
    kept = np.abs(radius - 0.75) > 0.05
    for h in holes:
        kept &= np.linalg.norm(q - h, axis=1) > 0.35
    assert kept.sum() > 500
    assert np.array_equal(z["labels"][200:][kept] < 0, radius[kept] < 0.75)
    assert int(((p["labels"][200:][kept] < 0) != (radius[kept] < 0.75)).sum()) > 0           # the parity leaks through the holes
