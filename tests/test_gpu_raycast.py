"""csrc/raycast.hip on the GPU: bit equality with the numpy restatement tests/raycast_ref.py (t, triangle, uv, normal, count)
on every mesh of the case makers and on each side of the kernel's tile (32), chunk (256) and split (64 chunks) boundaries,
culled against brute force, independence of triangle and ray order, bad rays, stability, inside / outside against
mathematics and against the voxeliser, the signed distance and its drivers."""
import functools
import os
import subprocess
import sys

import ctypes as C
import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raycast_ref as rr  # noqa: E402
import mesh_udf_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def cu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


class RawScene:
    """the C ABI as it is: triangles and rays in the order given (the Python wrapper sorts both)"""

    def __init__(self, v, f):
        from surfd_amd import _native as N
        self.N = N
        self.v, self.f = cu(v), cu(f, torch.int32)
        self.h = C.c_void_p()
        N.check(N.lib().surfd_rayscene_create(N.ptr(self.v), len(v), N.ptr(self.f), len(f), N.stream(), C.byref(self.h)))
        assert N.lib().surfd_rayscene_num_triangles(self.h) == len(f)

    def cast(self, rays, tmin=0.0, tmax=INF, flags=0):
        N, R = self.N, len(rays)
        r = cu(rays)
        t = torch.full((R,), -7.0, device="cuda")
        tri = torch.full((R,), -7, device="cuda", dtype=torch.int32)
        uv = torch.full((R, 2), -7.0, device="cuda")
        nrm = torch.full((R, 3), -7.0, device="cuda")
        cnt = torch.full((R,), -7, device="cuda", dtype=torch.int32)
        N.check(N.lib().surfd_rayscene_cast(self.h, N.ptr(r), R, tmin, tmax, flags, N.ptr(t), N.ptr(tri), N.ptr(uv), N.ptr(nrm), N.stream()))
        N.check(N.lib().surfd_rayscene_count(self.h, N.ptr(r), R, tmin, tmax, flags, N.ptr(cnt), N.stream()))
        torch.cuda.synchronize()
        return dict(t=t.cpu().numpy(), tri=tri.cpu().numpy(), uv=uv.cpu().numpy(), normal=nrm.cpu().numpy(), count=cnt.cpu().numpy())

    def __del__(self):
        self.N.lib().surfd_rayscene_destroy(self.h)


def same_bits(got, ref, what=""):
    for k in ("t", "tri", "uv", "normal", "count"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(1))
        assert bad.size == 0, f"{what}: {k} differs for {bad.size} of {len(a)} rays, first {bad[:5]}: {a[bad[:3]]} != {b[bad[:3]]}"


# ---- the cases: name -> (mesh, rays, tmin, tmax); reference results are computed once ----------------------------------------------
def _cases():
    out = {}
    big = {"icosphere": rr.icosphere(3), "torus": rr.torus(), "cube": rr.cube(), "octahedron": rr.octahedron(), "wavy_sheet": rr.wavy_sheet(),
           "spliced_sheet": rr.spliced_sheet(), "cube_flipped": rr.cube_flipped()}
    for i, (name, mesh) in enumerate(big.items()):                       # every mesh; the torus has 2304 triangles, 9 chunks
        out[f"mesh-{name}"] = (mesh, rr.mixed_rays(mesh, 257, 100 + 3 * i), 0.0, INF)
    torus = rr.torus()
    for F in (1, 31, 32, 33, 255, 256, 257, 511, 512, 513):             # each side of a tile and of a chunk
        mesh = rr.first_faces(torus, F)
        out[f"F-{F}"] = (mesh, rr.mixed_rays(mesh, 65, 200 + F), 0.0, INF)
    wide = rr.torus(96, 88)                                              # 16 896 triangles = 66 chunks: two chunks per split, 33 splits
    out["F-16896"] = (wide, rr.mixed_rays(wide, 64, 300), 0.0, INF)
    edge = rr.first_faces(wide, 64 * 256 + 1)                            # 65 chunks: the last split holds one chunk of one triangle
    out["F-16385"] = (edge, rr.mixed_rays(edge, 64, 301), 0.0, INF)
    full = rr.first_faces(wide, 64 * 256)                                # 64 chunks: one chunk per split
    out["F-16384"] = (full, rr.mixed_rays(full, 64, 302), 0.0, INF)
    ico = rr.icosphere(2)
    for R in (1, 63, 64, 65, 255, 256, 257):
        out[f"R-{R}"] = (ico, rr.mixed_rays(ico, R, 400 + R), 0.0, INF)
    out["R-5000"] = (big["icosphere"], rr.mixed_rays(big["icosphere"], 5000, 450), 0.0, INF)      # 20 blocks of rays x 5 splits
    out["range"] = (torus, rr.mixed_rays(torus, 257, 500), 0.3, 1.2)
    for name in ("cube", "cube_flipped"):
        for z0 in (-1.0, 0.0):
            out[f"lattice-{name}-{z0}"] = (big[name], rr.cube_lattice(z0), 0.0, INF)
    out["octahedron-outside"] = (big["octahedron"], rr.octahedron_rays(True), 0.0, INF)
    out["octahedron-centre"] = (big["octahedron"], rr.octahedron_rays(False), 0.0, INF)
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    (v, f), rays, tmin, tmax = CASES[name]
    return rr.cast(v, f, rays, tmin, tmax)


# ---- 1, 2: equality with the restatement, culled and brute force --------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_restatement_bit_for_bit(name):
    (v, f), rays, tmin, tmax = CASES[name]
    ref = reference(name)
    scene = RawScene(v, f)
    same_bits(scene.cast(rays, tmin, tmax, flags=1), ref, f"{name}, brute force")
    same_bits(scene.cast(rays, tmin, tmax, flags=0), ref, f"{name}, culled")
    print(f"{name}: F = {len(f)}, R = {len(rays)}, {int((ref['tri'] >= 0).sum())} hits, counts up to {int(ref['count'].max())}")
    if name.startswith("lattice-cube"):                                   # the contract's ties, on the device
        x, y = rays[:, 0], rays[:, 1]
        inside = (np.abs(x) < 0.5) & (np.abs(y) < 0.5)
        assert (ref["count"][inside] == (2 if rays[0, 2] < -0.5 else 1)).all() and (ref["count"][(np.abs(x) > 0.5) | (np.abs(y) > 0.5)] == 0).all()


def test_culling_skips_work_and_changes_nothing():
    from surfd_amd.raycast import RaycastingScene
    mesh = rr.torus(96, 88)
    rays = cu(rr.mixed_rays(mesh, 5000, 600))
    scene = RaycastingScene(cu(mesh[0]), cu(mesh[1]))
    for tmin, tmax in ((0.0, INF), (0.0, 1.0)):
        a = scene.cast_rays(rays, tmin, tmax, count_skipped=True)
        skipped, total = scene.last_skipped_tiles, scene.last_total_tiles
        b = scene.cast_rays(rays, tmin, tmax, brute_force=True)
        for k in a:
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k
        ca = scene.count_intersections(rays, tmin, tmax, count_skipped=True)
        cskipped = scene.last_skipped_tiles
        assert torch.equal(ca, scene.count_intersections(rays, tmin, tmax, brute_force=True))
        assert total == ((5000 + 63) // 64) * ((len(mesh[1]) + 31) // 32)
        print(f"tmax = {tmax}: cast skipped {skipped} of {total} (wave, tile) visits ({skipped / total:.1%}), count {cskipped} ({cskipped / total:.1%})")
        # how much is skipped depends on how compact a wave's rays are and sets no threshold here; what must hold: culling does
        # engage on a mesh of 66 chunks, and a cast, whose range ends at the lane's best hit, skips every tile the count skips
        assert 0 < cskipped <= skipped <= total


# ---- 3: order independence ----------------------------------------------------------------------------------------------------
def test_independent_of_triangle_and_ray_order():
    from surfd_amd.raycast import RaycastingScene
    v, f = rr.icosphere(3)
    rays = rr.mixed_rays((v, f), 1000, 700)
    base = RaycastingScene(cu(v), cu(f)).cast_rays(cu(rays))
    base_count = RaycastingScene(cu(v), cu(f)).count_intersections(cu(rays))
    ref = rr.cast(v, f, rays)
    assert np.array_equal(base["t_hit"].cpu().numpy().view(np.uint32), ref["t"].view(np.uint32))
    assert np.array_equal(base["primitive_ids"].cpu().numpy(), ref["tri"].astype(np.int64)) and base["primitive_ids"].dtype == torch.int64
    rng = np.random.default_rng(1)
    pf, pr = rng.permutation(len(f)), rng.permutation(len(rays))
    scene = RaycastingScene(cu(v), cu(f[pf]))
    got = scene.cast_rays(cu(rays[pr]))
    back = torch.from_numpy(np.argsort(pr)).cuda()
    ids = got["primitive_ids"][back]
    ids = torch.where(ids >= 0, torch.from_numpy(pf).cuda()[ids.clamp_min(0)], ids)
    assert torch.equal(ids, base["primitive_ids"])
    for k in ("t_hit", "primitive_uvs", "primitive_normals"):
        assert torch.equal(got[k][back].view(torch.int32), base[k].view(torch.int32)), k
    assert torch.equal(scene.count_intersections(cu(rays[pr]))[back], base_count)
    # a set of rays alone and inside a larger call
    alone = RaycastingScene(cu(v), cu(f)).cast_rays(cu(rays[100:164]))
    for k in base:
        assert torch.equal(alone[k].view(torch.int32) if alone[k].dtype == torch.float32 else alone[k],
                           base[k][100:164].view(torch.int32) if base[k].dtype == torch.float32 else base[k][100:164]), k


# ---- 4: bad rays --------------------------------------------------------------------------------------------------------------
def test_bad_rays_miss_and_leave_their_neighbours_alone():
    mesh, rays, _, _ = CASES["mesh-torus"]
    good = reference("mesh-torus")
    bad = rays.copy()
    where = np.array([0, 5, 63, 64, 130, 255, 256])
    bad[0, 0], bad[5, 4], bad[63, 3:], bad[64, 2], bad[130, 5], bad[255, :], bad[256, 3] = np.nan, np.inf, 0.0, -np.inf, np.nan, np.nan, -np.inf
    ref = rr.cast(*mesh, bad)
    assert (ref["tri"][where] == -1).all() and np.isinf(ref["t"][where]).all() and not ref["count"][where].any()
    keep = np.setdiff1d(np.arange(len(rays)), where)
    for k in ref:
        assert np.array_equal(ref[k][keep].view(np.uint32), good[k][keep].view(np.uint32))
    scene = RawScene(*mesh)
    for flags in (0, 1):
        got = scene.cast(bad, flags=flags)
        same_bits(got, ref, f"bad rays, flags {flags}")
        assert not got["uv"][where].any() and not got["normal"][where].any()
    from surfd_amd.raycast import RaycastingScene
    wrapped = RaycastingScene(cu(mesh[0]), cu(mesh[1])).cast_rays(cu(bad))
    assert np.array_equal(wrapped["t_hit"].cpu().numpy().view(np.uint32), ref["t"].view(np.uint32))
    assert np.array_equal(wrapped["primitive_ids"].cpu().numpy(), ref["tri"].astype(np.int64))


# ---- 5: stability -------------------------------------------------------------------------------------------------------------
def test_ten_repeats_give_identical_bits():
    (v, f), rays, tmin, tmax = CASES["R-5000"]
    scene = RawScene(v, f)
    first = scene.cast(rays, tmin, tmax)
    same_bits(first, reference("R-5000"), "first run")
    for i in range(9):
        same_bits(scene.cast(rays, tmin, tmax), first, f"repeat {i + 1}")


@pytest.mark.parametrize("name", ["cube", "sheet"])
def test_workspace_regrowth_changes_nothing(name):
    """One handle: 64 rays, then 5000, then the first 64 again, a cast and a count each time.  The handle's arena
    (csrc/meshscene.h) holds S * R partial results, 64-bit keys for the cast and 32-bit counts for the count in the same
    bytes, so the second round has to free and allocate it and the third runs in an arena larger than it needs.  Every call
    equals the same call on a fresh handle.  cube: 12 triangles, one chunk, S = 1; sheet: 450 triangles, two chunks, S = 2."""
    from surfd_amd.raycast import RaycastingScene
    mesh = rr.cube() if name == "cube" else rr.wavy_sheet(16)
    assert len(mesh[1]) == (12 if name == "cube" else 450)
    vd, fd = cu(mesh[0]), cu(mesh[1])
    rays = cu(rr.mixed_rays(mesh, 5000, 21))
    small = rays[:64].contiguous()
    scene = RaycastingScene(vd, fd)
    for r in (small, rays, small):
        hit, cnt = scene.cast_rays(r), scene.count_intersections(r)
        fresh = RaycastingScene(vd, fd).cast_rays(r)
        assert sorted(hit) == sorted(fresh)
        for key in hit:
            assert torch.equal(hit[key], fresh[key]), key
        assert torch.equal(cnt, RaycastingScene(vd, fd).count_intersections(r))


# ---- 6: inside / outside against mathematics ------------------------------------------------------------------------------------
def _occupancy(mesh, pts, nsamples):
    from surfd_amd.raycast import RaycastingScene
    occ, votes = RaycastingScene(cu(mesh[0]), cu(mesh[1])).compute_occupancy(cu(pts), nsamples=nsamples, return_votes=True)
    assert occ.dtype == torch.float32 and votes.dtype == torch.int32
    return occ.cpu().numpy() > 0, votes.cpu().numpy()


def test_inside_the_icosphere_is_inside_all_face_planes():
    # 320 faces: the slabs of +-1e-6 around the planes of F faces hold about F * 2e-6 / 2 of the cube's points, which for the
    # 1280 faces of the next subdivision is 0.13 %, already past the 0.1 % that may be excluded
    v, f = rr.icosphere(2)
    pts = np.random.default_rng(800).uniform(-1, 1, (20000, 3)).astype(np.float32)
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    h = pts.astype(np.float64) @ n.T - (a * n).sum(1)[None]              # [points, faces]: the signed distance to every face plane
    clear = (np.abs(h) > 1e-6).all(1)
    assert 1 - clear.mean() <= 1e-3
    truth = (h < 0).all(1)
    assert 3000 < truth.sum() < 6000
    for nsamples in (1, 3):
        occ, votes = _occupancy((v, f), pts, nsamples)
        assert np.array_equal(occ[clear], truth[clear]), f"nsamples = {nsamples}: {(occ != truth)[clear].sum()} wrong"
        assert np.isin(votes, (0, nsamples)).all()


def test_inside_the_torus_is_the_sign_of_its_implicit_function():
    mesh = rr.torus()
    pts = np.random.default_rng(801).uniform(-1, 1, (20000, 3)).astype(np.float32)
    pts[:, 2] *= 0.4
    sd = rr.torus_implicit(pts)
    chord = rr.torus_chord_error()
    assert 0 < chord < 0.004
    clear = np.abs(sd) > chord
    truth = sd < 0
    assert clear.mean() > 0.9 and 1500 < truth[clear].sum()
    for nsamples in (1, 3):
        occ, votes = _occupancy(mesh, pts, nsamples)
        assert np.array_equal(occ[clear], truth[clear]), f"nsamples = {nsamples}: {(occ != truth)[clear].sum()} wrong"
        assert np.isin(votes, (0, nsamples)).all()


def test_votes_tell_an_open_mesh():
    pts = np.random.default_rng(802).uniform(-0.7, 0.7, (20000, 3)).astype(np.float32)
    _, votes = _occupancy(rr.wavy_sheet(), pts, 3)
    assert np.isin(votes, (1, 2)).mean() > 0.3          # below the sheet +z says inside, +x and +y (mostly) do not


# ---- 7: inside / outside against the voxeliser ----------------------------------------------------------------------------------
def test_occupancy_equals_the_solid_voxelisation_away_from_the_surface():
    from surfd_amd import meshprep, voxelize
    from surfd_amd.raycast import RaycastingScene
    v, f = (cu(x) for x in rr.torus())
    R = 32
    grid, odd = voxelize.voxelize_solid(v, f, resolution=R)
    assert odd == 0
    g = (torch.arange(R, device="cuda", dtype=torch.float32) + 0.5) * (2.0 / R) - 1.0
    centres = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).contiguous()
    far = meshprep.closest_points(v, f, centres)[0] > (2.0 / R) * 3 ** 0.5
    assert int(far.sum()) > 0.8 * R ** 3
    occ = RaycastingScene(v, f).compute_occupancy(centres) > 0
    dense = grid.dense().reshape(-1)
    assert torch.equal(occ[far], dense[far])
    assert 100 < int(occ[far].sum()) < int(far.sum())


# ---- 8: signed distance -------------------------------------------------------------------------------------------------------
def test_signed_distance_is_the_mesh_distance_with_the_sign_of_the_occupancy():
    from surfd_amd import meshprep
    from surfd_amd.raycast import RaycastingScene
    v, f = (cu(x) for x in rr.icosphere(3))
    q = cu(np.random.default_rng(810).uniform(-1, 1, (5000, 3)).astype(np.float32))
    scene = RaycastingScene(v, f)
    sd = scene.compute_signed_distance(q)
    dist = meshprep.MeshDistance(v, f).closest(q)[0]
    occ = scene.compute_occupancy(q)
    assert torch.equal(sd.abs().view(torch.int32), dist.view(torch.int32))
    assert torch.equal(sd < 0, occ > 0) and 500 < int((sd < 0).sum()) < 2500
    assert torch.equal(scene.compute_signed_distance(q, nsamples=3), sd)
    assert torch.equal(meshprep.is_inside(v, f, q), occ > 0)
    sdf, grad = meshprep.compute_sdf_and_gradients(v, f, q)
    udf, ugrad = meshprep.compute_udf_and_gradients(v, f, q)
    assert torch.equal(sdf.view(torch.int32), sd.view(torch.int32))
    assert torch.equal(grad.view(torch.int32), (torch.sign(sd)[:, None] * ugrad).view(torch.int32))
    assert float((sdf.abs() - udf).abs().max()) <= 4 * 2.0 ** -24 * 3 ** 0.5


def test_compute_sdf_from_mesh_follows_the_reference():
    from surfd_amd import meshprep
    v, f = (cu(x) for x in rr.icosphere(3))
    counts = [3000, 2000, 500, 500]
    torch.manual_seed(3)
    q, val, grad = meshprep.compute_sdf_from_mesh(v, f, num_surface_points=5000, num_queries_on_surface=700, num_queries_per_std=counts)
    n = 700 + sum(counts)
    assert q.shape == (n, 3) and val.shape == (n,) and grad.shape == (n, 3) and q.dtype == val.dtype == grad.dtype == torch.float32
    assert not val[:700].any() and not grad[:700].any()
    assert float(meshprep.closest_points(v, f, q[:700].contiguous())[0].max()) <= 4 * 2.0 ** -24           # the leading block lies on the surface
    assert float(val.min()) == -np.float32(0.1) and float(val.max()) == np.float32(0.1)                  # the clip, both signs
    sdf, g2 = meshprep.compute_sdf_and_gradients(v, f, q[700:].contiguous())
    assert torch.equal(val[700:], sdf.clamp(-0.1, 0.1)) and torch.equal(grad[700:], g2)
    assert float(q.abs().max()) <= 1.0
    norms = grad[700:].norm(dim=1)
    assert bool(((norms == 0) | ((norms - 1).abs() <= 1e-6)).all())
    # given queries are kept, and the BCE form is 1 - values / max_dist of the same seeded run
    torch.manual_seed(3)
    q2, bce, g3 = meshprep.compute_sdf_from_mesh(v, f, num_surface_points=5000, num_queries_on_surface=700, num_queries_per_std=counts,
                                                 convert_to_bce_labels=True)
    assert torch.equal(q2, q) and torch.equal(g3, grad)
    assert torch.equal(bce, 1 - val / 0.1) and float(bce.min()) == 0.0 and float(bce.max()) == 2.0 and bool((bce[:700] == 1).all())
    given = q[700:1700].contiguous()
    q3, v3, _ = meshprep.compute_sdf_from_mesh(v, f, num_queries_on_surface=10, input_queries=given, max_dist=0.05)
    assert torch.equal(q3[10:], given) and torch.equal(v3[10:], sdf[:1000].clamp(-0.05, 0.05))


# ---- 9: visibility ------------------------------------------------------------------------------------------------------------
def test_visible_on_the_cube():
    from surfd_amd.raycast import RaycastingScene
    scene = RaycastingScene(*(cu(x) for x in rr.cube()))
    a = cu(np.array([[-1, 0.1, 0.2], [-1, 0.1, 0.2], [-1, 0.1, 0.2], [0, 0, 0], [0, 0, 0], [-0.5, 0, 0], [-0.5, 0, 0]], dtype=np.float32))
    b = cu(np.array([[1, 0.1, 0.2], [-1, 0.9, -0.7], [-0.75, 2, 2], [0.25, 0.25, 0.25], [0, 0, 1], [-1, 0, 0], [-1, 0, 0]], dtype=np.float32))
    #    through the cube     same side       past a corner    both inside      inside -> out  starts on the surface (eps 0 / eps > 0)
    vis = scene.visible(a, b)
    assert vis.dtype == torch.bool and vis.tolist() == [False, True, True, True, False, False, False]
    assert scene.visible(a, b, eps=1e-3).tolist() == [False, True, True, True, False, True, True]
    assert scene.visible(b, a).tolist()[:5] == [False, True, True, True, False]
    assert torch.equal(scene.visible(a, b, brute_force=True), vis)
    occluded = scene.test_occlusions(torch.cat([a, b - a], 1), tmax=1.0)
    assert torch.equal(occluded, ~vis)


# ---- 10: the example --------------------------------------------------------------------------------------------------------
def test_preprocess_udfs_signed(tmp_path):
    v, f = rr.icosphere(3)
    mesh_udf_ref.write_obj(tmp_path / "ball.obj", v, f)
    env = dict(os.environ, PYTHONPATH=ROOT)
    counts = [3000, 2000, 500, 500]
    base = [sys.executable, os.path.join(ROOT, "examples", "preprocess_udfs.py"), str(tmp_path / "ball.obj"), "--num_surface_points", "6000",
            "--num_queries_per_std", *map(str, counts), "--seed", "5"]
    r = subprocess.run(base + ["--output_dir", str(tmp_path / "signed"), "--signed", "--num_queries_on_surface", "400"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(tmp_path / "signed" / "ball.npz")
    n = 400 + sum(counts)
    assert sorted(z.files) == ["coords", "gradients", "labels", "pcd", "triangles", "vertices"]
    assert z["coords"].shape == (n, 3) and z["labels"].shape == (n,) and z["gradients"].shape == (n, 3)
    lab = z["labels"]
    assert lab.dtype == np.float32 and not lab[:400].any() and not z["gradients"][:400].any()
    assert (lab < 0).sum() > 1000 and (lab > 0).sum() > 1000 and lab.min() >= -np.float32(0.1) and lab.max() <= np.float32(0.1)
    radius = np.linalg.norm(z["coords"][400:].astype(np.float64), axis=1)
    far = np.abs(radius - 0.75) > 0.01                       # away from the faceted surface the sign is that of |x| - 0.75
    assert far.sum() > 1000 and np.array_equal(lab[400:][far] < 0, radius[far] < 0.75)
