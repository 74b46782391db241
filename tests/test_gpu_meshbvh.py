"""The mesh hierarchy (csrc/meshbvh.hip, accel="bvh") on the GPU: rays and closest points through it against brute force bit for
bit (and against tests/raycast_ref.py up to 513 triangles), on each side of a leaf (L = 4), of a node (L W = 16) and of the
levels above, on degenerate builds, the hierarchy's own invariants from the read-out against tests/bvh_ref.py, independence of
order, subsets, repeats and handles, that it culls, and the drivers."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_ref as br  # noqa: E402
import mesh_udf_ref as mr  # noqa: E402
import raycast_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
BRUTE, BVH, VISITS = 1, 4, 8
L, W = br.L, br.W


def cu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def _read(N, h, info, read):
    levels, leaves, nodes = C.c_int(), C.c_int(), C.c_int()
    sizes = (C.c_int32 * 16)()
    N.check(info(h, C.byref(levels), C.byref(leaves), C.byref(nodes), sizes, 16))
    boxes = torch.empty(nodes.value, 6, 4, device="cuda")
    tri = torch.empty(leaves.value, 4, device="cuda", dtype=torch.int32)
    N.check(read(h, N.ptr(boxes), N.ptr(tri), N.stream()))
    return [int(sizes[k]) for k in range(levels.value)], boxes.cpu().numpy(), tri.cpu().numpy()


class RawScene:
    """the C ABI as it is: triangles and rays in the order given, the hierarchy built"""

    def __init__(self, v, f):
        from surfd_amd import _native as N
        self.N = N
        self.v, self.f = cu(v), cu(f, torch.int32)
        self.h = C.c_void_p()
        N.check(N.lib().surfd_rayscene_create(N.ptr(self.v), len(v), N.ptr(self.f), len(f), N.stream(), C.byref(self.h)))
        N.check(N.lib().surfd_rayscene_build_bvh(self.h, N.stream()))
        N.check(N.lib().surfd_rayscene_build_bvh(self.h, N.stream()))          # idempotent

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

    def read(self):
        return _read(self.N, self.h, self.N.lib().surfd_rayscene_bvh_info, self.N.lib().surfd_rayscene_bvh_read)

    def __del__(self):
        self.N.lib().surfd_rayscene_destroy(self.h)


class RawMesh:
    """surfd_mesh through the C ABI, the hierarchy built"""

    def __init__(self, v, f, build=True):
        from surfd_amd import _native as N
        self.N = N
        self.v, self.f = cu(v), cu(f, torch.int32)
        self.h = C.c_void_p()
        N.check(N.lib().surfd_mesh_create(N.ptr(self.v), len(v), N.ptr(self.f), len(f), N.stream(), C.byref(self.h)))
        if build:
            N.check(N.lib().surfd_mesh_build_bvh(self.h, N.stream()))
            N.check(N.lib().surfd_mesh_build_bvh(self.h, N.stream()))

    def closest(self, q, bvh=True):
        N, Q = self.N, len(q)
        qd = cu(q)
        d = torch.full((Q,), -7.0, device="cuda")
        p = torch.full((Q, 3), -7.0, device="cuda")
        j = torch.full((Q,), -7, device="cuda", dtype=torch.int32)
        fn = N.lib().surfd_mesh_closest_bvh if bvh else N.lib().surfd_mesh_closest
        N.check(fn(self.h, N.ptr(qd), Q, 0 if bvh else BRUTE, N.ptr(d), N.ptr(p), N.ptr(j), None, N.stream()))
        torch.cuda.synchronize()
        return d.cpu().numpy(), p.cpu().numpy(), j.cpu().numpy()

    def read(self):
        return _read(self.N, self.h, self.N.lib().surfd_mesh_bvh_info, self.N.lib().surfd_mesh_bvh_read)

    def __del__(self):
        self.N.lib().surfd_mesh_destroy(self.h)


def same_bits(got, ref, what=""):
    for k in ("t", "tri", "uv", "normal", "count"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(1))
        assert bad.size == 0, f"{what}: {k} differs for {bad.size} of {len(a)} rays, first {bad[:5]}: {a[bad[:3]]} != {b[bad[:3]]}"


def same_closest(a, b, what=""):
    for x, y, k in zip(a, b, ("dist", "point", "tri")):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        bad = np.flatnonzero((x.view(np.uint32) != y.view(np.uint32)).reshape(len(x), -1).any(1))
        assert bad.size == 0, f"{what}: {k} differs for {bad.size} of {len(x)} queries, first {bad[:5]}: {x[bad[:3]]} != {y[bad[:3]]}"


def bad_rays(mesh, R, seed):
    """mixed rays with a NaN, an Inf, a zero direction, an origin beyond 2^20 and a direction below 2^-20 spliced in: the last
    two are legal rays that hit what they hit, untamed, so the hierarchy may skip nothing for them"""
    rays = rr.mixed_rays(mesh, R, seed).copy()
    rays[0, 0], rays[5, 4], rays[7, 3:], rays[9, 2] = np.nan, np.inf, 0.0, -np.inf
    rays[11, :3] = (2.0 ** 21, 0.0, 0.0); rays[11, 3:] = (-1.0, 0.0, 0.0)                  # towards the mesh from far away
    rays[13, :3] = (0.0, 3.0 * 2.0 ** 20, 0.0); rays[13, 3:] = (0.0, -2.0 ** 20, 0.0)
    rays[15, 3:] *= np.float32(2.0 ** -30)
    rays[17, :3] = (0.0, 0.0, -2.0); rays[17, 3:] = (0.0, 0.0, 2.0 ** -25)
    rays[19, 3:] = (2.0 ** -140, 1.0, 2.0 ** -60)                                          # nearly parallel to an axis
    return rays


# ---- the ray cases: name -> (mesh, rays, tmin, tmax) ------------------------------------------------------------------------------
def _ray_cases():
    out = {}
    big = {"icosphere": rr.icosphere(3), "torus": rr.torus(), "cube": rr.cube(), "octahedron": rr.octahedron(), "wavy_sheet": rr.wavy_sheet(),
           "spliced_sheet": rr.spliced_sheet(), "cube_flipped": rr.cube_flipped()}
    for i, (name, mesh) in enumerate(big.items()):
        out[f"mesh-{name}"] = (mesh, rr.mixed_rays(mesh, 257, 100 + 3 * i), 0.0, INF)
    wide = rr.torus(96, 88)                                              # 16 896 triangles
    for F in (1, 2, L, L + 1, L * W, L * W + 1, L * W * W - 1, L * W * W + 1, 255, 256, 257, 4097, 16385):
        mesh = rr.first_faces(wide, F)
        out[f"F-{F}"] = (mesh, rr.mixed_rays(mesh, 65, 200 + F), 0.0, INF)
    ico = rr.icosphere(2)
    for R in (1, 63, 64, 65, 257):
        out[f"R-{R}"] = (ico, rr.mixed_rays(ico, R, 400 + R), 0.0, INF)
    out["R-5000"] = (big["icosphere"], rr.mixed_rays(big["icosphere"], 5000, 450), 0.0, INF)
    out["range"] = (big["torus"], rr.mixed_rays(big["torus"], 257, 500), 0.3, 1.2)
    for name in ("cube", "cube_flipped"):
        for z0 in (-1.0, 0.0):
            out[f"lattice-{name}-{z0}"] = (big[name], rr.cube_lattice(z0), 0.0, INF)
    out["octahedron-outside"] = (big["octahedron"], rr.octahedron_rays(True), 0.0, INF)
    out["octahedron-centre"] = (big["octahedron"], rr.octahedron_rays(False), 0.0, INF)
    out["bad-rays-torus"] = (big["torus"], bad_rays(big["torus"], 257, 510), 0.0, INF)
    out["bad-rays-cube"] = (big["cube"], bad_rays(big["cube"], 65, 511), 0.0, INF)
    return out


RAY_CASES = _ray_cases()


@pytest.mark.parametrize("name", sorted(RAY_CASES))
def test_rays_equal_brute_force_bit_for_bit(name):
    (v, f), rays, tmin, tmax = RAY_CASES[name]
    scene = RawScene(v, f)
    brute = scene.cast(rays, tmin, tmax, flags=BRUTE)
    same_bits(scene.cast(rays, tmin, tmax, flags=BVH), brute, f"{name}, hierarchy")
    same_bits(scene.cast(rays, tmin, tmax, flags=BVH | BRUTE), brute, f"{name}, both flags: brute force wins")
    if len(f) <= 513:
        same_bits(brute, rr.cast(v, f, rays, tmin, tmax), f"{name}, restatement")
    print(f"{name}: F = {len(f)}, R = {len(rays)}, {int((brute['tri'] >= 0).sum())} hits, counts up to {int(brute['count'].max())}")
    assert name.startswith(("bad", "F-1", "F-2", "R-1")) or (brute["tri"] >= 0).any()


def test_hierarchy_flag_without_a_build_is_an_error():
    from surfd_amd import _native as N
    v, f = rr.cube()
    vd, fd = cu(v), cu(f, torch.int32)
    h = C.c_void_p()
    N.check(N.lib().surfd_rayscene_create(N.ptr(vd), len(v), N.ptr(fd), len(f), N.stream(), C.byref(h)))
    rays = cu(rr.cube_lattice(-1.0))
    cnt = torch.zeros(len(rays), device="cuda", dtype=torch.int32)
    assert N.lib().surfd_rayscene_count(h, N.ptr(rays), len(rays), 0.0, INF, BVH, N.ptr(cnt), N.stream()) == -2
    assert b"not built" in N.lib().surfd_last_error()
    a, b = C.c_int64(), C.c_int64()
    assert N.lib().surfd_rayscene_visits(h, C.byref(a), C.byref(b), N.stream()) == -2
    assert N.lib().surfd_rayscene_count(h, N.ptr(rays), len(rays), 0.0, INF, BVH | BRUTE, N.ptr(cnt), N.stream()) == 0    # brute force needs none
    N.lib().surfd_rayscene_destroy(h)
    m = RawMesh(v, f, build=False)
    q = cu(np.zeros((3, 3), np.float32))
    d = torch.zeros(3, device="cuda")
    assert N.lib().surfd_mesh_closest_bvh(m.h, N.ptr(q), 3, 0, N.ptr(d), None, None, None, N.stream()) == -2
    assert b"not built" in N.lib().surfd_last_error()
    assert N.lib().surfd_mesh_closest_bvh(m.h, N.ptr(q), 3, BRUTE, N.ptr(d), None, None, None, N.stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), np.full(3, 0.5, np.float32))


# ---- degenerate builds ----------------------------------------------------------------------------------------------------------
def _degenerate_meshes():
    out = {}
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.float32)
    out["identical"] = (v, np.tile(np.array([[0, 1, 2]]), (37, 1)))                       # every code equal
    g = np.linspace(-0.75, 0.75, 9)
    x, y = np.meshgrid(g, g, indexing="ij")
    pv = np.stack([x, y, np.full_like(x, 0.25)], -1).reshape(-1, 3).astype(np.float32)     # every box flat in z
    pf = []
    for i in range(8):
        for j in range(8):
            a, b, c, d = i * 9 + j, (i + 1) * 9 + j, (i + 1) * 9 + j + 1, i * 9 + j + 1
            pf += [(a, b, c), (a, c, d)]
    out["planar"] = (pv, np.array(pf))
    fv, ff = rr.wavy_sheet(12)
    fv = fv.copy()
    fv[17, 0] = 2.0 ** 21
    out["far-vertex"] = (fv, ff)
    nv, nf = rr.wavy_sheet(12)
    nv = nv.copy()
    nv[40, 2] = np.nan
    nv[90, 1] = np.inf
    out["nan-vertex"] = (nv, nf)
    return out


DEGENERATE = _degenerate_meshes()


def _planar_rays():
    """rays that lie in the plane z = 1/4 and start on it (inside and outside the sheet), rays across it, rays along it just off"""
    rng = np.random.default_rng(5)
    n = 120
    o = np.stack([rng.integers(-8, 9, n) / 8.0, rng.integers(-8, 9, n) / 8.0, np.full(n, 0.25)], 1)
    d = np.stack([rng.integers(-2, 3, n) / 2.0, rng.integers(-2, 3, n) / 2.0, np.zeros(n)], 1)
    d[(d == 0).all(1), 0] = 1.0
    in_plane = np.concatenate([o, d], 1)
    across = in_plane.copy()
    across[:, 2], across[:, 5] = -1.0, 1.0
    off = in_plane.copy()
    off[:, 2] += 2.0 ** -12
    return np.concatenate([in_plane, across, off]).astype(np.float32)


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_builds_equal_brute_force(name):
    v, f = DEGENERATE[name]
    rays = np.concatenate([rr.mixed_rays((np.nan_to_num(v, nan=0.0, posinf=0.0), f), 257, 900), _planar_rays(), rr.cube_lattice(-1.0)])
    scene = RawScene(v, f)
    brute = scene.cast(rays, flags=BRUTE)
    same_bits(scene.cast(rays, flags=BVH), brute, name)
    same_bits(scene.cast(rays, 0.25, 1.5, flags=BVH), scene.cast(rays, 0.25, 1.5, flags=BRUTE), name + ", window")
    assert (brute["tri"] >= 0).sum() > 50
    sizes, boxes, leaves = scene.read()
    if name in ("far-vertex", "nan-vertex"):                               # the root holds a box that is never skipped
        root = boxes[-1]
        assert (root[:3] == -np.inf).any() and (root[3:] == np.inf).any()
    mesh = RawMesh(v, f)
    q = np.concatenate([mr.pipeline_queries(np.nan_to_num(v, nan=0.0, posinf=0.0), f, 77, per_sigma=200, uniform=100, cloud=200),
                        np.nan_to_num(v, nan=0.0, posinf=0.0)[:64]]).astype(np.float32)
    same_closest(mesh.closest(q), mesh.closest(q, bvh=False), name)


# ---- closest points -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _closest_cases():
    out = {}
    for name, (v, t, seed) in mr.test_meshes().items():
        q = mr.test_queries(name, v, t, seed)[::4]
        out[name] = (v, t, np.concatenate([q, np.asarray(v, np.float32)[::7]]))          # pipeline queries, and on the vertices
    ico = rr.icosphere(3)
    far = (np.random.default_rng(8).normal(size=(64, 3)) * 1e4).astype(np.float32)
    out["icosphere-centre"] = (*ico, np.concatenate([np.zeros((70, 3), np.float32), ico[0], far]))       # a mass tie, vertices, far away
    cube = rr.cube()
    out["cube-centre"] = (*cube, np.concatenate([np.zeros((3, 3), np.float32), cube[0], far[:5]]))
    sheet = mr.wavy_sheet(100)                                                             # 19 602 triangles
    for F in (1, 2, L, L + 1, L * W, L * W + 1, L * W * W - 1, L * W * W + 1, 255, 256, 257, 4097, 16385):
        v, t = sheet[0], sheet[1][:F]
        out[f"F-{F}"] = (v, t, np.concatenate([mr.pipeline_queries(v, t, 600 + F, per_sigma=20, uniform=5, cloud=30), v[t[:, 0]][:40]]))
    for Q in (1, 63, 64, 65, 257, 5000):
        v, t = sheet[0], sheet[1][:5000]
        out[f"Q-{Q}"] = (v, t, mr.pipeline_queries(v, t, 700 + Q, per_sigma=1600, uniform=400, cloud=1500)[:Q])
    return out


@pytest.mark.parametrize("name", sorted(["wavy_sheet", "convex_polyhedron", "spliced_sheet", "zero_area", "needles", "icosphere-centre",
                                          "cube-centre"] + [f"F-{F}" for F in (1, 2, 4, 5, 16, 17, 63, 65, 255, 256, 257, 4097, 16385)] +
                                         [f"Q-{Q}" for Q in (1, 63, 64, 65, 257, 5000)]))
def test_closest_points_equal_brute_force_bit_for_bit(name):
    from surfd_amd import meshprep
    v, t, q = _closest_cases()[name]
    assert len(q) >= 1
    raw = RawMesh(v, t)                                                     # the handle's order is the caller's: no Morton sort
    same_closest(raw.closest(q), raw.closest(q, bvh=False), f"{name}, C ABI")
    md = meshprep.MeshDistance(cu(v), cu(t), accel="bvh")
    a = md.closest(cu(q))
    b = md.closest(cu(q), brute_force=True)
    c = meshprep.MeshDistance(cu(v), cu(t)).closest(cu(q))
    for x, y, z, what in zip(a, b, c, ("dist", "point", "tri")):
        assert torch.equal(x, y) and torch.equal(x, z), (name, what)
    if name.endswith("centre"):
        n = 70 if name.startswith("ico") else 3
        assert len(set(a[2][:n].tolist())) == 1 and float(a[0][:n].max()) == float(a[0][:n].min())     # the mass tie goes one way
    if name == "zero_area":
        d = md.closest(cu(np.asarray(v, np.float32)))[0]
        assert bool(torch.isfinite(d).all())


# ---- the hierarchy's invariants ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 5, 17, 65, 257, 4097, 16385])
def test_hierarchy_invariants_from_the_read_out(F):
    wide = rr.first_faces(rr.torus(96, 88), F)
    v, f = wide
    f = f[np.random.default_rng(F).permutation(len(f))]                    # no order to start from
    for kind in ("rays", "points"):
        handle = RawScene(v, f) if kind == "rays" else RawMesh(v, f)
        sizes, boxes, leaves = handle.read()
        corners, widths = br.corners_absolute(v, f) if kind == "rays" else br.corners_relative(v, f)
        ref = br.build(corners, widths)
        assert sizes == ref["lay"]["size"], kind
        ids = leaves.ravel()
        assert sorted(ids[ids >= 0].tolist()) == list(range(F)) and (ids[F:] == -1).all(), kind
        assert np.array_equal(leaves, ref["leaves"]), f"{kind}: the leaf order is not the stable sort of the restated codes"
        if kind == "rays":
            assert np.array_equal(boxes.view(np.uint32), ref["boxes"].view(np.uint32))     # min / max: nothing is rounded
        else:
            fin = np.isfinite(ref["boxes"])
            assert np.array_equal(np.isfinite(boxes), fin) and np.array_equal(boxes[~fin], ref["boxes"][~fin])
            assert np.abs(boxes[fin] - ref["boxes"][fin]).max() <= 2.0 ** -22 * 2             # the widening's own last bit (fmaf)
        # every box holds, by exact comparison, the caller's vertices of all triangles below it
        lay = ref["lay"]
        tri_v = np.asarray(v, np.float32)[f]                               # [F, 3, 3]
        lo = np.full((lay["nleaf"] * L, 3), np.inf, np.float32)
        hi = np.full((lay["nleaf"] * L, 3), -np.inf, np.float32)
        lo[:F], hi[:F] = tri_v[ids[:F]].min(1), tri_v[ids[:F]].max(1)
        lo, hi = lo.reshape(-1, L, 3).min(1), hi.reshape(-1, L, 3).max(1)  # per leaf
        for k in range(lay["levels"]):
            n = lay["size"][k]
            lo = np.concatenate([lo, np.full((n * W - len(lo), 3), np.inf, np.float32)]).reshape(n, W, 3)
            hi = np.concatenate([hi, np.full((n * W - len(hi), 3), -np.inf, np.float32)]).reshape(n, W, 3)
            got = boxes[lay["off"][k]:lay["off"][k] + n]
            there = lo[..., 0] <= hi[..., 0]
            assert np.array_equal(got[:, 0] <= got[:, 3], there), (kind, k)              # the children that exist
            assert (got[:, :3].transpose(0, 2, 1)[there] <= lo[there]).all() and (got[:, 3:].transpose(0, 2, 1)[there] >= hi[there]).all(), (kind, k)
            lo, hi = lo.min(1), hi.max(1)


# ---- independence ---------------------------------------------------------------------------------------------------------------
def _eq(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_independent_of_order_subsets_repeats_and_handles():
    from surfd_amd.meshprep import MeshDistance
    from surfd_amd.raycast import RaycastingScene
    v, f = rr.icosphere(3)
    rays = rr.mixed_rays((v, f), 1000, 700)
    q = mr.pipeline_queries(v, f, 71, per_sigma=300, uniform=100, cloud=300)
    scene = RaycastingScene(cu(v), cu(f), accel="bvh")
    base = scene.cast_rays(cu(rays))
    base_count = scene.count_intersections(cu(rays))
    dist = scene.mesh_distance()
    assert dist.accel == "bvh"
    base_q = dist.closest(cu(q))
    tiles = RaycastingScene(cu(v), cu(f))
    for k, x in tiles.cast_rays(cu(rays)).items():
        assert _eq(base[k], x), k
    assert torch.equal(tiles.count_intersections(cu(rays)), base_count)
    rng = np.random.default_rng(1)
    pf, pr, pq = rng.permutation(len(f)), rng.permutation(len(rays)), rng.permutation(len(q))
    other = RaycastingScene(cu(v), cu(f[pf]), accel="bvh")
    got = other.cast_rays(cu(rays[pr]))
    back = torch.from_numpy(np.argsort(pr)).cuda()
    ids = got["primitive_ids"][back]
    ids = torch.where(ids >= 0, torch.from_numpy(pf).cuda()[ids.clamp_min(0)], ids)
    # a tie in t between two triangles goes to the first in the Morton order, which the permutation keeps (the sort is stable
    # only within equal codes: an exact tie between triangles of equal code could change sides; none occurs with these rays)
    assert torch.equal(ids, base["primitive_ids"])
    for k in ("t_hit", "primitive_uvs", "primitive_normals"):
        assert _eq(got[k][back], base[k]), k
    assert torch.equal(other.count_intersections(cu(rays[pr]))[back], base_count)
    gq = MeshDistance(cu(v), cu(f[pf]), accel="bvh").closest(cu(q[pq]))
    backq = torch.from_numpy(np.argsort(pq)).cuda()
    assert _eq(gq[0][backq], base_q[0])
    # subsets alone
    alone = scene.cast_rays(cu(rays[100:164]))
    for k in base:
        assert _eq(alone[k], base[k][100:164]), k
    assert torch.equal(scene.count_intersections(cu(rays[::3])), base_count[::3])
    sub = dist.closest(cu(q[50:177]))
    for x, y in zip(sub, base_q):
        assert _eq(x, y[50:177])
    # ten repeats, and a second handle of the same mesh
    for i in range(10):
        again = scene.cast_rays(cu(rays))
        assert all(_eq(again[k], base[k]) for k in base), i
        assert torch.equal(scene.count_intersections(cu(rays)), base_count), i
        assert all(_eq(x, y) for x, y in zip(dist.closest(cu(q)), base_q)), i
    second = RaycastingScene(cu(v), cu(f), accel="bvh")
    assert all(_eq(x, base[k]) for k, x in second.cast_rays(cu(rays)).items())
    assert all(_eq(x, y) for x, y in zip(second.mesh_distance().closest(cu(q)), base_q))
    a, b = scene.read_bvh(), second.read_bvh()
    assert a["level_sizes"] == b["level_sizes"] and torch.equal(a["leaves"], b["leaves"]) and _eq(a["boxes"], b["boxes"])


# ---- it culls ---------------------------------------------------------------------------------------------------------------------
def test_the_hierarchy_culls():
    from surfd_amd.meshprep import MeshDistance
    from surfd_amd.raycast import RaycastingScene
    v, f = rr.wavy_sheet(92)
    assert len(f) == 16562
    rays = cu(rr.random_rays(5000, 31))
    tiles = RaycastingScene(cu(v), cu(f))
    want = tiles.count_intersections(rays, count_skipped=True)
    tile_pairs = (tiles.last_total_tiles - tiles.last_skipped_tiles) * 32 * 64
    tree = RaycastingScene(cu(v), cu(f), accel="bvh")
    got = tree.count_intersections(rays, count_visits=True)
    assert torch.equal(got, want) and int(want.sum()) > 500
    print(f"crossing counts, 5000 rays, 16 562 triangles: hierarchy {tree.last_pair_tests} pair tests and {tree.last_box_tests} box tests "
          f"({tree.last_pair_tests / 5000:.1f} and {tree.last_box_tests / 5000:.1f} per ray); tiles {tile_pairs} pair tests "
          f"({tile_pairs / 5000:.0f} per ray): 1 / {tile_pairs / max(tree.last_pair_tests, 1):.0f}")
    assert 0 < tree.last_pair_tests <= tile_pairs / 10
    cast = tree.cast_rays(rays, count_visits=True)
    print(f"first hits: {tree.last_pair_tests / 5000:.1f} pair tests and {tree.last_box_tests / 5000:.1f} box tests per ray")
    assert all(_eq(cast[k], x) for k, x in tiles.cast_rays(rays).items())
    with pytest.raises(ValueError, match="count_visits"):
        tiles.count_intersections(rays, count_visits=True)
    with pytest.raises(ValueError, match="count_visits"):
        tree.count_intersections(rays, brute_force=True, count_visits=True)
    q = cu(mr.pipeline_queries(v, f, 33, per_sigma=1500, uniform=500, cloud=1500))
    md = MeshDistance(cu(v), cu(f))
    want = md.closest(q, count_skipped=True)
    tile_pairs = (md.last_total_tiles - md.last_skipped_tiles) * 32 * 64
    mt = MeshDistance(cu(v), cu(f), accel="bvh")
    got = mt.closest(q, count_visits=True)
    assert all(_eq(x, y) for x, y in zip(got, want))
    print(f"closest points, {len(q)} queries: hierarchy {mt.last_pair_tests / len(q):.1f} pair tests and {mt.last_box_tests / len(q):.1f} box "
          f"tests per query; tiles {tile_pairs / len(q):.0f} pair tests per query: 1 / {tile_pairs / max(mt.last_pair_tests, 1):.0f}")
    assert 0 < mt.last_pair_tests <= tile_pairs / 10


# ---- the drivers ----------------------------------------------------------------------------------------------------------------
def test_drivers_give_the_same_tensors():
    from surfd_amd import meshprep
    v, f = (cu(x) for x in rr.icosphere(3))
    counts = [3000, 2000, 500, 500]
    out = {}
    for accel in ("tiles", "bvh"):
        torch.manual_seed(3)
        sdf = meshprep.compute_sdf_from_mesh(v, f, num_surface_points=5000, num_queries_on_surface=700, num_queries_per_std=counts, accel=accel)
        torch.manual_seed(3)
        udf = meshprep.compute_udf_from_mesh(v, f, num_surface_points=5000, num_queries_per_std=counts, accel=accel)
        out[accel] = sdf + udf
    for a, b in zip(out["tiles"], out["bvh"]):
        assert torch.equal(a, b)
    pts = out["tiles"][0][:2000].contiguous()
    assert torch.equal(meshprep.is_inside(v, f, pts, accel="bvh"), meshprep.is_inside(v, f, pts))
    assert torch.equal(meshprep.is_inside(v, f, pts, nsamples=3, accel="bvh"), meshprep.is_inside(v, f, pts, nsamples=3))
    assert torch.equal(meshprep.point_to_mesh_distance(pts, v, f, accel="bvh"), meshprep.point_to_mesh_distance(pts, v, f))
    for x, y in zip(meshprep.closest_points(v, f, pts, accel="bvh"), meshprep.closest_points(v, f, pts)):
        assert torch.equal(x, y)
    g1, g2 = (torch.Generator(device="cuda").manual_seed(9) for _ in range(2))
    w = cu(rr.torus()[0]), cu(rr.torus()[1])
    assert meshprep.mesh_distance(v, f, *w, n=4000, generator=g1, accel="bvh") == meshprep.mesh_distance(v, f, *w, n=4000, generator=g2)
    with pytest.raises(ValueError, match="accel"):
        meshprep.compute_sdf_from_mesh(v, f, accel="kd")


def test_preprocess_udfs_writes_the_same_bytes(tmp_path):
    v, f = rr.icosphere(3)
    assert len(f) == 1280
    mr.write_obj(tmp_path / "ball.obj", v, f)
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, os.path.join(ROOT, "examples", "preprocess_udfs.py"), str(tmp_path / "ball.obj"), "--num_surface_points", "6000",
            "--num_queries_per_std", "3000", "2000", "500", "500", "--seed", "3", "--signed", "--num_queries_on_surface", "400"]
    digest = {}
    for name, extra in (("plain", []), ("bvh", ["--accel", "bvh"])):
        r = subprocess.run(base + ["--output_dir", str(tmp_path / name)] + extra, capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        digest[name] = hashlib.sha256(open(tmp_path / name / "ball.npz", "rb").read()).hexdigest()
    assert digest["plain"] == digest["bvh"]
