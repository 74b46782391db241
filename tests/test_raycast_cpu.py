"""Ray casting without a GPU: the numpy restatement of csrc/raycast.hip (tests/raycast_ref.py) against an independent fp64
Moeller-Trumbore, the exact ties of the contract (rays through edges and vertices, all coordinates dyadic so that the fp64
arithmetic is exact), the refusals of the wrappers, the exports and the registers of the kernels.

Measured with the seeds below (20 000 rays per mesh): no ray had to be excluded for a hit within 1e-9 (barycentric) of an
edge, hit / miss and the face agreed on every ray, and t differed from the rounded Moeller-Trumbore value by at most 1 ulp of
fp32 (largest relative deviation of the fp32 t from the fp64 one 5.96e-8 = 2^-24)."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raycast_ref as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WELL_CONDITIONED = {"icosphere": lambda: rr.icosphere(2), "torus": lambda: rr.torus(24, 12), "cube": rr.cube, "octahedron": rr.octahedron,
                    "wavy_sheet": lambda: rr.wavy_sheet(12)}


def ulps(a, b):
    """distance of two positive float32 arrays in units of the last place"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- 1: the restatement against Moeller-Trumbore --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WELL_CONDITIONED))
def test_restatement_against_moeller_trumbore(name):
    v, f = WELL_CONDITIONED[name]()
    rays = rr.random_rays(20000, seed=11 + sorted(WELL_CONDITIONED).index(name), extent=1.0)
    got = rr.cast(v, f, rays)
    mt = rr.mt_cast(v, f, rays, edge=1e-9)
    clear = ~mt["near_edge"]
    excluded = 1.0 - clear.mean()
    assert excluded <= 1e-3, f"{excluded:.4%} of the rays pass within 1e-9 of an edge: choose another seed"
    hit, mt_hit = got["tri"] >= 0, mt["tri"] >= 0
    assert hit.sum() > 2000
    assert np.array_equal(hit[clear], mt_hit[clear])
    assert np.array_equal(got["count"][clear], mt["count"][clear])
    both = hit & mt_hit & clear
    with np.errstate(invalid="ignore"):
        separated = both & ((mt["t2"] - mt["t"]) > 2.0 ** -20 * np.abs(mt["t"]))
    assert np.array_equal(got["tri"][separated], mt["tri"][separated])
    same_face = both & (got["tri"] == mt["tri"])
    worst_ulp = int(ulps(got["t"][same_face], mt["t"][same_face].astype(np.float32)).max())
    worst_rel = float(np.max(np.abs(got["t"][same_face].astype(np.float64) - mt["t"][same_face]) / np.abs(mt["t"][same_face])))
    print(f"{name}: {len(f)} triangles, {int(hit.sum())} hits, excluded {excluded:.4%}, faces compared {int(separated.sum())}, "
          f"max |t - t_mt| = {worst_ulp} ulp (relative {worst_rel:.3e})")
    assert worst_ulp <= 1
    # the barycentric weights and the normal of the winner, against the independent ones
    a, b, c = (v[f[got["tri"][same_face], k]].astype(np.float64) for k in range(3))
    o, d = rays[same_face, :3].astype(np.float64), rays[same_face, 3:].astype(np.float64)
    p = o + got["t"][same_face, None].astype(np.float64) * d
    uv = got["uv"][same_face].astype(np.float64)
    q = a + uv[:, :1] * (b - a) + uv[:, 1:] * (c - a)
    assert np.abs(p - q).max() <= 4 * 2.0 ** -24 * (np.abs(o).max() + 2 * np.abs(got["t"][same_face]).max())
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs(got["normal"][same_face] - n).max() <= 2.0 ** -23


# ---- 2: exact ties --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["cube", "cube_flipped"])
def test_cube_lattice_counts(mesh):
    v, f = rr.MESHES[mesh]()
    rays = rr.cube_lattice(-1.0)
    x, y = rays[:, 0], rays[:, 1]
    inside = (np.abs(x) < 0.5) & (np.abs(y) < 0.5)
    outside = (np.abs(x) > 0.5) | (np.abs(y) > 0.5)
    assert inside.sum() == 49 and outside.sum() == 88 and (x == y)[inside].sum() == 7       # the faces' diagonals are in
    cnt = rr.count(v, f, rays)
    assert (cnt % 2 == 0).all()
    assert (cnt[inside] == 2).all()
    assert (cnt[outside] == 0).all()
    assert np.isin(cnt[~inside & ~outside], (0, 2)).all()          # on the silhouette: the surface folds back
    got = rr.cast(v, f, rays)
    assert (got["t"][inside] == 0.5).all() and (got["tri"][inside] >= 0).all()
    half = rr.count(v, f, rr.cube_lattice(0.0))
    assert (half[inside] == 1).all()
    assert (half[outside] == 0).all()


def test_octahedron_vertices_and_edges():
    v, f = rr.octahedron()
    outside = rr.octahedron_rays(outside=True)
    assert len(outside) == (6 + 12) * 6
    cnt = rr.count(v, f, outside)
    assert (cnt % 2 == 0).all() and cnt.max() == 2 and (cnt == 2).sum() >= 18
    centre = rr.octahedron_rays(outside=False)
    assert len(centre) == 12
    assert (rr.count(v, f, centre) % 2 == 1).all()


def test_pair_ranges_and_bad_rays():
    v, f = rr.cube()
    ray = np.array([[0.125, 0.25, -1, 0, 0, 2]], dtype=np.float32)         # direction of length 2: t counts in its units
    got = rr.cast(v, f, ray)
    assert got["t"][0] == 0.25 and got["count"][0] == 2
    assert rr.cast(v, f, ray, tmin=0.25)["t"][0] == 0.25                   # tmin is included
    assert rr.cast(v, f, ray, tmax=0.25)["tri"][0] == -1                   # tmax is not
    assert rr.cast(v, f, ray, tmin=0.3)["t"][0] == 0.75
    assert rr.count(v, f, ray, tmin=0.3, tmax=0.75)[0] == 0
    n = got["normal"][0]
    assert tuple(n) == (0.0, 0.0, -1.0)                                    # by the winding (outward), not turned to the ray
    bad = np.repeat(ray, 5, axis=0)
    bad[1, 0], bad[2, 5], bad[3, 3:], bad[4, 1] = np.nan, np.inf, 0.0, -np.inf
    got = rr.cast(v, f, bad)
    assert got["tri"].tolist() == [got["tri"][0], -1, -1, -1, -1]
    assert np.isinf(got["t"][1:]).all() and not got["uv"][1:].any() and not got["normal"][1:].any() and not got["count"][1:].any()


# ---- 3: refusals ----------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from surfd_amd import meshprep, raycast
    v, f = (torch.from_numpy(x) for x in rr.cube())
    pts = torch.zeros(4, 3)
    rays = torch.zeros(4, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raycast.RaycastingScene(v, f)
    with pytest.raises(TypeError):
        raycast.RaycastingScene(v.double(), f)
    with pytest.raises(TypeError):
        raycast.RaycastingScene(v, f.float())
    with pytest.raises(ValueError):
        raycast.RaycastingScene(v[:, :2], f)
    with pytest.raises(ValueError):
        raycast.RaycastingScene(v, f[:0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raycast._check_rays(rays)
    with pytest.raises(ValueError):
        raycast._check_rays(pts)
    with pytest.raises(TypeError):
        raycast._check_rays(rays.double())
    for tmin in (-1e-30, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tmin"):
            raycast._check_range(tmin, 1.0)
    with pytest.raises(ValueError, match="tmax"):
        raycast._check_range(0.0, float("nan"))
    for bad in (0, 2, 4, -1, 1.0, True):
        with pytest.raises(ValueError, match="nsamples"):
            meshprep.is_inside(v, f, pts, nsamples=bad)
    for fn in (meshprep.is_inside, meshprep.compute_sdf_and_gradients):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(v, f, pts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshprep.compute_sdf_from_mesh(v, f)
    with pytest.raises(TypeError):
        meshprep.is_inside(v, f, pts.double())
    with pytest.raises(ValueError):
        meshprep.is_inside(v, f, rays)


def test_abi_errors_are_return_codes():
    from surfd_amd import _native as N
    lib = N.lib()
    for sym in ("surfd_rayscene_create", "surfd_rayscene_destroy", "surfd_rayscene_num_triangles", "surfd_rayscene_cast",
                "surfd_rayscene_count", "surfd_rayscene_skipped"):
        assert sym in N.EXPORTED_SYMBOLS
    h = C.c_void_p()
    assert lib.surfd_rayscene_create(None, 3, None, 1, None, C.byref(h)) == -1
    assert lib.surfd_rayscene_create(None, 0, None, 0, None, None) == -1
    assert lib.surfd_rayscene_num_triangles(None) == 0
    lib.surfd_rayscene_destroy(None)
    assert lib.surfd_rayscene_cast(None, None, 1, -1.0, 1.0, 0, None, None, None, None, None) == -1
    assert b"tmin" in lib.surfd_last_error()
    assert lib.surfd_rayscene_count(None, None, 1, 0.0, float("nan"), 0, None, None) == -1
    assert b"tmax" in lib.surfd_last_error()
    assert lib.surfd_rayscene_cast(None, None, 1, 0.0, 1.0, 4, None, None, None, None, None) == -1
    assert b"flags" in lib.surfd_last_error()
    assert lib.surfd_rayscene_cast(None, None, 1, 0.0, 1.0, 0, None, None, None, None, None) == -1
    assert b"handle" in lib.surfd_last_error()


def test_trace_kernels_stay_in_registers():
    """the counting form is a reduction that the loop vectoriser once interleaved 32 deep: 256 registers and 972 bytes of scratch"""
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    kernels = {k: v for k, v in mod.kernel_metadata().items() if "surfd::rc_" in k}
    assert sum("rc_trace_kernel" in k for k in kernels) == 4 and len(kernels) == 8
    for name, k in kernels.items():
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 128, name          # four 256-thread workgroups per CU
