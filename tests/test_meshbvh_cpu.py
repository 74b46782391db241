"""The mesh hierarchy without a GPU: the exports and refusals, the index arithmetic of csrc/meshbvh_layout.h (restated in
tests/bvh_ref.py, and the header itself under AddressSanitizer and UBSan in a stand-alone program), that both box tests are
conservative against the pair tests' own restatements, and the registers of the traversal kernels.

Measured with the seeds below: 271 379 accepted (ray, triangle) pairs (needles and triangles without area included) and
724 608 (query, triangle, box) triples, none excluded, no box skipped; the least room the query bound left,
(threshold - D2) / md_pair's result, was 3.0e-5 = 2^-15: the margin itself, reached by a query on the box."""
import ctypes as C
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_ref as br  # noqa: E402
import mesh_udf_ref as mr  # noqa: E402
import raycast_ref as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("surfd_rayscene_build_bvh", "surfd_rayscene_visits", "surfd_rayscene_bvh_info", "surfd_rayscene_bvh_read",
               "surfd_mesh_build_bvh", "surfd_mesh_closest_bvh", "surfd_mesh_visits", "surfd_mesh_bvh_info", "surfd_mesh_bvh_read")


# ---- 1: ABI and refusals --------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_bound():
    from surfd_amd import _native as N
    header = open(os.path.join(ROOT, "include", "surfd_hip.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym in N.EXPORTED_SYMBOLS and f"{sym}(" in header, sym
    for flag in ("#define SURFD_RAY_BVH 4", "#define SURFD_RAY_COUNT_VISITS 8", "#define SURFD_MESH_COUNT_VISITS 2"):
        assert flag in header
    from surfd_amd import build
    assert "meshbvh.hip" in build.SOURCES


def test_abi_errors_are_return_codes():
    from surfd_amd import _native as N
    lib = N.lib()
    a, b = C.c_int64(), C.c_int64()
    n = C.c_int()
    assert lib.surfd_rayscene_build_bvh(None, None) == -1 and b"handle" in lib.surfd_last_error()
    assert lib.surfd_mesh_build_bvh(None, None) == -1 and b"handle" in lib.surfd_last_error()
    assert lib.surfd_rayscene_visits(None, C.byref(a), C.byref(b), None) == -1
    assert lib.surfd_mesh_visits(None, C.byref(a), C.byref(b), None) == -1
    assert lib.surfd_rayscene_bvh_info(None, C.byref(n), None, None, None, 0) == -1
    assert lib.surfd_mesh_bvh_info(None, C.byref(n), None, None, None, 0) == -1
    assert lib.surfd_rayscene_bvh_read(None, None, None, None) == -1
    assert lib.surfd_mesh_bvh_read(None, None, None, None) == -1
    assert lib.surfd_mesh_closest_bvh(None, None, 1, 0, None, None, None, None, None) == -1 and b"handle" in lib.surfd_last_error()
    assert lib.surfd_mesh_closest_bvh(None, None, 1, 4, None, None, None, None, None) == -1 and b"flags" in lib.surfd_last_error()
    assert lib.surfd_mesh_closest_bvh(None, None, -1, 0, None, None, None, None, None) == -1
    # the hierarchy flag without a hierarchy is an error, never a fallback (here: without a handle at all)
    for flags in (4, 4 | 8, 4 | 2):
        assert lib.surfd_rayscene_cast(None, None, 1, 0.0, 1.0, flags, None, None, None, None, None) == -1
        assert b"not built" in lib.surfd_last_error()
        assert lib.surfd_rayscene_count(None, None, 1, 0.0, 1.0, flags, None, None) == -1
    assert lib.surfd_rayscene_cast(None, None, 1, 0.0, 1.0, 16, None, None, None, None, None) == -1 and b"unknown flags" in lib.surfd_last_error()


def test_wrappers_refuse_cpu_tensors_and_unknown_accel():
    from surfd_amd import meshprep, raycast
    v, f = (torch.from_numpy(x) for x in rr.cube())
    pts = torch.zeros(4, 3)
    for accel in ("tiles", "bvh"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            raycast.RaycastingScene(v, f, accel=accel)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            meshprep.MeshDistance(v, f, accel=accel)
        for fn in (meshprep.is_inside, meshprep.compute_sdf_and_gradients, meshprep.closest_points, meshprep.compute_udf_and_gradients):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                fn(v, f, pts, accel=accel)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            meshprep.point_to_mesh_distance(pts, v, f, accel=accel)
    for bad in ("BVH", "", None, 1, "brute"):
        with pytest.raises(ValueError, match="accel"):
            raycast.RaycastingScene(v, f, accel=bad)
        with pytest.raises(ValueError, match="accel"):
            meshprep.MeshDistance(v, f, accel=bad)
        for fn in (meshprep.is_inside, meshprep.compute_sdf_and_gradients, meshprep.closest_points, meshprep.compute_udf_and_gradients):
            with pytest.raises(ValueError, match="accel"):
                fn(v, f, pts, accel=bad)
        with pytest.raises(ValueError, match="accel"):
            meshprep.point_to_mesh_distance(pts, v, f, accel=bad)
        with pytest.raises(ValueError, match="accel"):
            meshprep.mesh_distance(v, f, v, f, accel=bad)
        with pytest.raises(ValueError, match="accel"):
            meshprep.compute_udf_from_mesh(v, f, accel=bad)
        with pytest.raises(ValueError, match="accel"):
            meshprep.compute_sdf_from_mesh(v, f, accel=bad)


def test_example_flags():
    sys.path.insert(0, ROOT)
    from examples import preprocess_udfs
    assert preprocess_udfs.parse(["x.obj"]).accel == "tiles"
    assert preprocess_udfs.parse(["x.obj", "--accel", "bvh"]).accel == "bvh"
    with pytest.raises(SystemExit):
        preprocess_udfs.parse(["x.obj", "--accel", "kd"])


# ---- 2: the layout --------------------------------------------------------------------------------------------------------------
def test_layout_restatement_for_every_leaf_count_to_2000():
    for nleaf in range(1, 2001):
        br.check_layout(nleaf)
    for nleaf in (4 ** 6 - 1, 4 ** 6, 4 ** 6 + 1, 2 * 4 ** 6 + 1):
        br.check_layout(nleaf)
    assert br.layout(1)["levels"] == 1 and br.layout(16)["levels"] == 1 and br.layout(17)["levels"] == 2
    assert br.layout(2 ** 28)["levels"] == 13                        # the largest F the handles accept: within the 16 of the mask word


def test_layout_header_under_sanitizers(tmp_path):
    """tools/meshbvh_layout_check.cpp includes only csrc/meshbvh_layout.h; host compiler, ASan + UBSan, run as a child"""
    cxx = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++") or "", shutil.which("hipcc") and
                            os.path.join(os.path.dirname(os.path.realpath(shutil.which("hipcc"))), "..", "llvm", "bin", "clang++") or "")
                if c and os.path.exists(c)), None)
    assert cxx is not None, "no clang++ (ROCm's llvm ships one, with the sanitizer runtimes)"
    exe = str(tmp_path / "meshbvh_layout_check")
    src = os.path.join(ROOT, "tools", "meshbvh_layout_check.cpp")
    assert '#include "../surfd_amd/csrc/meshbvh_layout.h"' in open(src).read()
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "ok" in r.stdout and "5058 leaf counts" in r.stdout


def test_build_restatement_invariants():
    """the numpy build: every triangle in one leaf, boxes hold what is below them, a NaN and a far vertex are never skipped"""
    v, f = rr.wavy_sheet(12)
    v = v.copy()
    v[5, 1] = np.nan
    v[100, 0] = 2.0 ** 21
    for corners, widths in (br.corners_absolute(v, f), br.corners_relative(v, f)):
        b = br.build(corners, widths)
        lay = b["lay"]
        ids = b["leaves"].ravel()
        assert sorted(ids[ids >= 0].tolist()) == list(range(len(f)))
        boxes = b["boxes"]
        bad = ~(np.abs(corners) <= 2.0 ** 20).all((1, 2))
        for leaf in range(lay["nleaf"]):
            lo, hi = boxes[leaf // 4, :3, leaf % 4], boxes[leaf // 4, 3:, leaf % 4]
            tri = b["leaves"][leaf]
            tri = tri[tri >= 0]
            if bad[tri].any():
                assert (lo == -np.inf).all() and (hi == np.inf).all()
            else:
                assert (corners[tri] >= lo).all() and (corners[tri] <= hi).all()
                p = v[f[tri]]                                            # the caller's own vertices, exact comparison
                assert (p >= lo).all() and (p <= hi).all()
        root = boxes[lay["off"][-1]]
        assert (root[:3].min(1) == -np.inf).all() and (root[3:].max(1) == np.inf).all()


# ---- 3: the box tests are conservative ------------------------------------------------------------------------------------------
def _accepted_pairs():
    """(rays [N, 6], triangle corners [N, 3, 3], t [N], a neighbour's corners [N, 3, 3]) of every pair rc_pair accepts"""
    per_mesh = {"icosphere": 8000, "torus": 5000, "cube": 90000, "octahedron": 90000, "wavy_sheet": 10000, "spliced_sheet": 40000,
                "cube_flipped": 90000}
    rays_out, tri_out, t_out, nb_out = [], [], [], []
    rng = np.random.default_rng(7)
    for k, (name, make) in enumerate(rr.MESHES.items()):
        v, f = make()
        sets = [rr.mixed_rays((v, f), per_mesh[name], 300 + k)]
        if name.startswith("cube"):
            sets += [rr.cube_lattice(-1.0), rr.cube_lattice(0.0)]
        if name == "octahedron":
            sets += [rr.octahedron_rays(True), rr.octahedron_rays(False)]
        rays = np.concatenate(sets)
        A, B, Cc = rr._corners(v, f)
        r = rr._Rays(rays)
        corners = v[f]
        for a, b in rr._blocks(len(rays), len(f)):
            hit, t, _, _, _ = rr._pair_block(r.part(a, b), A, B, Cc, 0.0, np.inf)
            i, j = np.nonzero(hit)
            rays_out.append(rays[a + i])
            tri_out.append(corners[j])
            t_out.append(t[i, j])
            nb_out.append(corners[rng.integers(0, len(f), len(j))])
    return np.concatenate(rays_out), np.concatenate(tri_out), np.concatenate(t_out), np.concatenate(nb_out)


def test_ray_box_test_never_skips_an_accepted_pair():
    rays, tri, t, nb = _accepted_pairs()
    print(f"{len(rays)} accepted (ray, triangle) pairs")
    assert len(rays) >= 200_000
    lo, hi = tri.min(1), tri.max(1)
    flat1 = ((hi - lo) == 0).sum(1) == 1
    assert flat1.sum() >= 20_000                                   # the cubes' faces: boxes without extent on one axis
    boxes = {"tight": (lo, hi), "with a neighbour": (np.minimum(lo, nb.min(1)), np.maximum(hi, nb.max(1)))}
    for what, (blo, bhi) in boxes.items():
        assert not br.ray_box_skip(blo, bhi, rays, 0.0, np.inf).any(), what                 # the counting form
        assert not br.ray_box_skip(blo, bhi, rays, 0.0, t).any(), what + ", the bound at the pair's own t"
        assert not br.ray_box_skip(blo, bhi, rays, t, np.inf).any(), what + ", tmin at the pair's own t"
    # and it does skip: the same boxes moved away along an axis the ray does not follow
    far = br.ray_box_skip(lo + np.float32(64), hi + np.float32(64), rays, 0.0, np.inf)
    assert far.mean() > 0.9
    behind = br.ray_box_skip(lo, hi, rays, 0.0, t * np.float32(0.5))
    assert behind.mean() > 0.5


def test_ray_box_test_on_boxes_without_extent_on_two_axes():
    """A triangle that is hit has area, so its box has extent on two axes at least.  A box that is a segment along an axis (what
    a leaf of triangles without area is) is tried on its own: rays with dyadic coordinates that meet the segment exactly at
    t = 2, in its interior and at its ends, along the other axes and diagonally, are never skipped, also with the bound at
    t = 2 itself; the same rays moved sideways by 2^-10 or more are."""
    rays, lo, hi, through = [], [], [], []
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        a = np.zeros(3); a[axis], a[u], a[w] = -0.5, 0.125, -0.375
        b = a.copy(); b[axis] = 0.5
        for s in (-0.5, 0.0, 0.25, 0.5):                           # the point of the segment that the ray meets
            for du, dw in ((1, 0), (0, 1), (-1, 0), (1, 1), (1, -2), (0.5, 0.25)):
                for da in (0.0, 1.0, -0.5):
                    for off in (0.0, 2.0 ** -10):
                        p = a.copy(); p[axis] = s
                        d = np.zeros(3); d[axis], d[u], d[w] = da, du, dw
                        o = p - 2.0 * d
                        big = max(abs(du), abs(dw))
                        o[u] += off * -dw / big                    # sideways in the plane across the segment
                        o[w] += off * du / big
                        rays.append(np.concatenate([o, d])); lo.append(a); hi.append(b); through.append(off == 0.0)
    rays, lo, hi, through = np.array(rays, np.float32), np.array(lo, np.float32), np.array(hi, np.float32), np.array(through)
    assert through.sum() == 216 and (lo != hi).sum(1).max() == 1
    skip = br.ray_box_skip(lo, hi, rays, 0.0, np.inf)
    assert not skip[through].any()
    assert not br.ray_box_skip(lo, hi, rays, 0.0, 2.0)[through].any()      # the hit is at t = 2 exactly: the tie is kept
    assert not br.ray_box_skip(lo, hi, rays, 2.0, np.inf)[through].any()
    assert br.ray_box_skip(lo, hi, rays, 0.0, 1.9921875)[through].all()
    assert br.ray_box_skip(lo, hi, rays, 2.0078125, np.inf)[through].all()
    assert skip[~through].all()


def test_point_box_bound_never_exceeds_the_pair_test():
    """>= 200 000 (query, triangle) pairs: the squared box distance D2 never exceeds best2 + 2^-16 (best2 + F2) when best2 is
    md_pair's own result for a triangle in the box, so no box that holds the lane's winner (or a tie) is ever skipped"""
    total, least = 0, np.inf
    rng = np.random.default_rng(3)
    for k, (name, (v, t, seed)) in enumerate(mr.test_meshes().items()):
        F = len(t)
        sel = rng.choice(F, min(F, 256), replace=False)
        v32 = np.asarray(v, np.float32)
        corners, widths = br.corners_relative(v32, t[sel])
        lo, hi = (corners - widths).min(1), (corners + widths).max(1)
        nb = rng.integers(0, len(sel), len(sel))
        lo2, hi2 = np.minimum(lo, lo[nb]), np.maximum(hi, hi[nb])
        R = mr.kernel_records_fp32(v32, t[sel])
        q = [mr.test_queries(name, v, t, seed)[:80],
             v32[t[sel][:40, 0]], v32[t[sel][:40, 1]], v32[t[sel][:40, 2]],                         # on vertices
             np.stack([lo[:24, 0], 0.5 * (lo[:24, 1] + hi[:24, 1]), 0.5 * (lo[:24, 2] + hi[:24, 2])], 1),   # on box faces
             np.stack([0.5 * (lo[:24, 0] + hi[:24, 0]), hi[:24, 1], hi[:24, 2]], 1),                # on box edges
             (rng.normal(size=(24, 3)) * 1e6).astype(np.float32),                                   # 1e6 away
             (rng.normal(size=(24, 3)) * 30).astype(np.float32)]
        q = np.concatenate(q).astype(np.float32)
        with np.errstate(all="ignore"):
            dd, _ = mr._pair_fp32(R, q[:, None])                                                    # [Q, F]
        for blo, bhi in ((lo, hi), (lo2, hi2)):
            D2, F2 = br.point_box(blo[None], bhi[None], q[:, None])
            bound = br.point_box_bound(D2, F2, dd)
            assert (D2 <= bound).all(), name
            assert not br.point_box_skip(blo[None], bhi[None], q[:, None], dd).any(), name
            with np.errstate(all="ignore"):
                room = np.where(dd > 0, (bound.astype(np.float64) - D2) / np.where(dd > 0, dd, 1), np.inf)
            least = min(least, float(room.min()))
            total += dd.size
        # and the bound bites: against a best distance of a tenth of the box's, far boxes are skipped
        D2, F2 = br.point_box(lo[None], hi[None], q[-24:, None])
        assert br.point_box_skip(lo[None], hi[None], q[-24:, None], D2 * np.float32(0.01)).all()
    print(f"{total} (query, triangle, box) pairs, the least room (bound - D2) / dd = {least:.3e}")
    assert total >= 200_000 and least >= 0


# ---- 4: the kernels' registers --------------------------------------------------------------------------------------------------
def test_traversal_kernels_stay_in_registers():
    """the walk keeps level, node and one 64-bit mask: no stack, no private array, so no scratch; 128 registers = four
    256-thread workgroups per CU, the bound DESIGN.md section 8.11 states (as for rc_trace_kernel)"""
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    meta = mod.kernel_metadata()
    ray = {k: v for k, v in meta.items() if "surfd::bvr_" in k}
    pts = {k: v for k, v in meta.items() if "surfd::bvm_" in k}
    assert sum("bvr_trace_kernel" in k for k in ray) == 2 and len(ray) == 2
    assert sum("bvm_closest_kernel" in k for k in pts) == 1 and len(pts) == 1
    assert sum("surfd::bvh_" in k for k in meta) == 4                  # bounds, codes, leaves, levels
    for name, k in {**ray, **pts}.items():
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 128, name
    # the existing paths keep their kernels: the hierarchy added none under their prefixes
    assert sum("surfd::rc_" in k for k in meta) == 8 and sum("surfd::md_" in k for k in meta) == 5
