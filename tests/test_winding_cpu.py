"""The contract of the generalized winding number on the CPU: the numpy restatement tests/winding_ref.py
against analytic solid angles, against ray-crossing parity on closed meshes (an independent yardstick), on the holed sphere the
feature exists for, the stated association of the sum, and the refusals of the wrappers and the drivers.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raycast_ref as rr  # noqa: E402
import winding_ref as wr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLOSED = {"icosphere": rr.icosphere, "torus": rr.torus, "cube": rr.cube, "octahedron": rr.octahedron}


def one(v, f, p):
    return float(wr.winding_number(np.asarray(v, dtype=np.float32), np.asarray(f), np.asarray([p], dtype=np.float32))[0])


def parity_along(v, f, q, axis):
    rays = np.zeros((len(q), 6), dtype=np.float32)
    rays[:, :3] = q
    rays[:, 3 + axis] = 1.0
    return rr.count(v, f, rays) & 1


# ---- 1. analytic values -------------------------------------------------------------------------------------------------------
def test_octant_triangle_is_one_eighth():
    v = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    assert abs(one(v, [(0, 1, 2)], (0, 0, 0)) - 0.125) <= 1e-14         # the triangle spans one octant of the sphere
    assert abs(one(v, [(0, 2, 1)], (0, 0, 0)) + 0.125) <= 1e-14


def test_one_cube_face_is_one_sixth():
    v, f = rr.cube()
    for k in range(6):
        w = one(v, f[2 * k:2 * k + 2], (0, 0, 0))
        assert abs(abs(w) - 1 / 6) <= 1e-14, (k, w)
    assert abs(one(v, f, (0, 0, 0)) - 1.0) <= 1e-14                      # outward faces: +1 inside


def octasphere(subdivisions=2, radius=0.75):
    """the octahedron subdivided like raycast_ref.icosphere.  Its three coordinate planes are edge loops and stay so: the midpoint
    of two points with z = 0 has z = 0 exactly, before and after the normalisation and in fp32"""
    v, f = rr.octahedron()
    v, f = [p.astype(np.float64) for p in v], [tuple(t) for t in f]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, dtype=np.int64)


def test_half_sphere_through_the_query_is_one_half():
    """A surface whose boundary is a planar polygon through the query covers half of the sphere of directions: +-1/2.  The
    planarity has to be exact in fp32 for 1e-14, which the coordinate planes of the octahedron and of its subdivisions are.
    icosphere(2) has no such half: its faces with z >= 0 end in a zigzag, because the faces that the plane z = 0 cuts along a
    median are subdivided across it (their value from the origin is 0.4735...), so it is checked through its mirror symmetry
    instead: upper + lower + straddling = 1 and upper = lower."""
    for v, f in (rr.octahedron(), octasphere(2)):
        for axis in range(3):
            upper = f[(v[f][:, :, axis] >= 0).all(1)]
            assert 2 * len(upper) == len(f)
            w = one(v, upper, (0, 0, 0))
            assert abs(w - 0.5) <= 1e-14, (len(f), axis, w)
            assert abs(one(v, upper[:, [0, 2, 1]], (0, 0, 0)) + 0.5) <= 1e-14
    v, f = rr.icosphere(2)
    z = v[f][:, :, 2]
    up, low = f[(z >= 0).all(1)], f[(z <= 0).all(1)]
    mid = f[~(z >= 0).all(1) & ~(z <= 0).all(1)]
    assert len(up) == len(low) and len(mid) > 0
    wu, wl, wm = one(v, up, (0, 0, 0)), one(v, low, (0, 0, 0)), one(v, mid, (0, 0, 0))
    assert abs(wu - wl) <= 1e-14 and abs(wu + wl + wm - 1.0) <= 1e-14 and 0.4 < wu < 0.5


def test_zero_rules_and_nan():
    tri = np.array([(0.25, 0.5, 0.125), (1.5, -0.5, 0.75), (-0.5, 0.25, 2.0)], dtype=np.float32)
    for corner in tri:
        assert one(tri, [(0, 1, 2)], corner) == 0.0                      # a query on a vertex: a row of the determinant is zero
    inplane = (0.5 * (tri[0].astype(np.float64) + tri[1])).astype(np.float32)      # exactly representable: on an edge
    assert one(tri, [(0, 1, 2)], inplane) == 0.0
    assert one(tri, [(0, 0, 1)], (0.3, 0.2, 0.1)) == 0.0                 # a repeated corner
    line = [(0, 0, 0), (1, 1, 1), (2, 2, 2)]
    assert one(line, [(0, 1, 2)], (0.5, -0.25, 0.125)) == 0.0            # three corners in a line
    q = np.array([(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (0.1, 0.1, 0.1)], dtype=np.float32)
    v, f = rr.octahedron()
    w = wr.winding_number(v, f, q)
    assert np.isnan(w[:3]).all() and abs(w[3] - 1.0) <= 1e-14
    assert not wr.occupancy(w)[:3].any() and wr.occupancy(w)[3]


# ---- 2. an independent yardstick: crossing parity on closed meshes ------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CLOSED))
def test_equals_the_crossing_parity_on_closed_meshes(name):
    v, f = CLOSED[name]()
    q = np.random.default_rng(1).uniform(-1, 1, (2000, 3)).astype(np.float32)
    w = wr.winding_number(v, f, q)
    err = np.abs(w - parity_along(v, f, q, 2)).max()
    print(f"{name}: F = {len(f)}, max |w - parity| = {err:.3e}, bound {wr.tolerance(len(f)):.3e}")
    assert err <= wr.tolerance(len(f))


# ---- 3. the holed sphere ------------------------------------------------------------------------------------------------------
def test_holed_sphere_winding_against_parity():
    v, f, holes = wr.holed_sphere()
    assert len(rr.icosphere(3)[1]) == 1280 and len(f) == 1184
    q, kept, inside = wr.holed_sphere_queries(holes)
    qk, truth = q[kept], inside[kept]
    w = wr.winding_number(v, f, qk)
    wrong = int((wr.occupancy(w) != truth).sum())
    margin = float(np.abs(np.abs(w) - 0.5).min())
    votes = sum(parity_along(v, f, qk, axis) for axis in (2, 0, 1))
    wrong_z = int(((parity_along(v, f, qk, 2) == 1) != truth).sum())
    wrong_3 = int(((2 * votes > 3) != truth).sum())
    print(f"kept {kept.sum()}, winding wrong {wrong}, min margin {margin:.4f}, parity +z wrong {wrong_z}, majority wrong {wrong_3}")
    assert kept.sum() > 6000
    assert wrong == 0
    assert margin >= 0.3
    assert wrong_z >= 300
    assert wrong_3 >= 100


def test_inconsistent_orientation_means_nothing_and_inversion_is_forgiven():
    v, f = rr.cube_flipped()
    q = np.random.default_rng(1).uniform(-0.45, 0.45, (500, 3)).astype(np.float32)     # all inside the cube
    w = wr.winding_number(v, f, q)
    assert (parity_along(v, f, q, 2) == 1).all()                         # the parity does not care
    assert not wr.occupancy(w).all() and np.abs(w).max() < 0.7           # the winding number does
    v, f = rr.cube()
    w_in = wr.winding_number(v, f[:, [0, 2, 1]], q)
    assert np.abs(w_in + 1.0).max() <= wr.tolerance(len(f)) and wr.occupancy(w_in).all()


# ---- 4. the association is stated, not accidental -----------------------------------------------------------------------------
def test_the_group_association_is_close_to_a_flat_sum_and_not_the_same_bits():
    v, f = rr.torus(132, 64)                                             # 16 896 triangles: five groups
    q = np.random.default_rng(1).uniform(-1, 1, (64, 3)).astype(np.float32)
    grouped = wr.winding_number(v, f, q)
    chunked = wr.winding_number(v, f, q, group_chunks=None)              # chunk sums added left to right, no groups
    assert np.abs(grouped - chunked).max() <= wr.tolerance(len(f))
    assert (grouped.view(np.uint64) != chunked.view(np.uint64)).any()
    v, f = rr.torus()                                                    # 2 304 triangles: nine chunks, one group
    q = np.random.default_rng(1).uniform(-1, 1, (2000, 3)).astype(np.float32)
    a, b = wr.winding_number(v, f, q), wr.winding_number_flat(v, f, q)
    assert np.abs(a - b).max() <= wr.tolerance(len(f))
    assert (a.view(np.uint64) != b.view(np.uint64)).any()


# ---- 5. the ABI and the wrappers without a GPU --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from surfd_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        from surfd_amd.build import build_library
        build_library()
    return N.lib()


def test_abi_argument_errors_are_return_codes_before_any_hip_call(lib):
    h = C.c_void_p()
    one_ = C.c_void_p(8)                                                 # never dereferenced: every call below fails before a HIP call
    ERR_ARG = -1                                                         # SURFD_ERR_ARG
    assert lib.surfd_winding_create(None, 3, one_, 1, None, C.byref(h)) == ERR_ARG
    assert lib.surfd_winding_create(one_, 3, None, 1, None, C.byref(h)) == ERR_ARG
    assert lib.surfd_winding_create(one_, 3, one_, 1, None, None) == ERR_ARG
    assert lib.surfd_winding_create(one_, 0, one_, 1, None, C.byref(h)) == ERR_ARG
    assert lib.surfd_winding_create(one_, 3, one_, 0, None, C.byref(h)) == ERR_ARG
    assert lib.surfd_winding_create(one_, 3, one_, 715827883, None, C.byref(h)) == ERR_ARG     # 3 F = 2^31 + 1
    assert b"2^31" in lib.surfd_last_error() and h.value is None
    assert lib.surfd_winding_eval(None, one_, 1, 0, one_, None) == ERR_ARG
    assert lib.surfd_winding_num_triangles(None) == 0
    lib.surfd_winding_destroy(None)


def test_kernels_stay_in_registers():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    kernels = {k: v for k, v in mod.kernel_metadata().items() if "surfd::wn_" in k}
    assert len(kernels) == 4 and any("wn_kernel" in k for k in kernels)
    for name, k in kernels.items():
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 128, name          # four 256-thread workgroups per CU


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from surfd_amd import meshprep, voxelize, winding
    v, f = (torch.from_numpy(x) for x in rr.cube())
    p = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        winding.WindingScene(v, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        winding.winding_number(v, f, p)
    with pytest.raises(TypeError):
        winding.WindingScene(v.double(), f)
    with pytest.raises(TypeError):
        winding.WindingScene(v, f.float())
    with pytest.raises(ValueError):
        winding.WindingScene(v, f[:0])
    with pytest.raises(TypeError):
        winding.winding_number(v, f, p.double())
    with pytest.raises(ValueError):
        winding.winding_number(v, f, p[:, :2])
    for bad in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            winding._check_threshold(bad)
    with pytest.raises(ValueError, match="method"):
        meshprep.is_inside(v, f, p, method="flood")
    with pytest.raises(ValueError, match="nsamples"):
        meshprep.is_inside(v, f, p, nsamples=3, method="winding")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshprep.is_inside(v, f, p, method="winding")
    with pytest.raises(ValueError, match="sign"):
        meshprep.compute_sdf_and_gradients(v, f, p, sign="flood")
    with pytest.raises(ValueError, match="sign"):
        meshprep.compute_sdf_from_mesh(v, f, sign="flood")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshprep.compute_sdf_and_gradients(v, f, p, sign="winding")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        voxelize.voxelize_winding(v, f, 8)
    with pytest.raises(ValueError, match="resolution"):
        voxelize.voxelize_winding(v, f, 0)
    with pytest.raises(ValueError, match="resolution"):
        voxelize.voxelize_winding(v, f, 513)
    with pytest.raises(ValueError, match="bounds"):
        voxelize.voxelize_winding(v, f, 8, bounds=(1.0, 1.0))
    with pytest.raises(ValueError, match="threshold"):
        voxelize.voxelize_winding(v, f, 8, threshold=0.0)


# ---- 6. the drivers: argument errors, and defaults that leave the outputs as they were ----------------------------------------
def test_driver_arguments(tmp_path):
    from examples import evaluate, preprocess_udfs
    base = ["--generated", str(tmp_path), "--reference", str(tmp_path)]
    assert evaluate.parse(base).voxel_mode == "surface"
    assert evaluate.parse(base + ["--voxel_mode", "winding"]).voxel_mode == "winding"
    with pytest.raises(SystemExit):
        evaluate.parse(base + ["--voxel_mode", "flood"])
    with pytest.raises(SystemExit, match="--paired"):
        evaluate.run(evaluate.parse(base + ["--voxel_iou", "8", "--voxel_mode", "winding"]))
    d = preprocess_udfs.parse(["x.obj"])
    assert d.sign == "parity" and not d.signed
    assert preprocess_udfs.parse(["--signed", "--sign", "winding", "x.obj"]).sign == "winding"
    with pytest.raises(SystemExit):
        preprocess_udfs.parse(["--signed", "--sign", "flood", "x.obj"])
    out = tmp_path / "out"
    with pytest.raises(SystemExit, match="--signed"):
        preprocess_udfs.run(preprocess_udfs.parse(["--sign", "winding", "--output_dir", str(out), "x.obj"]))
    assert not out.exists()                                              # refused before anything is written


def test_defaults_keep_the_parity_path():
    """without the new options every consumer takes the path of before: the defaults are 'parity' / 'surface' and the unsigned
    driver never passes a sign"""
    import inspect
    from surfd_amd import meshprep
    assert inspect.signature(meshprep.is_inside).parameters["method"].default == "parity"
    assert inspect.signature(meshprep.compute_sdf_and_gradients).parameters["sign"].default == "parity"
    assert inspect.signature(meshprep.compute_sdf_from_mesh).parameters["sign"].default == "parity"
    assert meshprep.SIGN_METHODS == ("parity", "winding")
