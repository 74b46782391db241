"""The fast winding numbers (csrc/winding.hip's fast path) without a GPU, on the numpy restatement
tests/winding_fast_ref.py: the records of cases that can be checked by hand, beta = +inf against the exact restatement, the
approximation error against tests/winding_ref.py under the caps the feature was accepted with, and the refusals of the wrappers
and of the two drivers' flags."""
import functools
import os
import sys

import ctypes as C
import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_ref as br  # noqa: E402
import raycast_ref as rr  # noqa: E402
import winding_fast_ref as wf  # noqa: E402
import winding_ref as wr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. records that can be checked by hand ------------------------------------------------------------------------------------
def test_records_of_one_triangle():
    v = np.array([(0, 0, 0), (2, 0, 0), (0, 4, 0)], dtype=np.float32)
    tree = wf.build(v, np.array([(0, 1, 2)]))
    assert tree["records"].shape == (1, 4, 7)
    rec = tree["records"][0]
    centre = np.array([2.0, 4.0, 0.0]) / 3.0                             # ((A + B) + C) / 3, and a c / a of one triangle
    a = 4.0
    assert np.array_equal(rec[0, 3:6], [0.0, 0.0, a])                    # 0.5 (u x v) = (0, 0, 4)
    assert np.array_equal(rec[0, :3], (a * centre) / a)
    m = np.maximum(rec[0, :3] - [0, 0, 0], [2, 4, 0] - rec[0, :3])       # the farthest corner of the box [0, 2] x [0, 4] x [0, 0]
    assert rec[0, 6] == (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2] and m[1] == 4 - rec[0, 1]
    assert np.array_equal(rec[1:], np.tile(wf.ABSENT, (3, 1)))           # the three slots that hold nothing
    assert np.array_equal(tree["root_sums"], [a, *(a * centre), 0.0, 0.0, a])


def test_records_of_the_cube():
    v, f = rr.cube()
    tree = wf.build(v, f)
    assert tree["lay"]["nleaf"] == 3 and tree["lay"]["levels"] == 1 and tree["records"].shape == (1, 4, 7)
    a, ac, n = wf.triangle_moments(v, f)
    assert np.array_equal(a, np.full(12, 0.5))                           # twelve half unit squares
    rec = tree["records"][0]
    for c in range(3):
        ids = tree["leaves"][c]
        assert (ids >= 0).all()
        sa, sac, sn = 0.0, np.zeros(3), np.zeros(3)
        for i in ids:                                                    # slot order, left to right from +0
            sa, sac, sn = sa + a[i], sac + ac[i], sn + n[i]
        assert sa == 2.0 and np.array_equal(rec[c, :3], sac / sa) and np.array_equal(rec[c, 3:6], sn)
        lo, hi = tree["boxes"][0, :3, c].astype(np.float64), tree["boxes"][0, 3:, c].astype(np.float64)
        corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        assert np.isclose(rec[c, 6], ((corners - rec[c, :3]) ** 2).sum(1).max(), rtol=1e-15)
    assert np.array_equal(rec[3], wf.ABSENT)
    assert tree["root_sums"][0] == 6.0 and np.array_equal(tree["root_sums"][4:], np.zeros(3))      # a closed surface has no vector area
    assert np.abs(tree["root_sums"][1:4]).max() <= 6 * 2.0 ** -52       # the cube is centred on the origin


def test_a_leaf_without_area_takes_the_centre_of_its_box():
    v = np.array([(1, 1, 1), (3, 1, 1), (5, 1, 1), (2, 3, 7)], dtype=np.float32)
    f = np.array([(0, 1, 2), (2, 1, 0), (0, 0, 0), (1, 2, 2)])         # four triangles without area: one leaf
    tree = wf.build(v, f)
    rec = tree["records"][0, 0]
    assert np.array_equal(rec[:3], [3.0, 1.0, 1.0]) and np.array_equal(rec[3:6], np.zeros(3)) and rec[6] == 4.0
    w, ncl, ntri = wf.walk(tree, np.array([(30, 1, 1), (3, 1, 2)], dtype=np.float32), 2.0)
    assert np.array_equal(w, [0.0, 0.0]) and ncl.tolist() == [1, 0] and ntri.tolist() == [0, 4]


def test_a_box_beyond_2_to_20_is_never_approximated():
    v, f = rr.cube()
    v = v.copy()
    v[0] = (-2.0 ** 21, -0.5, -0.5)
    tree = wf.build(v, f)
    inf = tree["records"][0, :, 6] == np.inf
    assert inf.any() and not inf[3]
    q = np.array([(0.1, 0.2, 0.3), (1e7, 0, 0)], dtype=np.float32)
    w, ncl, ntri = wf.walk(tree, q, 1.0)
    touched = sum(int((tree["leaves"][c] >= 0).sum()) for c in range(3) if inf[c])
    assert (ntri >= touched).all()


def test_theta_pairs_is_winding_ref_theta():
    v, f = rr.icosphere(1)
    A, B, C = wr._corners(v, f)
    q = np.random.default_rng(0).uniform(-1, 1, (len(f), 3)).astype(np.float32)
    full = wr.theta(q, A, B, C)
    assert np.array_equal(wf.theta_pairs(q.astype(np.float64), A, B, C), np.diagonal(full))


# ---- 2. beta = +inf is the exact sum in the tree's order -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "torus", "wavy_sheet", "holed_sphere"])
def test_beta_inf_equals_the_exact_restatement(name):
    v, f = wr.holed_sphere()[:2] if name == "holed_sphere" else rr.MESHES[name]()
    q = np.random.default_rng(7).uniform(-1, 1, (200, 3)).astype(np.float32)
    q[5] = (np.nan, 0, 0)
    w, ncl, ntri = wf.walk(wf.build(v, f), q, np.inf)
    ok = np.arange(len(q)) != 5
    assert np.isnan(w[5]) and ncl[5] == 0 and ntri[5] == 0
    assert not ncl.any() and (ntri[ok] == len(f)).all()
    assert np.abs(w[ok] - wr.winding_number(v, f, q[ok])).max() <= wr.tolerance(len(f))


def test_a_query_does_not_depend_on_its_neighbours():
    v, f = rr.torus()
    tree = wf.build(v, f)
    q = np.random.default_rng(8).uniform(-1, 1, (64, 3)).astype(np.float32)
    w, ncl, ntri = wf.walk(tree, q, 2.0)
    for i in (0, 17, 63):
        wi, ci, ti = wf.walk(tree, q[i:i + 1], 2.0)
        assert wi[0].view(np.uint64) == w[i].view(np.uint64) and (ci[0], ti[0]) == (ncl[i], ntri[i])
    assert np.array_equal(wf.walk(tree, q[::-1], 2.0)[0][::-1].view(np.uint64), w.view(np.uint64))


# ---- 3. the approximation error against the exact restatement ------------------------------------------------------------------
ERROR_CASES = {"torus": lambda: rr.torus(132, 64), "icosphere": lambda: rr.icosphere(4), "holed_sphere": lambda: wr.holed_sphere()[:2]}
ERROR_CAPS = {2.0: 0.05, 3.0: 0.02}


@functools.lru_cache(maxsize=None)
def error_case(name):
    v, f = ERROR_CASES[name]()
    q = np.random.default_rng(3).uniform(-1, 1, (3000, 3)).astype(np.float32)
    exact = wr.winding_number(v, f, q)
    exact.setflags(write=False)
    return v, f, q, exact, wf.build(v, f)


@pytest.mark.parametrize("name", sorted(ERROR_CASES))
def test_the_approximation_error_stays_under_the_caps(name):
    """Measured with this restatement (beta = 2 / beta = 3), 3 000 uniform queries in [-1, 1]^3, max |w_fast - w_exact|:
    torus(132, 64) 3.36e-2 / 1.05e-2, icosphere(4) 2.19e-2 / 7.71e-3, holed sphere 1.43e-2 / 5.63e-3; no occupancy changes."""
    v, f, q, exact, tree = error_case(name)
    if name == "torus":
        assert len(f) == 16896
    clear = np.abs(np.abs(exact) - 0.5) > 0.1
    assert clear.sum() > 2000
    for beta, cap in ERROR_CAPS.items():
        w, ncl, ntri = wf.walk(tree, q, beta)
        err = float(np.abs(w - exact).max())
        flips = int((wr.occupancy(w) != wr.occupancy(exact))[clear].sum())
        print(f"{name}: F = {len(f)}, beta = {beta}: max |w_fast - w_exact| = {err:.3e} (cap {cap}), occupancy changes {flips}, "
              f"cluster terms {ncl.mean():.1f}, triangle terms {ntri.mean():.1f} per query")
        assert err <= cap, (name, beta, err)
        assert flips == 0, (name, beta, flips)
        assert (ncl + ntri).mean() < len(f) / 2                           # and it is the hierarchy that does it


# ---- 4. the ABI and the wrappers without a GPU ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from surfd_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        from surfd_amd.build import build_library
        build_library()
    return N.lib()


def test_abi_argument_errors_are_return_codes_before_any_hip_call(lib):
    from surfd_amd import _native as N
    for sym in ("surfd_winding_build_bvh", "surfd_winding_eval_fast", "surfd_winding_visits", "surfd_winding_bvh_info", "surfd_winding_bvh_read"):
        assert sym in N.EXPORTED_SYMBOLS, sym
    one_ = C.c_void_p(8)                                                 # never dereferenced
    a, b = C.c_int64(), C.c_int64()
    assert lib.surfd_winding_build_bvh(None, None) == -1
    assert lib.surfd_winding_eval_fast(None, one_, 1, 2.0, 0, one_, None) == -1
    assert lib.surfd_winding_visits(None, C.byref(a), C.byref(b), None) == -1
    assert lib.surfd_winding_bvh_info(None, None, None, None, None, 0) == -1
    assert lib.surfd_winding_bvh_read(None, None, None, None, None) == -1
    assert lib.surfd_abi_version() == 1


def test_the_fast_kernels_stay_in_registers():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    kernels = {k: v for k, v in mod.kernel_metadata().items() if "surfd::fwn_" in k}
    assert len(kernels) == 4 and any("fwn_walk_kernel" in k for k in kernels)
    for name, k in kernels.items():
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".private_segment_fixed_size"] == 0, name
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 128, name          # four 256-thread workgroups per CU


def test_wrappers_refuse_bad_arguments():
    from surfd_amd import voxelize, winding
    v, f = (torch.from_numpy(x) for x in rr.cube())
    p = torch.zeros(4, 3)
    for bad in (0.5, 0.0, -2.0, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="beta"):
            winding._check_beta(bad)
        with pytest.raises(ValueError, match="beta"):
            winding.WindingScene(v, f, accel="bvh", beta=bad)
        with pytest.raises(ValueError, match="beta"):
            winding.winding_number(v, f, p, accel="bvh", beta=bad)
        with pytest.raises(ValueError, match="beta"):
            voxelize.voxelize_winding(v, f, 8, accel="bvh", beta=bad)
        with pytest.raises(ValueError, match="beta"):
            wf.check_beta(bad)
    assert winding._check_beta(1) == 1.0 and winding._check_beta(float("inf")) == float("inf") and wf.check_beta(np.inf) == np.inf
    for bad in ("tiles", "fast", None):
        with pytest.raises(ValueError, match="accel"):
            winding.WindingScene(v, f, accel=bad)
        with pytest.raises(ValueError, match="accel"):
            winding.winding_number(v, f, p, accel=bad)
        with pytest.raises(ValueError, match="accel"):
            voxelize.voxelize_winding(v, f, 8, accel=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # the arguments are fine: the CPU tensors are refused last
        winding.WindingScene(v, f, accel="bvh", beta=3.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        winding.winding_number(v, f, p, accel="bvh")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        voxelize.voxelize_winding(v, f, 8, accel="bvh", beta=float("inf"))


def test_driver_arguments(tmp_path):
    from examples import evaluate, preprocess_udfs
    base = ["--generated", str(tmp_path), "--reference", str(tmp_path)]
    a = evaluate.parse(base)
    assert a.winding_accel == "exact" and a.winding_beta == 2.0
    a = evaluate.parse(base + ["--winding_accel", "bvh", "--winding_beta", "3"])
    assert a.winding_accel == "bvh" and a.winding_beta == 3.0
    with pytest.raises(SystemExit):
        evaluate.parse(base + ["--winding_accel", "tiles"])
    with pytest.raises(SystemExit, match="--voxel_mode winding"):
        evaluate.run(evaluate.parse(base + ["--paired", "--winding_accel", "bvh"]))
    with pytest.raises(SystemExit, match="--voxel_mode winding"):
        evaluate.run(evaluate.parse(base + ["--paired", "--voxel_iou", "8", "--voxel_mode", "solid", "--winding_accel", "bvh"]))
    with pytest.raises(SystemExit, match="--winding_beta"):
        evaluate.run(evaluate.parse(base + ["--paired", "--voxel_iou", "8", "--voxel_mode", "winding", "--winding_accel", "bvh", "--winding_beta", "0.5"]))
    d = preprocess_udfs.parse(["x.obj"])
    assert d.winding_accel == "exact" and d.winding_beta == 2.0
    assert preprocess_udfs.parse(["--winding_accel", "bvh", "--winding_beta", "inf", "x.obj"]).winding_beta == float("inf")
    with pytest.raises(SystemExit):
        preprocess_udfs.parse(["--winding_accel", "tiles", "x.obj"])
    out = tmp_path / "out"
    with pytest.raises(SystemExit, match="--sign winding"):
        preprocess_udfs.run(preprocess_udfs.parse(["--signed", "--winding_accel", "bvh", "--output_dir", str(out), "x.obj"]))
    with pytest.raises(SystemExit, match="--winding_beta"):
        preprocess_udfs.run(preprocess_udfs.parse(["--signed", "--sign", "winding", "--winding_accel", "bvh", "--winding_beta", "nan",
                                                   "--output_dir", str(out), "x.obj"]))
    assert not out.exists()                                              # refused before anything is written
