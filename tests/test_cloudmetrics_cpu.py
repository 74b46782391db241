"""CPU-side checks of the point-cloud metrics (surfd_amd/cloudmetrics.py, csrc/cloudnn.hip): the two exports exist and are
bound, argument errors are return codes, the kernels are in the code object without spills or scratch, the set metrics give the
known answers on hand-built matrices (ties included), the normalisations are right on hand-checkable clouds, the module
refuses what it cannot take, and the yardstick (tests/cloud_ref.py) agrees with itself; the launch plan the library reports
(surfd_cloud_nn_matrix_plan) against a table worked out by hand, and the yardstick's restatement of the kernel's summation order
against its free-order one on every shape the GPU tests use.  Every test here fails on a tree without surfd_amd/cloudmetrics.py
or without the surfd_cloud_* symbols."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from surfd_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOUD_EXPORTS = ("surfd_cloud_nn", "surfd_cloud_nn_matrix", "surfd_cloud_nn_matrix_plan")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        from surfd_amd.build import build_library
        build_library()
    return N.lib()


@pytest.fixture(scope="module")
def CM():
    from surfd_amd import cloudmetrics
    return cloudmetrics


# ---- 1. library -------------------------------------------------------------------------------------------------------------------
def test_exports_and_bindings(lib):
    raw = C.CDLL(N.LIB_PATH)
    for sym in CLOUD_EXPORTS:
        assert hasattr(raw, sym), sym
        assert sym in N.EXPORTED_SYMBOLS, sym
    assert lib.surfd_abi_version() == 1
    assert "cloudnn.hip" in __import__("surfd_amd.build", fromlist=["SOURCES"]).SOURCES


def test_argument_errors_are_return_codes(lib):
    p = C.c_void_p(16)                                         # never dereferenced: every call below fails its checks first
    assert lib.surfd_cloud_nn(None, p, 1, 4, 4, p, p, None) == -1
    assert b"surfd_cloud_nn: null" in lib.surfd_last_error()
    assert lib.surfd_cloud_nn(p, None, 1, 4, 4, p, p, None) == -1
    assert lib.surfd_cloud_nn(p, p, -1, 4, 4, p, p, None) == -1
    assert lib.surfd_cloud_nn(p, p, 1, 0, 4, p, p, None) == -1
    assert b"must be positive" in lib.surfd_last_error()
    assert lib.surfd_cloud_nn(p, p, 1, 4, -3, p, p, None) == -1
    assert lib.surfd_cloud_nn(p, p, 0, 4, 4, p, p, None) == 0            # B = 0: a no-op
    assert lib.surfd_cloud_nn(None, None, 0, 4, 4, None, None, None) == 0
    assert lib.surfd_cloud_nn_matrix(None, 1, 4, p, 1, 4, 0.0, p, None, None) == -1
    assert b"surfd_cloud_nn_matrix: null" in lib.surfd_last_error()
    assert lib.surfd_cloud_nn_matrix(p, 1, 4, None, 1, 4, 0.0, p, None, None) == -1
    assert lib.surfd_cloud_nn_matrix(p, 1, 4, p, 1, 4, 0.0, None, None, None) == -1
    assert b"null mean" in lib.surfd_last_error()
    for M, Na, Rr, Nb in ((0, 4, 1, 4), (1, 0, 1, 4), (1, 4, 0, 4), (1, 4, 1, 0), (-2, 4, 1, 4)):
        assert lib.surfd_cloud_nn_matrix(p, M, Na, p, Rr, Nb, 0.0, p, None, None) == -1, (M, Na, Rr, Nb)
        assert b"must be positive" in lib.surfd_last_error()
    assert lib.surfd_cloud_nn_matrix(p, 1 << 21, 4, p, 1, 4, 0.0, p, None, None) == -4


def test_kernels_do_not_spill():
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    meta = mod.kernel_metadata()
    names = [k for k in meta if "surfd::cn_" in k]
    assert any("surfd::cn_nn_kernel" in k for k in names), names
    assert sum("cn_matrix_kernel<" in k for k in names) == 4                # P in {1, 2, 4, 8}
    assert len(names) == 5, names
    for k in names:
        v = meta[k]
        assert v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".private_segment_fixed_size"] == 0, (k, v)
        assert v[".group_segment_fixed_size"] <= 40 * 1024, (k, v)           # four workgroups per CU fit the 160 KiB of LDS


def test_inner_loop_instruction_count():
    """the figure the file header and DESIGN.md section 8.3 quote: VALU instructions per point pair of cn_matrix_kernel<8>'s
    inner loop, counted from the shipped library's disassembly; 9 is what the pair test costs when written out"""
    spec = importlib.util.spec_from_file_location("cloudmetrics_time", os.path.join(ROOT, "tools", "cloudmetrics_time.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    valu, pairs, ops = mod.inner_loop_valu()
    print(f"cn_matrix_kernel<8> inner loop: {valu} VALU instructions for {pairs} pairs = {valu / pairs:.3f} per pair; {ops}")
    assert pairs == 32
    assert valu / pairs <= 9.0
    assert not any(o.startswith("v_pk_") or o.startswith("v_fma") or o.startswith("v_mac") for o in ops), ops


# ---- 2. set metrics on hand-built matrices ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_identical_sets(CM, dtype):
    g = torch.Generator().manual_seed(0)
    D = torch.rand(6, 6, generator=g, dtype=dtype) + 0.5
    D = D + D.t()
    D.fill_diagonal_(0.0)
    r = CM.mmd_cov(D)
    assert r["cov"] == 1.0 and r["mmd"] == 0.0 and r["mmd_smp"] == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("G,Rr", [(5, 5), (4, 7), (7, 3)])
def test_two_separated_clusters(CM, dtype, G, Rr):
    """samples on a line: the generated ones around 0, the reference ones around 100; D = |x - y|"""
    xg = torch.arange(G, dtype=dtype) * 0.25
    xr = 100 + torch.arange(Rr, dtype=dtype) * 0.5
    D = lambda a, b: (a[:, None] - b[None, :]).abs()
    r = CM.one_nna(D(xg, xg), D(xr, xr), D(xg, xr))
    assert r == {"acc": 1.0, "acc_gen": 1.0, "acc_ref": 1.0}
    ref = R.one_nna_f64(D(xg, xg).numpy(), D(xr, xr).numpy(), D(xg, xr).numpy())
    assert r == ref
    mc = CM.mmd_cov(D(xg, xr))
    # every generated sample is nearest to reference 0; the nearest generated sample of every reference is the last one
    assert mc["cov"] == 1 / Rr
    assert mc["mmd"] == pytest.approx(float((xr - xg[-1]).double().mean()), rel=1e-6)
    assert mc["mmd_smp"] == pytest.approx(float((xr[0] - xg).double().mean()), rel=1e-6)
    assert mc == pytest.approx(R.mmd_cov_f64(D(xg, xr).numpy()), rel=1e-6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_interleaved_sets(CM, dtype):
    """generated at 0, 10, 20, ..., reference at 1, 11, 21, ...: every sample's nearest other sample has the other label"""
    xg = torch.arange(5, dtype=dtype) * 10
    xr = xg + 1
    D = lambda a, b: (a[:, None] - b[None, :]).abs()
    r = CM.one_nna(D(xg, xg), D(xr, xr), D(xg, xr))
    assert r == {"acc": 0.0, "acc_gen": 0.0, "acc_ref": 0.0}
    mc = CM.mmd_cov(D(xg, xr))
    assert mc["cov"] == 1.0 and mc["mmd"] == 1.0 and mc["mmd_smp"] == 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_exact_ties_go_to_the_lower_index(CM, dtype):
    # rows: generated samples; every row's minimum 1 is reached twice or three times
    D = torch.tensor([[1, 1, 5, 5],
                      [7, 1, 1, 1],
                      [1, 2, 1, 9]], dtype=dtype)
    mc = CM.mmd_cov(D)
    assert mc["cov"] == 2 / 4                                  # arg-mins 0, 1, 0: references {0, 1}
    assert mc["mmd"] == 1.0 and mc["mmd_smp"] == 1.0
    assert mc == R.mmd_cov_f64(D.numpy())
    # union of 2 + 2 samples where every off-diagonal distance is the same: every nearest other sample is index 0 (or 1 for
    # sample 0), which is a generated one
    one = torch.ones(2, 2, dtype=dtype)
    r = CM.one_nna(one, one, one)
    assert r == {"acc": 0.5, "acc_gen": 1.0, "acc_ref": 0.0}
    assert r == R.one_nna_f64(one.numpy(), one.numpy(), one.numpy())
    # a tie between a generated (index 1) and a reference (index 2) neighbour of sample 0: the generated one wins
    D_gg = torch.tensor([[0, 3], [3, 0]], dtype=dtype)
    D_rr = torch.tensor([[0, 9], [9, 0]], dtype=dtype)
    D_gr = torch.tensor([[3, 8], [8, 8]], dtype=dtype)
    r = CM.one_nna(D_gg, D_rr, D_gr)
    assert r == R.one_nna_f64(D_gg.numpy(), D_rr.numpy(), D_gr.numpy())
    assert r["acc_gen"] == 1.0 and r["acc_ref"] == 0.0       # both reference samples are nearest to generated 0 (3 and 8 < 9)
    D_gr[0, 0] = 2                                            # now sample 0's nearest other sample is reference 0, uniquely
    assert CM.one_nna(D_gg, D_rr, D_gr)["acc_gen"] == 0.5


def test_set_metrics_against_the_loops_on_random_matrices(CM):
    g = torch.Generator().manual_seed(3)
    for G, Rr in ((9, 9), (5, 11), (12, 4)):
        pts = torch.rand(G + Rr, 2, generator=g, dtype=torch.float64)
        U = (pts[:, None] - pts[None]).norm(dim=-1)
        D_gg, D_rr, D_gr = U[:G, :G].contiguous(), U[G:, G:].contiguous(), U[:G, G:].contiguous()
        assert CM.one_nna(D_gg, D_rr, D_gr) == pytest.approx(R.one_nna_f64(D_gg.numpy(), D_rr.numpy(), D_gr.numpy()), abs=0)
        assert CM.mmd_cov(D_gr) == pytest.approx(R.mmd_cov_f64(D_gr.numpy()), rel=1e-14)


def test_set_metric_refusals(CM):
    with pytest.raises(ValueError, match="2-D"):
        CM.mmd_cov(torch.zeros(3))
    with pytest.raises(ValueError, match="float32 or float64"):
        CM.mmd_cov(torch.zeros(3, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="NaN"):
        CM.mmd_cov(torch.full((2, 2), float("nan")))
    with pytest.raises(ValueError, match="D_gg must be"):
        CM.one_nna(torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(2, 3))


# ---- 3. the yardstick against itself ----------------------------------------------------------------------------------------------
def test_yardstick_fp32_against_fp64():
    err, n = R.fp32_restatement_error()
    print(f"fp32 restatement vs fp64 on {n} cloud pairs: largest relative error of a mean = {err:.3f} u (bound 7 u)")
    assert err * R.U < R.MEAN_BOUND
    # selection order of the restatement: duplicates and exact ties go to the lower index
    a = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    b = np.array([[2, 0, 0], [0.5, 0, 0], [0.5, 0, 0], [-0.5, 0, 0]], np.float32)
    d2, idx = R.nn_f32(a, b)
    assert idx.tolist() == [1, 1] and d2.tolist() == [0.25, 0.25]
    assert R.nn_f64(a, b).tolist() == [0.25, 0.25]
    assert R.ulp_distance(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1


def test_gpu_test_inputs_are_decided_clearly():
    """the condition item 8 of the GPU tests needs (asserted there again on the same matrices): on the fp64 Chamfer matrices of
    the 12 + 12 analytic shapes, every arg-min the set metrics take is decided by more than 1e-5 relative"""
    allc, splits = R.metric_sets()
    assert allc.shape == (24, 2048, 3) and allc.dtype == np.float32
    assert np.isfinite(allc).all() and np.abs(allc).max() <= 1.0
    m = R.matrix_f64(allc, allc)
    D = m + m.T
    for name, (gi, ri) in splits.items():
        gaps = R.assert_decided(*R.split_matrices(D, gi, ri))
        print(name, gaps)
    D_gr, D_gg, D_rr = R.split_matrices(D, *splits["copy"])
    assert R.mmd_cov_f64(D_gr) == {"mmd": 0.0, "cov": 1.0, "mmd_smp": 0.0} and R.one_nna_f64(D_gg, D_rr, D_gr)["acc"] <= 0.5
    assert R.one_nna_f64(*[R.split_matrices(D, *splits["disjoint"])[k] for k in (1, 2, 0)])["acc"] == 1.0


# ---- 4. normalisation --------------------------------------------------------------------------------------------------------------
def test_normalize_clouds(CM):
    x = torch.tensor([[[0.0, 0, 0], [4, 0, 0], [4, 2, 0], [0, 2, 0]],
                      [[1.0, 1, 1], [1, 1, 3], [1, 1, 1], [1, 1, 3]]])
    assert CM.normalize_clouds(x, "none") is x
    b = CM.normalize_clouds(x, "bbox")
    assert torch.equal(b[0], torch.tensor([[-1.0, -0.5, 0], [1, -0.5, 0], [1, 0.5, 0], [-1, 0.5, 0]]))
    assert torch.equal(b[1], torch.tensor([[0.0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, 1]]))
    s = CM.normalize_clouds(x, "unit_sphere")
    assert torch.allclose(s[0].mean(0), torch.zeros(3), atol=1e-7)
    assert torch.allclose(s.norm(dim=-1).amax(-1), torch.ones(2), atol=1e-6)
    assert torch.allclose(s[0], torch.tensor([[-2.0, -1, 0], [2, -1, 0], [2, 1, 0], [-2, 1, 0]]) / 5 ** 0.5, atol=1e-6)
    # a single cloud [N, 3]; a cloud without extent is only centred; fp64 stays fp64
    assert torch.equal(CM.normalize_clouds(x[0], "bbox"), b[0])
    p = torch.full((1, 4, 3), 0.5, dtype=torch.float64)
    for mode in ("bbox", "unit_sphere"):
        out = CM.normalize_clouds(p, mode)
        assert out.dtype == torch.float64 and float(out.abs().max()) < 1e-15
    with pytest.raises(ValueError, match="unknown mode"):
        CM.normalize_clouds(x, "sphere")
    with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
        CM.normalize_clouds(torch.zeros(4, 2), "bbox")


# ---- the module's refusals (no GPU needed) -----------------------------------------------------------------------------------------
def test_input_checks_before_any_launch(CM):
    ok = torch.zeros(2, 8, 3)
    for fn in (CM.nearest_neighbors, CM.chamfer_distance, CM.chamfer_matrix, CM.compute_all_metrics):
        with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
            fn(torch.zeros(8, 3), ok)
        with pytest.raises(ValueError, match="float32"):
            fn(ok.double(), ok)
        with pytest.raises(ValueError, match="contiguous"):
            fn(torch.zeros(2, 3, 8).transpose(1, 2), ok)
        with pytest.raises(ValueError, match="at least one point"):
            fn(ok, torch.zeros(2, 0, 3))
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn(ok, ok)
    with pytest.raises(ValueError, match="f_threshold"):
        CM.chamfer_distance(ok, ok, f_threshold=0.0)
    assert CM._tau2(0.01) == float(np.float32(0.01 * 0.01))


# ---- 5. the launch plan ------------------------------------------------------------------------------------------------------------
def matrix_plan_of(lib, M, Na, Rr):
    """(P, S, span, query_tiles) as the library reports them"""
    out = [C.c_int(-1) for _ in range(4)]
    rc = lib.surfd_cloud_nn_matrix_plan(M, Na, Rr, *[C.byref(v) for v in out])
    assert rc == 0, (rc, lib.surfd_last_error())
    return tuple(v.value for v in out)


# worked out by hand from the header: P = 1, 2, 4, 8 for Na <= 256, <= 512, <= 1024, above; query_tiles = ceil(Na / (256 P))
PLAN_OF_NA = {1: (1, 1), 256: (1, 1), 257: (2, 1), 512: (2, 1), 513: (4, 1), 1024: (4, 1), 1025: (8, 1), 2048: (8, 1), 2049: (8, 2),
              4096: (8, 2), 4097: (8, 3)}
# want = min(R, max(1, ceil(2048 / M))), span = ceil(R / want), S = ceil(R / span): (M, R) -> (S, span)
PLAN_OF_SETS = {(5, 7): (7, 1), (2048, 2): (1, 2), (1025, 3): (2, 2), (700, 7): (3, 3), (2049, 5): (1, 5), (3, 2049): (683, 3),
                (1, 2049): (1025, 2), (1, 4100): (1367, 3)}


def test_launch_plan_against_the_table(lib):
    for Na, (P, tiles) in PLAN_OF_NA.items():
        for M, Rr in ((1, 1), (700, 7)):
            got = matrix_plan_of(lib, M, Na, Rr)
            assert (got[0], got[3]) == (P, tiles), (Na, M, Rr, got)
    for (M, Rr), (S, span) in PLAN_OF_SETS.items():
        for Na in (5, 2049):
            got = matrix_plan_of(lib, M, Na, Rr)
            assert got[1:3] == (S, span), (M, Rr, Na, got)
            assert S * span >= Rr and (S - 1) * span < Rr, (M, Rr, S, span)   # the ranges cover every cloud and none is empty
    # every out pointer may be NULL, on its own and all together
    assert lib.surfd_cloud_nn_matrix_plan(700, 300, 7, None, None, None, None) == 0
    for k in range(4):
        out = [C.c_int(-1) for _ in range(4)]
        args = [None if n == k else C.byref(v) for n, v in enumerate(out)]
        assert lib.surfd_cloud_nn_matrix_plan(700, 300, 7, *args) == 0
        assert [v.value for v in out] == [-1 if n == k else w for n, w in enumerate((2, 3, 3, 1))]


def test_launch_plan_refuses_what_the_launch_refuses(lib):
    p = C.c_void_p(16)                                         # never dereferenced: every launch below fails its checks first
    prefix = lambda: lib.surfd_last_error().split(b", Nb")[0]
    cases = [((0, 4, 1), -1), ((1, 0, 1), -1), ((1, 4, 0), -1), ((-2, 4, 1), -1), ((1, -1, 1), -1), ((1, 4, -5), -1),
             (((1 << 20) + 1, 4, 1), -4), ((1, (1 << 24) + 1, 1), -4), ((1, 4, (1 << 20) + 1), -4)]
    for (M, Na, Rr), code in cases:
        out = [C.c_int(-1) for _ in range(4)]
        assert lib.surfd_cloud_nn_matrix_plan(M, Na, Rr, *[C.byref(v) for v in out]) == code, (M, Na, Rr)
        said = prefix()
        assert said.startswith(b"surfd_cloud_nn_matrix: M = %d, Na = %d, R = %d" % (M, Na, Rr)), said
        assert [v.value for v in out] == [-1] * 4                            # a refusal writes nothing
        assert lib.surfd_cloud_nn_matrix(p, M, Na, p, Rr, 4, 0.0, p, None, None) == code, (M, Na, Rr)
        assert prefix() == said
    # the limits themselves are accepted: want = max(1, ceil(2048 / 2^20)) = 1, so one range of all 2^20 clouds
    assert matrix_plan_of(lib, 1 << 20, 1 << 24, 1 << 20) == (8, 1, 1 << 20, 1 << 13)


# ---- 6. the kernel's summation order, restated, against the free-order restatement -----------------------------------------------------
GRID_NA = (1, 2, 63, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097)
GRID_NB = (1, 3, 4, 5, 2047, 2048, 2049, 4097)


def test_kernel_order_against_free_order_and_fp64():
    """what tests/test_gpu_cloudmetrics.py holds the kernel to bit for bit is itself within 1 ulp of the free-order mean and
    within MEAN_BOUND of the fp64 mathematics, on the whole shape grid of the GPU tests"""
    worst_ulp, worst_rel = 0, 0.0
    for Na in GRID_NA:
        a = R.random_cloud(1, Na, Na)[0]
        for Nb in GRID_NB:
            b = R.random_cloud(1, Nb, 7 * Nb + 1)[0]
            d2, _ = R.nn_f32(a, b)
            got = R.mean_kernel_order(d2)
            assert got.dtype == np.float32
            ulp = int(R.ulp_distance(got, R.mean_f32(a, b)[0]).max())
            m64 = R.mean_f64(a, b)
            rel = abs(float(got) - m64) / m64
            assert ulp <= 1, (Na, Nb, ulp)
            assert rel <= R.MEAN_BOUND, (Na, Nb, rel / R.U)
            worst_ulp, worst_rel = max(worst_ulp, ulp), max(worst_rel, rel)
    print(f"kernel-order mean on {len(GRID_NA) * len(GRID_NB)} cloud pairs: at most {worst_ulp} ulp from the free-order mean, "
          f"largest relative error against fp64 = {worst_rel / R.U:.3f} u (bound 7 u)")
    # the order itself where it decides the bits: worked out by hand in wave_order_case's docstring
    a, b, want, exact = R.wave_order_case()
    d2, _ = R.nn_f32(a, b)
    assert sorted(d2[d2 > 0].tolist()) == [2.0 ** -52] * 4 + [2.0 ** -22, 4.0]
    assert R.mean_kernel_order(d2) == want == np.float32(4 / 256) and exact > want
    w = [float(d2[k:k + 64].astype(np.float64).sum()) for k in range(0, 256, 64)]     # exact: at most two addends of one size
    assert np.float32(((w[0] + w[1]) + (w[2] + w[3])) / 256.0) == exact             # another association, another result
    matrix, below = R.matrix_kernel_order(R.random_cloud(2, 300, 1), R.random_cloud(3, 77, 2), 0.01)
    assert matrix.shape == below.shape == (2, 3) and matrix.dtype == np.float32 and below.dtype == np.int64
    assert R.matrix_kernel_order(R.random_cloud(2, 300, 1), R.random_cloud(3, 77, 2))[1] is None
