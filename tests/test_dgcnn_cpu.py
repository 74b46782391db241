"""CPU-side checks of the point-cloud encoder (surfd_amd/dgcnn.py, csrc/dgcnn.hip): the C ABI enumerates the reference
checkpoint layout, the kernels are in the code object without spills or scratch, the module refuses what it does not
implement, random_point_sampling draws what the reference draws, and the g18 fixture has its documented contents.  The last
part proves tests/dgcnn_ref.py (the restatement the GPU tests judge the kernels by) on that fixture, and checks on the CPU
what its exact network cases rest on."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import dgcnn_ref as R
from surfd_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DGCNN_EXPORTS = ("surfd_dgcnn_create", "surfd_dgcnn_destroy", "surfd_dgcnn_num_params", "surfd_dgcnn_param_info",
                 "surfd_dgcnn_set_param", "surfd_dgcnn_finalize", "surfd_dgcnn_knn", "surfd_dgcnn_forward",
                 "surfd_dgcnn_forward_features")


def reference_state_dict_spec(L):
    """Dgcnn(L).state_dict() of the reference (AutoEncoder/models/dgcnn.py:42-53), restated: keys, shapes, order."""
    spec = []
    for i, c in enumerate((64, 64, 128, 256, L), 1):
        spec += [(f"bn_{i}.weight", (c,)), (f"bn_{i}.bias", (c,)), (f"bn_{i}.running_mean", (c,)), (f"bn_{i}.running_var", (c,)),
                 (f"bn_{i}.num_batches_tracked", ())]
    spec += [("conv_1.weight", (64, 6)), ("conv_2.weight", (64, 128)), ("conv_3.weight", (128, 128)), ("conv_4.weight", (256, 256)),
             ("conv_5.weight", (L, 512))]
    return spec


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        from surfd_amd.build import build_library
        build_library()
    return N.lib()


def test_exports(lib):
    raw = C.CDLL(N.LIB_PATH)
    for sym in DGCNN_EXPORTS:
        assert hasattr(raw, sym), sym
        assert sym in N.EXPORTED_SYMBOLS, sym


@pytest.mark.parametrize("L", [32, 64])
def test_param_info_matches_reference_state_dict(lib, L):
    h = C.c_void_p()
    N.check(lib.surfd_dgcnn_create(L, 20, C.byref(h)))
    try:
        got = []
        for i in range(lib.surfd_dgcnn_num_params(h)):
            key, shp, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
            N.check(lib.surfd_dgcnn_param_info(h, i, C.byref(key), shp, C.byref(nd)))
            got.append((key.value.decode(), tuple(shp[:nd.value])))
    finally:
        lib.surfd_dgcnn_destroy(h)
    assert got == reference_state_dict_spec(L)
    from surfd_amd.dgcnn import Dgcnn
    assert [(k, tuple(v.shape)) for k, v in Dgcnn(L).state_dict().items()] == got


def test_create_and_finalize_errors(lib):
    h = C.c_void_p()
    assert lib.surfd_dgcnn_create(32, 0, C.byref(h)) == -4
    assert lib.surfd_dgcnn_create(32, 33, C.byref(h)) == -4
    assert lib.surfd_dgcnn_create(0, 20, C.byref(h)) == -1
    N.check(lib.surfd_dgcnn_create(32, 20, C.byref(h)))
    try:
        assert lib.surfd_dgcnn_set_param(h, b"conv_9.weight", None, N.shape_arr((1,)), 1, None) == -1
        assert lib.surfd_dgcnn_set_param(h, b"bn_1.num_batches_tracked", None, N.shape_arr(()), 0, None) == 0
        assert lib.surfd_dgcnn_finalize(h, None) == -2                       # nothing set yet
        assert b"not set" in lib.surfd_last_error()
        # a cloud with fewer points than k is rejected before anything runs (no device needed)
        assert lib.surfd_dgcnn_knn(h, C.c_void_p(16), 1, 19, None, C.c_void_p(16), None) == -1
        assert b"fewer than k" in lib.surfd_last_error()
        assert lib.surfd_dgcnn_forward(h, C.c_void_p(16), 1, 10, C.c_void_p(16), None) == -1
    finally:
        lib.surfd_dgcnn_destroy(h)


def test_kernels_do_not_spill():
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    meta = mod.kernel_metadata()
    names = [k for k in meta if "surfd::dg_" in k]
    for base in ("dg_knn_kernel", "dg_knn_merge_kernel", "dg_linear_kernel", "dg_edge_kernel", "dg_global_kernel", "dg_prep_kernel"):
        assert any(f"surfd::{base}" in k for k in names), (base, names)
    assert sum("dg_knn_kernel<" in k for k in names) == 5                   # K in {8, 16, 20, 24, 32}
    for k in names:
        v = meta[k]
        assert v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".private_segment_fixed_size"] == 0, (k, v)


def test_module_refusals():
    from surfd_amd.dgcnn import Dgcnn
    m = Dgcnn(32)
    x = torch.zeros(1, 64, 3)
    with pytest.raises(RuntimeError, match="eval-mode only"):
        m(x)                                                                 # a fresh module is in training mode
    with pytest.raises(NotImplementedError, match="'avg'"):
        Dgcnn(32, aggregate_ops_local="avg").eval()(x)
    with pytest.raises(NotImplementedError, match="not supported"):
        Dgcnn(32, aggregate_ops_global="none").eval()(x)                     # the rearrange fall-through (dgcnn.py:109-110)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(x)


def test_input_checks_before_any_launch():
    """What forward / knn check on the points before anything reaches the library (the CPU-tensor refusal comes last, so the
    other messages are seen here without a GPU)."""
    from surfd_amd.dgcnn import Dgcnn
    m = Dgcnn(32).eval()
    with pytest.raises(ValueError, match="at least k = 20 points"):
        m._check_input(torch.zeros(1, 19, 3))
    bad = torch.zeros(1, 40, 3)
    bad[0, 7, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN or Inf"):
        m._check_input(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m._check_input(torch.zeros(1, 40, 3))
    with pytest.raises(TypeError, match="float32"):
        m._check_input(torch.zeros(1, 40, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
        m._check_input(torch.zeros(40, 3))


def test_random_point_sampling_matches_reference(golden):
    from surfd_amd.dgcnn import random_point_sampling
    z = golden("g18_dgcnn")
    for tag in ("larger", "smaller", "batched"):
        shape = tuple(int(s) for s in z[f"rps_{tag}__shape"])
        num = int(z[f"rps_{tag}__num"])
        pcd = torch.arange(shape[-2]).float()[:, None].expand(*shape).contiguous()
        torch.manual_seed(10)
        got = random_point_sampling(pcd, num)
        assert got.shape == (*shape[:-2], num, shape[-1])
        assert np.array_equal(got[..., 0].long().numpy(), z[f"rps_{tag}__idx"]), tag
    assert len(np.unique(z["rps_smaller__idx"])) < 1000                     # 500 points -> 1000: drawn with replacement
    assert len(np.unique(z["rps_larger__idx"])) == 1000


def test_g18_fixture_layout(golden):
    z = golden("g18_dgcnn")
    for name, n in (("a", 2048), ("b", 2048), ("c", 10000)):
        assert z[f"{name}__pts"].shape == (n, 3) and z[f"{name}__pts"].dtype == np.float32
        assert z[f"{name}__rows"].shape == (128,)
        assert z[f"{name}__x1234"].shape == (128, 512)
        for L in (32, 64):
            assert z[f"{name}__latent_L{L}_f32"].shape == (L,) and z[f"{name}__latent_L{L}_f32"].dtype == np.float32
            assert z[f"{name}__latent_L{L}_f64"].shape == (L,) and z[f"{name}__latent_L{L}_f64"].dtype == np.float64
        if n == 2048:
            idx = z[f"{name}__knn_idx"]
            assert idx.shape == (n, 20)
            assert np.array_equal(idx[:, 0], np.arange(n))                  # every point is its own first neighbour
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g18_dgcnn.npz")) < 1 << 20


def test_synth_state_dict_exercises_every_branch():
    from surfd_amd.dgcnn import Dgcnn
    from surfd_amd.synth import synth_dgcnn_state_dict
    sd = synth_dgcnn_state_dict(32, seed=0)
    Dgcnn(32).load_state_dict(sd, strict=True)
    for i in range(1, 6):
        w, v = sd[f"bn_{i}.weight"], sd[f"bn_{i}.running_var"]
        assert (w < 0).any() and (w > 0).any() and (w == 0).any()
        assert (v > 0).all() and not torch.all(v == 1)
    Dgcnn(1).load_state_dict(synth_dgcnn_state_dict(1, seed=1), strict=True)   # the latent size knn_points itself creates


# ---- tests/dgcnn_ref.py, the restatement the GPU tests judge the kernels by, proven on the reference-made fixture ----------
@pytest.fixture(scope="module")
def restated(golden):
    """{(cloud, L, 'f32' | 'f64'): (latent [L], x1234 [N, 512])} of clouds a and b with the fixture's own neighbours"""
    from surfd_amd.synth import synth_dgcnn_state_dict
    z = golden("g18_dgcnn")
    out = {}
    for name in ("a", "b"):
        x = torch.from_numpy(z[f"{name}__pts"])[None]
        idx = torch.from_numpy(z[f"{name}__knn_idx"].astype(np.int64))[None]
        for L in (32, 64):
            sd = synth_dgcnn_state_dict(L, seed=0)
            for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
                lat, x1234 = R.dgcnn_forward(sd, x, idx, dt)
                assert lat.dtype == dt and x1234.dtype == dt
                out[name, L, tag] = (lat[0], x1234[0])
    return out


@pytest.mark.parametrize("L", [32, 64])
def test_restatement_fp64_reproduces_reference_latents(golden, restated, L):
    z = golden("g18_dgcnn")
    for name in ("a", "b"):
        ref = torch.from_numpy(z[f"{name}__latent_L{L}_f64"])
        err = float((restated[name, L, "f64"][0] - ref).abs().max())
        assert err <= 1e-12 * float(ref.abs().max()), (name, err)


@pytest.mark.parametrize("L", [32, 64])
def test_restatement_fp32_reproduces_reference_latents(golden, restated, L):
    z = golden("g18_dgcnn")
    for name in ("a", "b"):
        ref = torch.from_numpy(z[f"{name}__latent_L{L}_f32"])
        err = float((restated[name, L, "f32"][0] - ref).abs().max())
        assert err <= 1e-5 * float(ref.abs().max()) + 1e-6, (name, err)


def test_restatement_fp32_reproduces_reference_features(golden, restated):
    z = golden("g18_dgcnn")
    for name in ("a", "b"):
        got = restated[name, 32, "f32"][1][torch.from_numpy(z[f"{name}__rows"]).long()]
        ref = torch.from_numpy(z[f"{name}__x1234"])
        for blk, (c0, c1) in enumerate(R.X_SLICES, 1):
            err = float((got[:, c0:c1] - ref[:, c0:c1]).abs().max())
            assert err <= 1e-5 * float(ref[:, c0:c1].abs().max()) + 1e-6, (name, blk, err)


def test_restated_knn_reproduces_fixture_indices(golden):
    z = golden("g18_dgcnn")
    for name in ("a", "b"):
        d, i = R.knn_f32(torch.from_numpy(z[f"{name}__pts"])[None], 20)
        assert d.dtype == torch.float32 and i.dtype == torch.int64
        assert np.array_equal(i[0].numpy(), z[f"{name}__knn_idx"].astype(np.int64)), name
        assert bool((d[..., 1:] >= d[..., :-1]).all()) and bool((d[..., 0] == 0).all())


def test_exact_running_var():
    v = np.float32(R.exact_running_var())
    assert float(v) == R.exact_running_var()                                # an fp32 value
    assert np.float32(v + np.float32(1e-5)) == np.float32(1.0)
    t = torch.full((4,), float(v)) + 1e-5                                   # and so in torch's fp32 arithmetic
    assert bool((t == 1.0).all()) and bool((1 / torch.sqrt(t) == 1.0).all())


@pytest.mark.parametrize("k,N,B,L", R.NETWORK_SHAPES)
def test_exact_case_preconditions(k, N, B, L):
    """What the exact network cases of tests/test_gpu_dgcnn.py rest on, checked where no GPU is needed: with these inputs
    the fp32 evaluation has nothing to round, so the answer cannot depend on the order of a sum."""
    x, idx, sd, info = R.exact_case(k, N, B, L)
    assert x.shape == (B, N, 3) and idx.shape == (B, N, k)
    assert torch.equal(x * 8, (x * 8).round())                              # the 1/8 lattice
    assert B == 1 or not any(torch.equal(x[0], x[b]) for b in range(1, B))  # the clouds of a batch differ
    for i in range(1, 6):
        W = sd[f"conv_{i}.weight"]
        assert bool(((W == 0) | (W.abs() == 1)).all()) and int((W != 0).sum(1).max()) <= 4 and int((W != 0).sum(1).min()) >= 1
        s, t = R.fold_bn(sd, i, torch.float32)
        assert torch.equal(s, sd[f"bn_{i}.weight"])                         # the folded scale is bn.weight, exactly
        assert bool(((s.abs() == 1) | (s.abs() == 2)).all())
        if i < 5 or L > 1:                                                  # (one channel cannot have both signs)
            assert bool((s > 0).any()) and bool((s < 0).any())
        assert torch.equal(t * 8, (t * 8).round())
    assert bool((sd["bn_5.weight"][0] < 0))                                 # L = 1 takes the min branch
    lat64, x64 = R.dgcnn_forward(sd, x, idx, torch.float64, fold_dtype=torch.float32)
    lat32, x32 = R.dgcnn_forward(sd, x, idx, torch.float32)
    assert torch.equal(x32.double(), x64) and torch.equal(lat32.double(), lat64)
    assert info["min_act"] > 0 and float(x64.min()) > 0 and float(lat64.min()) > 0
    assert torch.equal(x64 * 8, (x64 * 8).round()) and torch.equal(lat64 * 8, (lat64 * 8).round())
    assert 8 * info["bound"] < 2 ** 24, info                                # no partial sum, in any order, leaves the exact range
    for c0, c1 in R.X_SLICES:                                               # not a constant network: the features vary
        assert x64[..., c0:c1].unique().numel() > 8 or N * k <= 8
