"""CPU-side checks of the point-cloud encoder (surfd_amd/dgcnn.py, csrc/dgcnn.hip): the C ABI enumerates the reference
checkpoint layout, the kernels are in the code object without spills or scratch, the module refuses what it does not
implement, random_point_sampling draws what the reference draws, and the g18 fixture has its documented contents."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

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
