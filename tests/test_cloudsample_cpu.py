"""CPU-side checks of the farthest point sampling (surfd_amd/cloudsample.py, csrc/cloudfps.hip): the two exports exist and are
bound, argument errors are return codes, the kernels are in the code object without spills or scratch and their LDS fits a CU,
the module refuses what it cannot take before any library call, the yardstick (tests/fps_ref.py) gives the hand-computed picks on
a six-point example with a tie and a duplicate, and the evaluation driver knows --sampling.  Every test here fails on a tree
without surfd_amd/cloudsample.py or without the surfd_cloud_fps* symbols."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from surfd_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fps_ref as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPS_EXPORTS = ("surfd_cloud_fps", "surfd_cloud_fps_workspace_bytes")
LDS_PER_CU = 160 * 1024
STREAM_LDS_MAX = 768 + 4 * 32768                  # the streamed tier's dynamic LDS at its largest (csrc/cloudfps.hip's header)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        from surfd_amd.build import build_library
        build_library()
    return N.lib()


@pytest.fixture(scope="module")
def CS():
    from surfd_amd import cloudsample
    return cloudsample


# ---- 1. library -------------------------------------------------------------------------------------------------------------------
def test_exports_and_bindings(lib):
    raw = C.CDLL(N.LIB_PATH)
    for sym in FPS_EXPORTS:
        assert hasattr(raw, sym), sym
        assert sym in N.EXPORTED_SYMBOLS, sym
    assert lib.surfd_abi_version() == 1
    assert "cloudfps.hip" in __import__("surfd_amd.build", fromlist=["SOURCES"]).SOURCES


def test_workspace_bytes(lib):
    assert lib.surfd_cloud_fps_workspace_bytes(3, 8192) == 0
    assert lib.surfd_cloud_fps_workspace_bytes(3, 32768) == 0
    assert lib.surfd_cloud_fps_workspace_bytes(3, 32769) == 4 * 3
    assert lib.surfd_cloud_fps_workspace_bytes(8, 100000) == 4 * 8 * (100000 - 32768)
    assert lib.surfd_cloud_fps_workspace_bytes(1 << 20, 1 << 20) == 4 * (1 << 20) * ((1 << 20) - 32768)       # beyond 2^31: int64
    for B, n in ((-1, 100000), (1, 0), (1, (1 << 20) + 1), ((1 << 20) + 1, 100000)):
        assert lib.surfd_cloud_fps_workspace_bytes(B, n) == 0, (B, n)


def test_argument_errors_are_return_codes(lib):
    p = C.c_void_p(16)                                         # never dereferenced: every call below fails its checks first
    fps = lib.surfd_cloud_fps
    assert fps(p, -1, 4, None, None, 2, p, p, None, None) == -1
    assert b"surfd_cloud_fps: B = -1 is negative" in lib.surfd_last_error()
    assert fps(p, 1, 0, None, None, 2, p, p, None, None) == -1
    assert b"surfd_cloud_fps: N = 0, K = 2 must be positive" in lib.surfd_last_error()
    assert fps(p, 1, 4, None, None, 0, p, p, None, None) == -1
    assert b"must be positive" in lib.surfd_last_error()
    assert fps(p, 0, 4, None, None, 2, p, p, None, None) == 0             # B = 0: a no-op
    assert fps(None, 0, 4, None, None, 2, None, None, None, None) == 0
    assert fps(None, 1, 4, None, None, 2, p, p, None, None) == -1
    assert b"surfd_cloud_fps: null points" in lib.surfd_last_error()
    assert fps(p, 1, 4, None, None, 2, None, p, None, None) == -1
    assert b"surfd_cloud_fps: null idx_out" in lib.surfd_last_error()
    assert fps(p, 1, (1 << 20) + 1, None, None, 2, p, p, p, None) == -4
    assert b"surfd_cloud_fps: B = 1, N = 1048577 is beyond the supported size" in lib.surfd_last_error()
    assert fps(p, (1 << 20) + 1, 4, None, None, 2, p, p, p, None) == -4
    assert fps(p, 1, 32769, None, None, 2, p, p, None, None) == -1         # the first size that needs a workspace
    assert b"surfd_cloud_fps: null workspace" in lib.surfd_last_error()


def test_kernels_do_not_spill_and_fit_the_cu():
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    meta = mod.kernel_metadata()
    names = [k for k in meta if "surfd::fps_" in k]
    assert any("surfd::fps_stream_kernel" in k for k in names), names
    for P, T in ((1, 64), (1, 256), (2, 256), (4, 256), (8, 256), (16, 256), (8, 1024)):
        assert sum(f"fps_resident_kernel<{P}, {T}>" in k for k in names) == 1, (P, T, names)
    assert len(names) == 8, names
    for k in names:
        v = meta[k]
        print(k.split("(")[0], v)
        assert v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".private_segment_fixed_size"] == 0, (k, v)
        lanes_1024 = "1024>" in k or "stream" in k                               # 1 024 lanes = 4 waves per SIMD of 512 registers
        assert v[".vgpr_count"] + v.get(".agpr_count", 0) <= (128 if lanes_1024 else 256), (k, v)
        static = v[".group_segment_fixed_size"]
        assert static <= 768, (k, v)                                             # the slots; the streamed tier's LDS is dynamic
        assert static + (STREAM_LDS_MAX if "stream" in k else 0) <= LDS_PER_CU, (k, v)


# ---- 2. the module's refusals (no GPU needed) ---------------------------------------------------------------------------------------
def test_input_checks_before_any_library_call(CS, monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(N, "lib", no_library)
    ok = torch.zeros(2, 8, 3)
    for fn in (CS.farthest_point_sampling, CS.sample_farthest_points):
        with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
            fn(torch.zeros(8, 3), 4)
        with pytest.raises(ValueError, match="float32"):
            fn(ok.double(), 4)
        with pytest.raises(ValueError, match="contiguous"):
            fn(torch.zeros(2, 3, 8).transpose(1, 2), 4)
        with pytest.raises(ValueError, match="at least one point"):
            fn(torch.zeros(2, 0, 3), 4)
        with pytest.raises(ValueError, match="K must be an int"):
            fn(ok, 4.0)
        with pytest.raises(ValueError, match=r"lengths must be a \[B\]"):
            fn(ok, 4, lengths=torch.tensor([8, 8, 8]))
        with pytest.raises(ValueError, match="lengths must be int32 or int64"):
            fn(ok, 4, lengths=torch.tensor([8.0, 8.0]))
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn(ok, 4)
    with pytest.raises(ValueError, match=r"start_index must be a \[B\]"):
        CS.farthest_point_sampling(ok, 4, start_index=torch.tensor([0]))
    with pytest.raises(ValueError, match="start_index must be an int or"):
        CS.farthest_point_sampling(ok, 4, start_index=1.5)
    with pytest.raises(ValueError, match="no CPU fallback"):               # the refusal comes before the ranges
        CS.farthest_point_sampling(ok, 0)
    # the ranges, as farthest_point_sampling checks them after the CPU-tensor refusal (tests/test_gpu_cloudsample.py reaches them
    # through the public call)
    B, n = 2, 8
    CS._check_ranges(4, B, n, None, 0)
    CS._check_ranges(100, B, n, torch.tensor([8, 1]), torch.tensor([7, 0]))
    with pytest.raises(ValueError, match="K must be at least 1"):
        CS._check_ranges(0, B, n, None, 0)
    with pytest.raises(ValueError, match="K must be at least 1"):
        CS._check_ranges(-3, B, n, None, 0)
    with pytest.raises(ValueError, match="more than the supported"):
        CS._check_ranges(4, B, (1 << 20) + 1, None, 0)
    for bad in ([0, 8], [8, 9], [-1, 3]):
        with pytest.raises(ValueError, match=r"lengths must lie in 1 \.\. N = 8"):
            CS._check_ranges(4, B, n, torch.tensor(bad), 0)
    for bad in (-1, 8):
        with pytest.raises(ValueError, match="start_index must lie in"):
            CS._check_ranges(4, B, n, None, bad)
    with pytest.raises(ValueError, match="start_index must lie in"):
        CS._check_ranges(4, B, n, torch.tensor([8, 3]), 3)                 # 3 is outside the cloud of length 3
    for bad in ([0, 8], [-1, 0]):
        with pytest.raises(ValueError, match="start_index must lie in"):
            CS._check_ranges(4, B, n, None, torch.tensor(bad))
    with pytest.raises(ValueError, match="start_index must lie in"):
        CS._check_ranges(4, B, n, torch.tensor([8, 3]), torch.tensor([7, 3]))


def test_sample_points_evenly_refusals():
    from surfd_amd import meshprep as M
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    t = torch.tensor([[0, 1, 2]])
    with pytest.raises(ValueError, match="number_of_points must be positive"):
        M.sample_points_evenly(v, t, 0)
    with pytest.raises(ValueError, match="init_factor"):
        M.sample_points_evenly(v, t, 4, init_factor=0)

# ---- 3. the yardstick ------------------------------------------------------------------------------------------------------------
def test_yardstick_on_the_hand_example():
    idx, cover2 = F.fps_f32(F.HAND_POINTS, 8)
    assert idx.tolist() == F.HAND_IDX
    assert cover2.tolist() == F.HAND_COVER2 and cover2.dtype == np.float32
    i64, c64 = F.fps_f64(F.HAND_POINTS, 8)
    assert i64.tolist() == F.HAND_IDX and c64.tolist() == F.HAND_COVER2
    # another start, a truncated cloud, and the batch form
    idx, cover2 = F.fps_f32(F.HAND_POINTS, 3, start=5)                   # from (0, 4, 0): farthest is 2 (32), then 0 (16, tie-free)
    assert idx.tolist() == [5, 2, 0] and cover2.tolist() == [32.0, 16.0, 4.0]
    idx, cover2 = F.fps_f32(F.HAND_POINTS, 4, n=3)                       # points 0, 1, 2 only
    assert idx.tolist() == [0, 2, 1, -1] and cover2.tolist() == [16.0, 1.0, 0.0, 0.0]
    bi, bc = F.fps_batch(np.stack([F.HAND_POINTS, F.HAND_POINTS]), 4, lengths=[6, 3], start=[5, 0])
    assert bi.tolist() == [[5, 2, 0, 3], [0, 2, 1, -1]] and bc[1].tolist() == [16.0, 1.0, 0.0, 0.0]
    # cover2 is what it says: the largest squared distance of a point to its nearest pick
    x = F.R.random_cloud(1, 300, 5)[0]
    idx, cover2 = F.fps_f32(x, 40)
    assert (np.diff(cover2) <= 0).all()
    # fp32 against fp64: 5 u on a squared distance (two subtractions squared, the product, two additions; section 8.3 of
    # DESIGN.md), which the minimum and the maximum keep; 1 u spare
    assert abs(F.cover2_of(x, x[idx]) - float(cover2[-1])) <= 6 * 2.0 ** -24 * float(cover2[-1])
    gaps = F.decisions(F.HAND_POINTS, 6)
    assert gaps[0] == 0 and gaps[3] == 0 and gaps[2] > 0                 # the tie of 2 and 5, the duplicate, a decided round


# ---- 4. the driver -----------------------------------------------------------------------------------------------------------------
def test_evaluate_help_lists_sampling():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "evaluate.py"), "--help"], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--sampling {uniform,even}" in r.stdout and "--init_factor" in r.stdout
