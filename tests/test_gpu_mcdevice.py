"""csrc/mcdevice.hip on the GPU against the host mesher of the same library: every comparison is
np.array_equal on vertices, faces, normals and values of `mcubes._run(volume.cpu().numpy(), None, 1, level, classic)`, floats
through their bit patterns so that -0 and NaN count.  No tolerance.  Each case runs for both triangle tables."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_fields  # noqa: E402

pytestmark = pytest.mark.gpu

CLASSIC = [True, False]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def host(volume, level, classic):
    from surfd_amd import mcubes
    return mcubes._run(np.ascontiguousarray(volume, np.float32), None, 1, level, classic)


def device(volume, level, classic):
    from surfd_amd.mcubes import marching_cubes_device
    out = marching_cubes_device(torch.tensor(np.asarray(volume, np.float32)).cuda(), level, classic=classic,
                                return_normals=True, return_values=True)
    assert [o.dtype for o in out] == [torch.float32, torch.int32, torch.float32, torch.float32] and all(o.is_cuda for o in out)
    return tuple(o.cpu().numpy() for o in out)


def assert_same(got, want, what=""):
    for name, g, w in zip(("vertices", "faces", "normals", "values"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(bits(g), bits(w)), (what, name, int((bits(g) != bits(w)).sum()), g.size)


def check(volume, level, classic, what=""):
    want = host(volume, level, classic)
    assert_same(device(volume, level, classic), want, what)
    return want


@functools.lru_cache(maxsize=None)
def noise(shape, seed=0):
    v = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def sphere_shell(n):
    """min(| |p| - 0.6 |, 0.1) over [-1, 1]^3"""
    ax = np.linspace(-1.0, 1.0, n, dtype=np.float32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    v = np.minimum(np.abs(np.sqrt(x * x + y * y + z * z) - np.float32(0.6)), np.float32(0.1)).astype(np.float32)
    v.setflags(write=False)
    return v


# ---- 1. every pattern ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classic", CLASSIC)
def test_every_sign_pattern_with_four_magnitude_draws(classic):
    """2x2x2 volumes, +-U(0.05, 1) with the signs of all 256 patterns, four draws each: the face and interior tests go both ways.
    One handle serves all 1024 volumes (the same shape)."""
    rng = np.random.default_rng(11)
    sizes = set()
    for pattern in range(256):
        # corner k of the marching-cubes order sits at (x, y, z) = (((k + 1) >> 1) & 1, (k >> 1) & 1, k >> 2)
        sign = np.empty((2, 2, 2), np.float32)
        for k in range(8):
            sign[k >> 2, (k >> 1) & 1, ((k + 1) >> 1) & 1] = 1.0 if (pattern >> k) & 1 else -1.0
        for draw in range(4):
            vol = (sign * rng.uniform(0.05, 1.0, size=(2, 2, 2))).astype(np.float32)
            want = check(vol, 0.0, classic, f"pattern {pattern} draw {draw}")
            sizes.add(len(want[1]))
    assert 0 in sizes and max(sizes) >= 4          # the empty patterns and the large fans were among them


# ---- 2. every case in context -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0.0, 0.3])
@pytest.mark.parametrize("classic", CLASSIC)
def test_noise_12_shares_vertices_across_every_edge_slot(classic, level):
    want = check(noise((12, 12, 12)), level, classic)
    assert len(want[0]) > 1000


# ---- 3. ties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classic", CLASSIC)
def test_corners_exactly_on_the_level(classic):
    """integers from {-1, 0, 1} at level 0: weights 1 / TINY, vertices that coincide with corners.  The host result is finite
    everywhere (asserted here, on the CPU, first); the bits are compared whatever it holds."""
    vol = np.random.default_rng(3).integers(-1, 2, size=(11, 11, 11)).astype(np.float32)
    want = host(vol, 0.0, classic)
    finite = all(np.isfinite(a).all() for a in (want[0], want[2], want[3]))
    assert_same(device(vol, 0.0, classic), want)
    assert finite and len(want[0]) > 100


# ---- 4. shapes across launch boundaries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 9, 13), (3, 4, 70), (2, 130, 3), (67, 2, 2), (33, 33, 33)])
@pytest.mark.parametrize("classic", CLASSIC)
def test_shapes_across_launch_boundaries(classic, shape):
    want = check(noise(shape, seed=sum(shape)), 0.0, classic)
    assert len(want[1]) > 0


# ---- 5. the workload's shape, small ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classic", CLASSIC)
def test_sphere_shell_is_closed_on_the_device(classic):
    from surfd_amd import meshtopo
    from surfd_amd.mcubes import marching_cubes_device
    vol = sphere_shell(64)
    check(vol, 0.01, classic)
    v, f = marching_cubes_device(torch.tensor(vol).cuda(), 0.01, classic=classic)
    assert f.is_cuda and len(f) > 10000
    assert meshtopo.is_closed(f, len(v))           # two closed sheets, judged from the device tensors


@pytest.mark.parametrize("classic", CLASSIC)
def test_open_sheet(classic):
    want = check(mc_fields.open_sheet(48)[0], 0.01, classic)
    assert len(want[1]) > 1000


# ---- 6. dense, many workgroups in the scan --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classic", CLASSIC)
def test_noise_40_many_workgroups(classic):
    want = check(noise((40, 40, 40)), 0.0, classic)
    assert len(want[1]) > 100000


# ---- 7. nothing to find ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classic", CLASSIC)
@pytest.mark.parametrize("fill", ["constant", "above"])
def test_nothing_to_find(fill, classic):
    vol = np.full((9, 10, 11), 0.25, np.float32) if fill == "constant" else (np.abs(noise((9, 10, 11))) + np.float32(1.0))
    got = device(vol, 0.5 if fill == "above" else 0.25, classic)
    assert [g.shape for g in got] == [(0, 3), (0, 3), (0, 3), (0,)]
    assert_same(got, host(vol, 0.5 if fill == "above" else 0.25, classic))


# ---- 8. reuse and stability ----------------------------------------------------------------------------------------------------------------
def run_handle(m, vol, level, classic):
    return tuple(o.cpu().numpy() for o in m.run(vol, level, classic, normals=True, values=True))


@pytest.mark.parametrize("classic", CLASSIC)
def test_one_handle_across_volumes_and_repeated_runs(classic):
    from surfd_amd.mcubes import DeviceMesher
    dense = torch.tensor(noise((40, 40, 40))).cuda()
    empty = torch.full((40, 40, 40), 0.25, device="cuda")
    want = host(noise((40, 40, 40)), 0.0, classic)
    m = DeviceMesher((40, 40, 40))
    first = run_handle(m, dense, 0.0, classic)
    nothing = run_handle(m, empty, 0.25, classic)
    third = run_handle(m, dense, 0.0, classic)
    assert [g.shape for g in nothing] == [(0, 3), (0, 3), (0, 3), (0,)]
    assert_same(first, want, "first")
    assert_same(third, first, "after an empty run")
    for k in range(10):
        assert_same(run_handle(m, dense, 0.0, classic), first, f"repeat {k}")
    m.close()


@pytest.mark.parametrize("classic", CLASSIC)
def test_non_default_stream(classic):
    from surfd_amd.mcubes import marching_cubes_device
    vol = torch.tensor(noise((40, 40, 40))).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = marching_cubes_device(vol, 0.0, classic=classic, return_normals=True, return_values=True)
    s.synchronize()
    assert_same(tuple(o.cpu().numpy() for o in out), host(noise((40, 40, 40)), 0.0, classic))


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from surfd_amd.mcubes import marching_cubes_device
    with pytest.raises(ValueError):
        marching_cubes_device(torch.zeros(4, 4, 4), 0.0)
    with pytest.raises(ValueError):
        marching_cubes_device(torch.zeros(4, 4, device="cuda"), 0.0)
    with pytest.raises(ValueError):
        marching_cubes_device(torch.zeros(4, 1, 4, device="cuda"), 0.0)
    with pytest.raises((ValueError, TypeError)):
        marching_cubes_device(torch.zeros(4, 4, 8, device="cuda")[:, :, ::2], 0.0)


def test_half_and_double_volumes_are_converted_to_fp32():
    from surfd_amd.mcubes import marching_cubes_device
    vol = noise((12, 12, 12))
    for dtype in (torch.float16, torch.float64):
        t = torch.tensor(vol).cuda().to(dtype)
        v, f = marching_cubes_device(t, 0.0)
        want = host(t.float().cpu().numpy(), 0.0, True)
        assert np.array_equal(bits(v.cpu().numpy()), bits(want[0])) and np.array_equal(f.cpu().numpy(), want[1])


# ---- 10. end to end ------------------------------------------------------------------------------------------------------------------------------
GRID = 64          # the smallest grid GridFiller builds (a power of two in [64, 1024])


class ShellField:
    """the analytic field of mcubes.bench_e2: a sphere shell above z = 0, a rim below"""

    def __call__(self, c):
        x, y, z = c[:, 0], c[:, 1], c[:, 2]
        up = (torch.sqrt(x * x + y * y + z * z) - 0.6).abs()
        rho = torch.sqrt(x * x + y * y) - 0.6
        return torch.clamp(torch.where(z >= 0, up, torch.sqrt(rho * rho + z * z)), max=0.1)


@pytest.mark.parametrize("normalize", [False, True])
def test_get_watertight_mesh_on_the_device_equals_the_host_path(normalize):
    from surfd_amd.meshudf import get_watertight_mesh
    hv, hf = get_watertight_mesh(ShellField(), GRID, normalize=normalize)
    dv, df = get_watertight_mesh(ShellField(), GRID, normalize=normalize, device=True)
    assert dv.is_cuda and df.is_cuda and dv.dtype == torch.float64 and df.dtype == torch.int64
    assert len(hf) > 500
    assert np.array_equal(dv.cpu().numpy().view(np.uint64), np.ascontiguousarray(hv).view(np.uint64))
    assert np.array_equal(df.cpu().numpy(), hf)


def test_get_watertight_mesh_min_faces_on_both_paths():
    from surfd_amd.meshudf import get_watertight_mesh
    full = get_watertight_mesh(ShellField(), GRID)
    hv, hf = get_watertight_mesh(ShellField(), GRID, min_faces=50)
    dv, df = get_watertight_mesh(ShellField(), GRID, min_faces=50, device=True)
    assert 0 < len(hf) <= len(full[1])
    assert np.array_equal(dv.cpu().numpy().view(np.uint64), np.ascontiguousarray(hv).view(np.uint64))
    assert np.array_equal(df.cpu().numpy(), hf)
