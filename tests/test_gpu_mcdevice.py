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
import mc_cases_ref as R  # noqa: E402
import mc_fields  # noqa: E402
from test_mc_cases_cpu import BANK, REQUIRED_EXITS, REQUIRED_FANS  # noqa: E402

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
    """2x2x2 volumes, +-U(0.05, 1) with the signs of all 256 patterns, four draws each.  One handle serves all 1024 volumes (the
    same shape).  What this covers: every pattern of both tables on a cube that shares nothing, and 36 of Lewiner's 83 fans
    through 28 exits of test_interior; magnitudes this tame leave most face and interior tests going one way only.  The rest of
    the case analysis is section 11's (the fan bank)."""
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


# ---- 11. every fan, in context (the fan bank) ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bank_volume(layout):
    """the bank's cubes as 2x2x2 blocks of one volume; the cubes between blocks get whatever patterns fall out and share edges
    with the bank's.  "flat": (2, 2 r, 2 c), blocks along y and x.  "deep": (2 n', 2, 2 k), blocks along z and x, so the cube
    that creates a shared vertex lies a whole plane back.  Blocks past the bank's end are 1 (above the level)."""
    cubes = np.load(BANK, allow_pickle=False)["cubes"]
    n = len(cubes)
    if layout == "flat":
        c = int(np.ceil(np.sqrt(n)))
        vol = np.ones((2, 2 * ((n + c - 1) // c), 2 * c), np.float32)
        for i, cube in enumerate(cubes):
            vol[:, 2 * (i // c):2 * (i // c) + 2, 2 * (i % c):2 * (i % c) + 2] = R.cube_volume(cube)
    else:
        k = 4
        vol = np.ones((2 * ((n + k - 1) // k), 2, 2 * k), np.float32)
        for i, cube in enumerate(cubes):
            vol[2 * (i // k):2 * (i // k) + 2, :, 2 * (i % k):2 * (i % k) + 2] = R.cube_volume(cube)
    vol.setflags(write=False)
    return vol


@pytest.mark.parametrize("layout", ["flat", "deep"])
def test_every_fan_of_the_bank_in_one_volume(layout):
    """the census is taken again on the volume as laid out (the plain port over every cube, on the host): all 78 fans and 45
    interior exits are in what the device meshes with one launch per table"""
    vol = bank_volume(layout)
    fans, exits = R.census(R.cubes_of(vol, 0.0))
    assert not REQUIRED_FANS - fans, sorted(REQUIRED_FANS - fans, key=str)
    assert not REQUIRED_EXITS - exits, sorted(REQUIRED_EXITS - exits)
    for classic in CLASSIC:
        want = check(vol, 0.0, classic, f"{layout} classic={classic}")
        assert len(want[1]) > len(np.load(BANK, allow_pickle=False)["cubes"])


# ---- 12. the level between floats --------------------------------------------------------------------------------------------------------------
def around_level(level, seed=5):
    """9x9x9 voxels drawn from the five floats f - 2 ulp .. f + 2 ulp around f = float32(level)"""
    f = np.float32(level)
    up1, dn1 = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
    five = np.array([np.nextafter(dn1, np.float32(-np.inf)), dn1, f, up1, np.nextafter(up1, np.float32(np.inf))], np.float32)
    assert np.isfinite(five).all() and len(set(five.view(np.uint32).tolist())) == 5
    return five[np.random.default_rng(seed).integers(0, 5, size=(9, 9, 9))]


# 0.3, 0.1: float32 rounds up (the threshold steps down one float); 0.7: rounds down; float32(0.3), 0.25: the level is a float and
# voxels equal it; 1e-46 rounds to 0; 1e-40 is subnormal; 16777217 is a tie that rounds to even
LEVELS = [0.3, 0.1, 0.7, float(np.float32(0.3)), 0.25, -0.3, 1e-46, 1e-40, -0.0, 16777217.0]


@pytest.mark.parametrize("level", LEVELS, ids=[repr(v) for v in LEVELS])
@pytest.mark.parametrize("classic", CLASSIC)
def test_voxels_within_two_ulp_of_the_level(classic, level):
    vol = around_level(level)
    want = host(vol, level, classic)
    assert len(want[0]) > 500 and all(np.isfinite(a).all() for a in (want[0], want[2], want[3]))
    assert_same(device(vol, level, classic), want, f"level {level!r}")


@pytest.mark.parametrize("level", [1e39, -1e39, float("inf"), float("-inf"), float("nan")], ids=repr)
@pytest.mark.parametrize("classic", CLASSIC)
def test_levels_outside_float_range_find_nothing(classic, level):
    vol = noise((9, 10, 11))
    want = host(vol, level, classic)
    got = device(vol, level, classic)
    assert [w.shape for w in want] == [(0, 3), (0, 3), (0, 3), (0,)]
    assert [g.shape for g in got] == [(0, 3), (0, 3), (0, 3), (0,)]
    assert_same(got, want)


# ---- 13. scales ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scaled_noise(scale):
    v = (noise((12, 12, 12)).astype(np.float64) * scale).astype(np.float32)
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("scale", [1e-42, 1e-38, 1e-20, 1e-9, 1e9, 1e30], ids=repr)
@pytest.mark.parametrize("classic", CLASSIC)
def test_noise_12_at_scales_from_subnormal_to_1e30(classic, scale):
    """at 1e-42 every voxel and every value is an fp32 subnormal; at 1e-9 and below every product of two corners is under TINY, so
    every face test of the non-classic table ties and the mesh has another face count than the unscaled volume's"""
    vol = scaled_noise(scale)
    want = host(vol, 0.0, classic)
    assert len(want[0]) > 2000 and all(np.isfinite(a).all() for a in (want[0], want[2], want[3]))
    if scale == 1e-42:
        tiny = float(np.finfo(np.float32).tiny)
        assert ((want[3] > 0) & (want[3] < tiny)).all() and (np.abs(vol) < tiny).all()
    if scale <= 1e-9 and not classic:
        assert len(want[1]) != len(host(noise((12, 12, 12)), 0.0, classic)[1])
    assert_same(device(vol, 0.0, classic), want, f"scale {scale!r}")


# ---- 14. deep scans: more than 1024 groups ---------------------------------------------------------------------------------------------------------
def ones_with_noise_at_group_boundaries(shape, seed=9):
    """1.0 everywhere, and 600 voxels of noise across the start of groups 0, 1, 2, 1023, 1024, 1025 and the last one (a group:
    1024 chunks of 64 voxels), so that active cubes straddle the group boundaries and the 1024-group mark of the second scan level"""
    vol = np.full(shape, 1.0, np.float32)
    flat = vol.reshape(-1)
    groups = -(-flat.size // 65536)
    assert groups > 1025
    rng = np.random.default_rng(seed)
    for g in (0, 1, 2, 1023, 1024, 1025, groups - 1):
        run = rng.standard_normal(600).astype(np.float32)
        lo = g * 65536 - 300
        flat[max(lo, 0):lo + 600] = run[max(lo, 0) - lo:]
    return vol, groups


# (130, 720, 720): 1029 groups, the top level scans with 2 entries per thread and a partly filled last segment; (3, 2, 22 400 000):
# 2051 groups, 3 entries per thread, and a row length of 25 bits for the reciprocal division
@pytest.mark.parametrize("shape,groups,classic", [((130, 720, 720), 1029, True), ((130, 720, 720), 1029, False),
                                                  ((3, 2, 22400000), 2051, True)])
def test_more_than_1024_groups_in_the_scan(shape, groups, classic):
    from surfd_amd.mcubes import DeviceMesher
    vol, ngroups = ones_with_noise_at_group_boundaries(shape)
    assert ngroups == groups
    want = host(vol, 0.0, classic)
    assert len(want[0]) > 5000
    # the voxel a vertex lies in: vertices exist on both sides of the 1024-group mark
    cell = np.floor(want[0].astype(np.float64)).astype(np.int64)
    group_of = ((cell[:, 0] * shape[1] + cell[:, 1]) * shape[2] + cell[:, 2]) // 65536
    assert {1023, 1024}.issubset(set(group_of.tolist()))
    m = DeviceMesher(shape)
    t = torch.from_numpy(vol).cuda()
    try:
        got = tuple(o.cpu().numpy() for o in m.run(t, 0.0, classic, normals=True, values=True))
    finally:
        m.close()
        del t
        torch.cuda.empty_cache()
    assert_same(got, want, f"{shape}")


@pytest.mark.parametrize("classic", CLASSIC)
def test_noise_48_dense_across_two_groups(classic):
    want = check(noise((48, 48, 48)), 0.0, classic)
    assert len(want[1]) > 200000


# ---- 15. the plateau -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [float(np.float32(0.1)), 0.1], ids=["float32(0.1)", "0.1"])
@pytest.mark.parametrize("classic", CLASSIC)
def test_plateau_on_the_level(classic, level):
    """sphere_shell clamps at float32(0.1), so most of the volume sits ON that level.  "On" is not above, and nothing else in the
    field is above either: at float32(0.1) host and device both find nothing.  At the double 0.1, just below that float, the
    plateau is above and the surface is where the shell meets it."""
    vol = sphere_shell(64)
    assert (vol == np.float32(0.1)).sum() > vol.size // 2
    want = host(vol, level, classic)
    assert all(np.isfinite(a).all() for a in (want[0], want[2], want[3]))
    assert len(want[1]) > 10000 if level == 0.1 else len(want[1]) == 0
    assert_same(device(vol, level, classic), want)


@pytest.mark.parametrize("classic", CLASSIC)
def test_plateau_on_the_level_below_the_surface(classic):
    """the same field negated, at level -float32(0.1): the plateau sits on the level, the shell is above it, and every active cube
    at the rim has corners that equal the level — weight 1 / TINY, vertices that coincide with corners — next to whole regions of
    cubes with all eight corners on the level"""
    vol = -sphere_shell(64)
    level = -float(np.float32(0.1))
    assert (vol == np.float32(level)).sum() > vol.size // 2 and (vol > np.float32(level)).any()
    want = host(vol, level, classic)
    assert len(want[1]) > 10000 and all(np.isfinite(a).all() for a in (want[0], want[2], want[3]))
    on_a_corner = (want[0] == np.floor(want[0])).all(axis=1)
    assert on_a_corner.sum() > 1000                # vertices pulled onto a corner that equals the level
    assert_same(device(vol, level, classic), want)


# ---- 16. optional outputs, the handle's state ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normals,values", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("classic", CLASSIC)
def test_optional_outputs(classic, normals, values):
    from surfd_amd.mcubes import DeviceMesher
    want = host(noise((12, 12, 12)), 0.0, classic)
    m = DeviceMesher((12, 12, 12))
    v, f, n, s = m.run(torch.tensor(noise((12, 12, 12))).cuda(), 0.0, classic, normals=normals, values=values)
    assert (n is None) == (not normals) and (s is None) == (not values)
    got = (v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy() if normals else want[2], s.cpu().numpy() if values else want[3])
    m.close()
    assert_same(got, want)


def test_emit_and_active_need_a_finished_run():
    import ctypes as C

    from surfd_amd import _native as N
    from surfd_amd.mcubes import DeviceMesher
    STATE = -2                                     # SURFD_ERR_STATE
    L = N.lib()
    vol = torch.tensor(noise((12, 12, 12))).cuda()
    want = host(noise((12, 12, 12)), 0.0, True)
    nv, nf = len(want[0]), len(want[1])

    def buffers():
        return (torch.empty((nv, 3), device="cuda"), torch.empty((nf, 3), device="cuda", dtype=torch.int32),
                torch.empty((nv, 3), device="cuda"), torch.empty((nv,), device="cuda"))

    def refused(m):
        na = C.c_int64(-7)
        b = buffers()
        return (L.surfd_mcd_emit(m._h, *(N.ptr(t) for t in b), N.stream()) == STATE and L.surfd_mcd_active(m._h, C.byref(na)) == STATE
                and na.value == -7)

    m = DeviceMesher((12, 12, 12))
    assert refused(m)                              # a fresh handle
    first = run_handle(m, vol, 0.0, True)
    assert_same(first, want, "first")
    assert m.active_cubes > 0
    m.classify_only(vol, 0.0, True)
    assert refused(m)                              # classify overwrote the masks and counts the last run's emit would read
    a, b = C.c_int64(), C.c_int64()
    N.check(L.surfd_mcd_run(m._h, N.ptr(vol), 0.0, 1, N.stream(), C.byref(a), C.byref(b)))
    assert (a.value, b.value) == (nv, nf)
    out = buffers()
    N.check(L.surfd_mcd_emit(m._h, *(N.ptr(t) for t in out), N.stream()))
    assert_same(tuple(o.cpu().numpy() for o in out), first, "run + emit after classify_only")
    m.close()
