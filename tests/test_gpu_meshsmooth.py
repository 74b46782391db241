"""csrc/meshsmooth.hip on the GPU against the sequential restatement tests/meshsmooth_ref.py.  Positions and
the area-weighted normals are compared bit for bit; the angle-weighted normals within the bound that the device's acos allows;
the Laplacian also against meshproc within the bound measured on the CPU (tests/test_meshsmooth_cpu.py).  The shapes are the
smallest at which the kernels can go wrong (meshsmooth_ref.shapes)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshsmooth_ref as R  # noqa: E402
from test_meshsmooth_cpu import laplacian_bound  # noqa: E402

from surfd_amd import meshproc as mp  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = R.shapes()
NAMES = sorted(SHAPES)


def cu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def smoother(name):
    from surfd_amd.meshsmooth import MeshSmoother
    v, f = SHAPES[name]
    return MeshSmoother(cu(f), len(v))


@functools.lru_cache(maxsize=None)
def ref(name, what, *args):
    """the restatement's result, worked out once per (shape, call) and shared; callers do not write to it"""
    v, f = SHAPES[name]
    out = getattr(R, what)(v, f, *args)
    for a in (out if isinstance(out, tuple) else (out,)):
        a.setflags(write=False)
    return out


def same(got, want):
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got, want), f"max |difference| {np.abs(got - want).max():.3e}, {int((got != want).sum())} entries"


@pytest.mark.parametrize("name", NAMES)
def test_counts(name):
    v, f = SHAPES[name]
    s = smoother(name)
    assert (s.num_border_halfedges, s.num_border_vertices) == R.counts(f)
    assert (s.num_faces, s.num_vertices) == (len(f), len(v))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("cotangent,boundary", [(True, True), (True, False), (False, True), (False, False)])
def test_laplacian_equals_the_restatement(name, cotangent, boundary):
    v, f = SHAPES[name]
    s = smoother(name)
    want = ref(name, "laplacian", 3, cotangent, boundary)
    same(s.laplacian(cu(v), 3, cotangent, boundary), want)


@pytest.mark.parametrize("name", NAMES)
def test_smooth_borders_equals_the_restatement_and_meshproc(name):
    v, f = SHAPES[name]
    got = smoother(name).smooth_borders(cu(v))
    same(got, ref(name, "smooth_borders"))
    same(got, mp.smooth_borders(v, f))
    if name == "tetrahedron":
        same(got, v)                                         # closed: the identity


@pytest.mark.parametrize("name", NAMES)
def test_umbrella_and_taubin_equal_the_restatement(name):
    v, f = SHAPES[name]
    s = smoother(name)
    same(s.umbrella(cu(v), 0.5, sweeps=3), ref(name, "umbrella", 0.5, None, 3))
    same(s.taubin(cu(v), 4), ref(name, "taubin", 4))
    same(s.taubin(cu(v)), ref(name, "taubin"))


@pytest.mark.parametrize("name", NAMES)
def test_area_normals_equal_the_restatement(name):
    v, f = SHAPES[name]
    unit, raw = smoother(name).vertex_normals(cu(v), "area", return_raw=True)
    want_unit, want_raw = ref(name, "vertex_normals", "area")
    same(raw, want_raw)
    same(unit, want_unit)


def angle_bound(name):
    """per component of the raw sum: deg(v) 2^-48.  Every term is a unit-normal component (|.| <= 1, the same bits on both sides)
    times an angle <= pi < 4; an acos within 4 ulp on the device (the OpenCL bound) and 1 ulp on the host leaves the two angles
    within 5 * 2^-51 < 2^-48 of each other; deg(v) terms."""
    v, f = SHAPES[name]
    return R.valence(f, len(v))[:, None] * 2.0 ** -48


@pytest.mark.parametrize("name", NAMES)
def test_angle_normals_within_the_acos_bound(name):
    v, f = SHAPES[name]
    unit, raw = smoother(name).vertex_normals(cu(v), "angle", return_raw=True)
    unit, raw = unit.cpu().numpy(), raw.cpu().numpy()
    want_unit, want_raw = ref(name, "vertex_normals", "angle")
    bound = angle_bound(name)
    err = np.abs(raw - want_raw)
    print(f"{name}: raw error / bound {np.max(err / np.maximum(bound, 2.0 ** -60), initial=0.0):.3f}")
    assert (err <= bound).all()
    length = np.sqrt((want_raw * want_raw).sum(axis=1))
    big = length >= 1e-3
    assert (np.abs(unit - want_unit)[big] <= (bound / np.maximum(length, 1e-3)[:, None])[big]).all()
    assert np.array_equal(unit[length == 0], np.zeros_like(unit[length == 0]))
    # fp32 positions are converted exactly: the same result as their fp64 copy
    v32 = v.astype(np.float32)
    a = smoother(name).vertex_normals(cu(v32), "angle")
    b = smoother(name).vertex_normals(cu(v32.astype(np.float64)), "angle")
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", R.WELL_CONDITIONED)
@pytest.mark.parametrize("boundary", [True, False])
def test_laplacian_within_the_measured_bound_of_meshproc(name, boundary):
    v, f = SHAPES[name]
    got = smoother(name).laplacian(cu(v), 3, True, boundary).cpu().numpy()
    err = np.abs(got - mp.laplacian_smooth(v, f, 3, True, boundary)).max()
    print(f"{name} boundary={boundary}: {err / (2.0 ** -52 * np.abs(v).max()):.3f} units")
    assert err <= laplacian_bound(v)


def test_fp32_positions_steps_zero_and_empty():
    from surfd_amd import meshsmooth
    v, f = SHAPES["sheet5"]
    v32 = v.astype(np.float32)
    s = smoother("sheet5")
    same(s.laplacian(cu(v32)), R.laplacian(v32.astype(np.float64), f))
    same(s.smooth_borders(cu(v32)), R.smooth_borders(v32.astype(np.float64), f))
    x = cu(v)
    for out in (s.laplacian(x, steps=0), s.taubin(x, steps=0), s.smooth_borders(x, iterations=0)):
        assert out.data_ptr() != x.data_ptr() and torch.equal(out, x)           # a copy
    same(s.laplacian(cu(v32), steps=0), v32.astype(np.float64))
    # one-shot forms
    same(meshsmooth.laplacian_smooth(x, cu(f)), ref("sheet5", "laplacian", 3, True, True))
    same(meshsmooth.smooth_borders(x, cu(f, torch.int32)), ref("sheet5", "smooth_borders"))
    same(meshsmooth.taubin_smooth(x, cu(f)), ref("sheet5", "taubin"))
    # F = 0: the input comes back
    v0, f0 = SHAPES["empty"]
    x0 = cu(v0)
    e = smoother("empty")
    assert e.laplacian(x0) is x0 and e.taubin(x0) is x0 and e.smooth_borders(x0) is x0
    same(e.vertex_normals(x0), np.zeros_like(v0))


def test_sweeps_are_jacobi_over_several_workgroups():
    """1 600 vertices: seven workgroups, the last one partly filled.  A sweep that wrote into the buffer it reads would differ
    from the restatement after two steps; so would a second sweep that read the first sweep's input."""
    v, f = SHAPES["sheet40"]
    s = smoother("sheet40")
    for steps in (1, 2, 3):
        same(s.umbrella(cu(v), 0.5, sweeps=steps), R.umbrella(v, f, 0.5, None, steps))
        same(s.laplacian(cu(v), steps), R.laplacian(v, f, steps))
    x = cu(v)
    s.laplacian(x, 2)
    same(x, v)                                               # the caller's positions are not written


def test_repeated_runs_are_bit_identical():
    v, f = SHAPES["icosphere2"]
    s = smoother("icosphere2")
    x = cu(v)
    first = (s.laplacian(x), s.taubin(x), s.umbrella(x, 0.3, sweeps=5), s.vertex_normals(x))
    for _ in range(9):
        again = (s.laplacian(x), s.taubin(x), s.umbrella(x, 0.3, sweeps=5), s.vertex_normals(x))
        assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_one_handle_many_vertex_arrays():
    v, f = SHAPES["sheet40"]
    s = smoother("sheet40")
    rng = np.random.default_rng(5)
    arrays = [v, v + 0.05 * rng.standard_normal(v.shape), 3.0 * v[::-1].copy()]
    outs = [s.laplacian(cu(a)) for a in arrays]              # all enqueued before any is read
    outs_b = [s.smooth_borders(cu(a)) for a in arrays]
    for a, o, b in zip(arrays, outs, outs_b):
        same(o, R.laplacian(a, f))
        same(b, R.smooth_borders(a, f))


def test_taubin_keeps_the_radius_better_than_the_umbrella():
    v, f = SHAPES["icosphere2"]
    s = smoother("icosphere2")
    radius = lambda p: float(p.norm(dim=1).mean())           # noqa: E731
    assert abs(radius(s.taubin(cu(v), 10)) - 1.0) < abs(radius(s.umbrella(cu(v), 0.5, sweeps=10)) - 1.0)


def test_refusals():
    from surfd_amd import meshsmooth
    v, f = SHAPES["two_triangles"]
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshsmooth.MeshSmoother(tf)
    s = meshsmooth.MeshSmoother(tf.cuda(), len(v))
    for call in (s.laplacian, s.smooth_borders, s.taubin, s.vertex_normals):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(tv)
        with pytest.raises(ValueError):
            call(tv.cuda()[:, :2])
        with pytest.raises(ValueError):
            call(tv.cuda()[:3])                              # another number of vertices than the handle's
        with pytest.raises(TypeError):
            call(tv.cuda().half())
    with pytest.raises(ValueError):
        meshsmooth.MeshSmoother(tf.cuda()[:, :2])
    with pytest.raises(TypeError):
        meshsmooth.MeshSmoother(tf.cuda().float())
    with pytest.raises(ValueError):
        s.vertex_normals(tv.cuda(), weight="uniform")
    with pytest.raises(ValueError):
        s.laplacian(tv.cuda(), steps=-1)
    # an index outside [0, V): refused by the library at creation, with its error code, never read
    for bad in ([[0, 1, 4]], [[0, -1, 2]]):
        with pytest.raises(RuntimeError, match=r"libsurfd_hip error -1: .*outside \[0, 4\)"):
            meshsmooth.MeshSmoother(torch.tensor(f.tolist() + bad).cuda(), 4)
    with pytest.raises(RuntimeError, match="outside"):
        meshsmooth.laplacian_smooth(tv.cuda()[:3].contiguous(), tf.cuda())


@pytest.mark.parametrize("name", ["tetrahedron", "icosphere2"])
def test_renderer_takes_device_normals(name):
    from surfd_amd import render as RD
    v, f = SHAPES[name]
    v32 = cu((v - v.mean(axis=0)).astype(np.float32))
    ft = cu(f)
    r = RD.Renderer(48, max_views=2)
    cams = RD.orbit_cameras(2, 25.0, 2.8, size=48)
    host = r.render(v32, ft, cams, smooth=True)
    dev = r.render(v32, ft, cams, smooth="device")
    for k in ("face", "depth", "mask"):
        assert torch.equal(host[k], dev[k]), k
    assert int(host["mask"].sum()) > 100
    # the two sets of vertex normals differ by at most the angle bound in fp64, so by at most one fp32 rounding (2^-24 below 1) per
    # component; the interpolated normal is divided by its length, >= 1/3 between the corners of a tetrahedron (x 3), components
    # mix through the normalisation and the camera rotation (x sqrt 3), and the fp32 chain rounds a handful of times on changed
    # inputs (2^-24 each): below 16 * 2^-24
    diff = (host["normal"] - dev["normal"]).abs().max()
    print(f"{name}: max normal difference {float(diff):.3e}")
    assert float(diff) <= 16 * 2.0 ** -24
    with pytest.raises(ValueError):
        r.render(v32, ft, cams, smooth="host")


def test_get_mesh_from_udf_device_post_is_bit_identical():
    from surfd_amd import synth
    from surfd_amd.cbndec import CbnDecoder, make_udf_func
    from surfd_amd.meshudf import get_mesh_from_udf
    from surfd_amd.spec import DecoderConfig
    dec = CbnDecoder(63, 32, 512, 5)
    dec.load_state_dict(synth.synth_decoder_state_dict(DecoderConfig(latent_dim=32)), strict=True)
    dec = dec.cuda().eval()
    # the untrained decoder's udf never comes close to 0, and get_mesh_from_udf drops faces whose probes lie above 1 / N: of the
    # seeds tried on the CPU oracle this one leaves the most grid points below 1 / 64 (about a thousand), so faces survive
    lat = (torch.randn(1, 32, generator=torch.Generator().manual_seed(2)) * 0.8).cuda()
    field = make_udf_func(dec, lat)
    kw = dict(coords_range=(-1, 1), max_dist=0.1, N=64, max_batch=2 ** 16)
    v0, t0 = get_mesh_from_udf(field, differentiable=False, **kw)
    v1, t1 = get_mesh_from_udf(field, differentiable=False, device_post=True, **kw)
    assert len(t0) > 0 and v1.dtype == torch.float32 and t1.dtype == torch.int64
    assert torch.equal(t0, t1) and torch.equal(v0, v1)
    assert not torch.equal(v0, get_mesh_from_udf(field, differentiable=False, smooth_borders=False, **kw)[0])      # the mesh has a border to smooth
    v2, t2 = get_mesh_from_udf(field, differentiable=True, device_post=True, **kw)
    assert torch.equal(t0, t2)
    np.testing.assert_allclose(v2.detach().cpu().numpy(), v0.cpu().numpy(), atol=1e-6)
