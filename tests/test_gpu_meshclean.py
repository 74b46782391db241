"""csrc/meshclean.hip on the GPU against surfd_amd.meshproc: vertices and faces bit for bit and in the same
order, no tolerance anywhere.  The shapes are the smallest at which each rule can go wrong (meshclean_ref.shapes); the stats of
clean_until_stable are compared with the sequential restatement, which tests/test_meshclean_cpu.py pins to meshproc."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshclean_ref as R  # noqa: E402

from surfd_amd import meshproc as mp  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = R.shapes()
NAMES = sorted(SHAPES)


def cu(x, dtype=None):
    t = torch.from_numpy(np.array(x))                         # a copy: the shared references are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def same_v(got, want):
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), f"{int((got.view(np.int64) != want.view(np.int64)).sum())} entries differ"


def same_f(got, want):
    assert got.dtype == torch.int64 and got.is_cuda
    want = torch.from_numpy(np.array(want).reshape(-1, 3))
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    assert torch.equal(got.cpu(), want), f"{int((got.cpu() != want).any(dim=1).sum())} faces differ"


@functools.lru_cache(maxsize=None)
def host(name):
    """meshproc's own chain on a fixture, worked out once and shared (callers do not write to it): the cull, then the duplicate
    pass, the height test and the caps, each on the result before it; and the whole clean_until_stable with the restatement's stats"""
    v, f = SHAPES[name]
    with np.errstate(all="ignore"):
        v1, f0 = mp.cull_and_merge(v, f)
        fd = mp.drop_duplicate_faces(f0)
        fg = mp.drop_degenerate_faces(v1, fd)
        fh = mp.fill_small_holes(v1, fg)
        cv, cf = mp.clean_until_stable(v, f)
        raw = (mp.drop_duplicate_faces(f), mp.drop_degenerate_faces(v, f), mp.fill_small_holes(v, f))
    out = dict(v1=v1, f0=f0, fd=fd, fg=fg, fh=fh, cv=cv, cf=cf, raw=raw, stats=R.clean_until_stable(v, f)[2])
    for a in (v1, f0, fd, fg, fh, cv, cf) + raw:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_cull_and_merge(name):
    from surfd_amd import meshclean as MC
    v, f = SHAPES[name]
    gv, gf = MC.cull_and_merge(cu(v), cu(f))
    same_v(gv, host(name)["v1"]); same_f(gf, host(name)["f0"])


@pytest.mark.parametrize("name", NAMES)
def test_drop_duplicate_faces(name):
    from surfd_amd import meshclean as MC
    h = host(name)
    same_f(MC.drop_duplicate_faces(cu(h["f0"])), h["fd"])
    same_f(MC.drop_duplicate_faces(cu(SHAPES[name][1])), h["raw"][0])


@pytest.mark.parametrize("name", NAMES)
def test_drop_degenerate_faces(name):
    from surfd_amd import meshclean as MC
    h = host(name)
    same_f(MC.drop_degenerate_faces(cu(h["v1"]), cu(h["fd"])), h["fg"])
    v, f = SHAPES[name]                                      # the raw mesh: NaN coordinates, repeated indices, coincident vertices
    same_f(MC.drop_degenerate_faces(cu(v), cu(f)), h["raw"][1])


@pytest.mark.parametrize("name", NAMES)
def test_fill_small_holes(name):
    from surfd_amd import meshclean as MC
    h = host(name)
    same_f(MC.fill_small_holes(cu(h["v1"]), cu(h["fg"])), h["fh"])
    v, f = SHAPES[name]
    same_f(MC.fill_small_holes(cu(v), cu(f)), h["raw"][2])


@pytest.mark.parametrize("name", NAMES)
def test_clean_until_stable(name):
    from surfd_amd import meshclean as MC
    v, f = SHAPES[name]
    h = host(name)
    gv, gf, st = MC.clean_until_stable(cu(v), cu(f), return_stats=True)
    same_v(gv, h["cv"]); same_f(gf, h["cf"])
    assert st == h["stats"], (st, h["stats"])
    gv, gf = MC.clean_until_stable(cu(v), cu(f, torch.int32))
    same_v(gv, h["cv"]); same_f(gf, h["cf"])


def test_heights_on_random_triangles():
    """the height test on triangles of every scale down to its thresholds, slivers among them: the same faces as meshproc keeps"""
    from surfd_amd import meshclean as MC
    rng = np.random.default_rng(11)
    v = rng.standard_normal((3000, 3)) * 10.0 ** rng.integers(-9, 3, size=(3000, 1))
    f = rng.integers(0, len(v), size=(4000, 3))
    thin = np.arange(0, 3000 - 3, 3)
    v[thin + 2] = v[thin] + (v[thin + 1] - v[thin]) * rng.random((len(thin), 1)) + rng.standard_normal((len(thin), 3)) * 1e-8
    f = np.vstack([f, np.stack([thin, thin + 1, thin + 2], axis=1)])
    want = mp.drop_degenerate_faces(v, f)
    assert 0 < len(want) < len(f)
    same_f(MC.drop_degenerate_faces(cu(v), cu(f)), want)


def test_repeated_runs_are_bit_identical():
    from surfd_amd import meshclean as MC
    v, f = cu(SHAPES["sheet64"][0]), cu(SHAPES["sheet64"][1])
    v0, f0 = MC.clean_until_stable(v, f)
    for _ in range(9):
        v1, f1 = MC.clean_until_stable(v, f)
        assert torch.equal(f0, f1) and torch.equal(v0.view(torch.int64), v1.view(torch.int64))


@pytest.mark.parametrize("name", ["soup", "octahedron_minus_one"])
def test_float32_input_is_widened_exactly(name):
    from surfd_amd import meshclean as MC
    v, f = SHAPES[name]
    v32 = v.astype(np.float32)
    with np.errstate(all="ignore"):
        wv, wf = mp.clean_until_stable(v32, f)               # np.asarray(..., float64) of the float32 array
    gv, gf = MC.clean_until_stable(cu(v32), cu(f))
    same_v(gv, wv); same_f(gf, wf)
    gv64, gf64 = MC.clean_until_stable(cu(v32).double(), cu(f))
    assert torch.equal(gf, gf64) and torch.equal(gv.view(torch.int64), gv64.view(torch.int64))


@pytest.mark.parametrize("top", [2 ** 20 - 3, 2 ** 20 - 2, 2 ** 20 - 1, 2 ** 20, 2 ** 21 - 1, 2 ** 21 + 5])
def test_duplicate_order_across_the_packing_boundary(top):
    """meshproc._pack_rows changes its method where an index reaches 2^20 - 1; the order does not, here or there"""
    from surfd_amd import meshclean as MC
    f = np.array([[top, 3, 7], [7, top, 3], [2, top - 1, top], [top, top - 1, 2], [0, 1, 2], [top - 1, 5, 6], [5, 6, top - 1], [1, 0, 2]], dtype=np.int64)
    want = mp.drop_duplicate_faces(f)
    assert len(want) == 4
    same_f(MC.drop_duplicate_faces(cu(f)), want)


def test_refusals():
    from surfd_amd import meshclean as MC
    v, f = SHAPES["octahedron_minus_one"]
    dv, df = cu(v), cu(f)
    calls = [lambda v, f: MC.cull_and_merge(v, f), lambda v, f: MC.drop_degenerate_faces(v, f), lambda v, f: MC.fill_small_holes(v, f),
             lambda v, f: MC.clean_until_stable(v, f)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(torch.from_numpy(v), torch.from_numpy(f))
        with pytest.raises(ValueError):
            call(dv[:, :2], df)
        with pytest.raises(ValueError):
            call(dv, df.reshape(-1))
        with pytest.raises(TypeError):
            call(dv.half(), df)
        with pytest.raises(TypeError):
            call(dv, df.float())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MC.drop_duplicate_faces(torch.from_numpy(f))
    with pytest.raises(ValueError):
        MC.drop_duplicate_faces(df[:, :2])
    with pytest.raises(TypeError):
        MC.drop_duplicate_faces(df.double())
    # an index outside [0, V): the library's SURFD_ERR_ARG (-1), raised and not a fault; the device still answers afterwards
    for bad_index in (len(v), -1, 2 ** 31 - 1):
        bad = f.copy(); bad[3, 1] = bad_index
        for call in calls:
            with pytest.raises(RuntimeError, match=r"libsurfd_hip error -1:.*outside \[0, 6\)"):
                call(dv, cu(bad))
    with pytest.raises(RuntimeError, match="libsurfd_hip error -1:.*negative"):
        MC.drop_duplicate_faces(cu(np.array([[0, 1, 2], [0, -1, 2], [2, 1, 0]])))
    # a finite coordinate beyond the 64-bit keys, whether or not a face names the vertex
    for row in (1, 5):
        far = v.copy(); far[row, 2] = -2.0 ** 62 / 1e8
        with pytest.raises(RuntimeError, match="libsurfd_hip error -1:.*2\\^62"):
            MC.cull_and_merge(cu(far), cu(f[:3] if row == 5 else f))          # f[:3] names the vertices 0 - 4 only
    far = v.copy(); far[1, 2] = 2.0 ** 61 / 1e8
    gv, gf = MC.cull_and_merge(cu(far), df)
    wv, wf = mp.cull_and_merge(far, f)
    same_v(gv, wv); same_f(gf, wf)
    gv, gf = MC.clean_until_stable(dv, df)
    same_f(gf, host("octahedron_minus_one")["cf"])


def test_empty_meshes():
    from surfd_amd import meshclean as MC
    v, f = SHAPES["tetrahedron"]
    no_v, no_f = cu(np.zeros((0, 3))), cu(np.zeros((0, 3), dtype=np.int64))
    for dv, df in ((no_v, no_f), (cu(v), no_f), (no_v, cu(f))):
        gv, gf = MC.cull_and_merge(dv, df)
        assert tuple(gv.shape) == (0, 3) and tuple(gf.shape) == (0, 3) and gv.dtype == torch.float64 and gf.dtype == torch.int64
        gv, gf, st = MC.clean_until_stable(dv, df, return_stats=True)
        assert tuple(gv.shape) == (0, 3) and tuple(gf.shape) == (0, 3) and st["rounds"] == 1
    assert tuple(MC.drop_duplicate_faces(no_f).shape) == (0, 3)
    assert tuple(MC.drop_degenerate_faces(cu(v), no_f).shape) == (0, 3)
    assert tuple(MC.fill_small_holes(cu(v), no_f).shape) == (0, 3)
    same_f(MC.fill_small_holes(cu(v), cu(f[:2])), f[:2])     # fewer than three faces: the input


def test_get_mesh_from_udf_device_clean_is_bit_identical():
    """the decoder, latent seed and arguments of test_get_mesh_from_udf_device_post_is_bit_identical (tests/test_gpu_meshsmooth.py)"""
    from surfd_amd import synth
    from surfd_amd.cbndec import CbnDecoder, make_udf_func
    from surfd_amd.meshudf import get_mesh_from_udf
    from surfd_amd.spec import DecoderConfig
    dec = CbnDecoder(63, 32, 512, 5)
    dec.load_state_dict(synth.synth_decoder_state_dict(DecoderConfig(latent_dim=32)), strict=True)
    dec = dec.cuda().eval()
    lat = (torch.randn(1, 32, generator=torch.Generator().manual_seed(2)) * 0.8).cuda()
    field = make_udf_func(dec, lat)
    kw = dict(coords_range=(-1, 1), max_dist=0.1, N=64, max_batch=2 ** 16)
    v0, t0 = get_mesh_from_udf(field, differentiable=False, **kw)
    v1, t1 = get_mesh_from_udf(field, differentiable=False, device_clean=True, **kw)
    assert len(t0) > 0 and v1.dtype == torch.float32 and t1.dtype == torch.int64
    assert torch.equal(t0, t1) and torch.equal(v0, v1)
    v2, t2 = get_mesh_from_udf(field, differentiable=False, smooth_borders=False, device_clean=True, **kw)
    assert torch.equal(t0, t2) and torch.equal(v2, get_mesh_from_udf(field, differentiable=False, smooth_borders=False, **kw)[0])
    v3, t3 = get_mesh_from_udf(field, differentiable=True, device_clean=True, **kw)
    assert torch.equal(t0, t3)
    np.testing.assert_allclose(v3.detach().cpu().numpy(), v0.cpu().numpy(), atol=1e-6)
