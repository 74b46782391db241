"""The device hole filling (surfd_amd.meshfill, csrc/meshfill.hip) against its sequential restatement tests/meshfill_ref.py: the
faces with their caps, cap_loop and every count, bit for bit and in the same order; every length at which the kernel takes
another path (wave width, the three classes, a span longer than a wave, the first table in global memory, a table past 64 K
entries), the head of the loop at every place modulo 4, every kind of border in one call, and the C ABI with sentinels."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshfill_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

RING_LENGTHS = [3, 4, 5, 31, 32, 33, 64, 127, 128, 129, 200, 384]


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def mesh(name, *args):
    """(vertices, faces) of the named mesh of meshfill_ref, made once"""
    if name == "rings":                                       # loops of all three classes side by side, one of them with a NaN
        lengths, bad = args
        parts = [R.ring(n, seed=n) for n in lengths]
        v, f = R.side_by_side(parts)
        if bad is not None:
            v[sum(n + 1 for n in lengths[:bad]) + 1, 2] = np.nan
        return v, f
    return getattr(R, name)(*args)[:2]


@functools.lru_cache(maxsize=None)
def want(max_edges, name, *args):
    """the restatement's (faces, cap_loop, counts), computed once and shared"""
    v, f = mesh(name, *args)
    return R.fill_holes(v, f, max_edges)


def same(got, ref):
    gf, gl, gs = got
    wf, wl, ws = ref
    assert gf.dtype == torch.int64 and gl.dtype == torch.int64
    assert gs == ws, (gs, ws)
    assert tuple(gf.shape) == wf.shape and np.array_equal(gf.cpu().numpy(), wf)
    assert np.array_equal(gl.cpu().numpy(), wl)


def run(v, f, max_edges):
    from surfd_amd import meshfill as MF
    return MF.fill_holes(cu(v), cu(f), max_edges=max_edges, return_cap_loop=True, return_stats=True)


@pytest.mark.parametrize("n", RING_LENGTHS)
def test_single_rings(n):
    same(run(*mesh("ring", n, n), 1024), want(1024, "ring", n, n))


@pytest.mark.parametrize("rotate", [1, 2, 3])
@pytest.mark.parametrize("n", RING_LENGTHS)
def test_rings_with_the_head_at_every_place(n, rotate):
    same(run(*mesh("ring", n, n, rotate), 1024), want(1024, "ring", n, n, rotate))


@pytest.mark.parametrize("max_edges", [128, 1024])
def test_sheet_with_every_kind_of_border(max_edges):
    ref = want(max_edges, "bumped_sheet")
    assert ref[2]["irregular_border_edges"] > 0 and ref[2]["loops_too_long"] == (1 if max_edges == 128 else 0)
    assert ref[2]["longest_filled"] == (48 if max_edges == 128 else 160)
    same(run(*mesh("bumped_sheet"), max_edges), ref)


@pytest.mark.parametrize("max_edges", [3, 4, 32, 33, 100])
def test_sheet_at_other_limits(max_edges):
    same(run(*mesh("bumped_sheet"), max_edges), want(max_edges, "bumped_sheet"))


@pytest.mark.parametrize("bad", [None, 0, 2, 4, 5])
def test_loops_of_every_class_in_one_call_and_a_nan_among_them(bad):
    """a non-finite loop leaves a gap in the planned rows: the caps behind it move up"""
    args = ("rings", (7, 40, 3, 150, 33, 32), bad)
    ref = want(1024, *args)
    assert ref[2]["loops_nonfinite"] == (0 if bad is None else 1)
    same(run(*mesh(*args), 1024), ref)


@pytest.mark.parametrize("name", ["flat_hexagon", "flat_grid_hole"])
def test_flat_ties(name):
    same(run(*mesh(name), 128), want(128, name))


def test_punched_icosphere_is_closed_afterwards():
    from surfd_amd import meshtopo
    v, f = mesh("punched_icosphere")
    assert not meshtopo.is_closed(cu(f), len(v))
    got = run(v, f, 128)
    same(got, want(128, "punched_icosphere"))
    assert meshtopo.is_closed(got[0], len(v))
    s = meshtopo.MeshTopology(got[0], len(v)).summary()
    assert s["edge_manifold"] and s["euler_characteristic"] == 2 and s["consistently_oriented"]


def test_float32_and_int32_inputs():
    from surfd_amd import meshfill as MF
    v, f = mesh("rings", (7, 40, 3, 150, 33, 32), None)
    v32 = v.astype(np.float32)
    ref = R.fill_holes(v32.astype(np.float64), f, 1024)
    same(MF.fill_holes(cu(v32), cu(f.astype(np.int32)), 1024, True, True), ref)
    same(MF.fill_holes(cu(v32.astype(np.float64)), cu(f), 1024, True, True), ref)
    only = MF.fill_holes(cu(v), cu(f))                        # the defaults: one tensor
    assert isinstance(only, torch.Tensor) and np.array_equal(only.cpu().numpy(), want(128, "rings", (7, 40, 3, 150, 33, 32), None)[0])


def test_hole_sizes():
    from surfd_amd import meshfill as MF
    v, f = mesh("bumped_sheet")
    assert MF.hole_sizes(cu(v), cu(f)) == R.hole_sizes(f)
    v, f = mesh("ring", 1030, 1)                              # longer than any max_edges: still listed
    assert MF.hole_sizes(cu(v), cu(f)) == [1030]


def test_longest_loop_properties_only():
    """n = 1024: the restatement takes too long for the suite there.  1022 caps, every border edge matched once against its
    direction, two runs bit-identical."""
    n = 1024
    v, f = mesh("ring", n, 9, 2)
    gf, gl, st = run(v, f, 1024)
    assert st == {"loops_filled": 1, "caps": n - 2, "loops_too_long": 0, "loops_nonfinite": 0, "irregular_border_edges": 0, "border_edges": n,
                  "longest_filled": n}
    caps = gf[len(f):].cpu().numpy()
    assert caps.shape == (n - 2, 3) and bool((gl == 0).all())
    half = np.concatenate([caps[:, [0, 1]], caps[:, [1, 2]], caps[:, [2, 0]]])
    key = half[:, 0] * (n + 1) + half[:, 1]
    border = f[:, 1] * (n + 1) + f[:, 0]                      # the ring's edges (f[:, 0] -> f[:, 1]) reversed
    assert np.array_equal(np.sort(key[np.isin(key, border)]), np.sort(border))
    inner = key[~np.isin(key, border)]                        # every diagonal once in each direction
    back = half[:, 1] * (n + 1) + half[:, 0]
    assert len(inner) == 2 * (n - 3) and len(np.unique(inner)) == len(inner) and np.array_equal(np.sort(inner), np.sort(back[~np.isin(key, border)]))
    again = run(v, f, 1024)
    assert torch.equal(again[0], gf) and torch.equal(again[1], gl) and again[2] == st


def test_repeated_runs_are_bit_identical():
    v, f = mesh("bumped_sheet")
    first = run(v, f, 1024)
    same(first, want(1024, "bumped_sheet"))
    for _ in range(4):
        got = run(v, f, 1024)
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]) and got[2] == first[2]


def test_raw_abi_writes_stop_at_the_counts():
    """the C ABI as it is: caps and cap_loop carry a sentinel and TAIL rows more than planned; plan's counts, run's counts, the
    rows written and nothing behind them; the handle runs twice; too few rows are refused and write nothing"""
    from surfd_amd import _native as N
    L, TAIL, SENT = N.lib(), 7, -77
    for args in (("rings", (7, 40, 3, 150, 33, 32), 2), ("bumped_sheet",)):
        v, f = mesh(*args)
        wf, wl, ws = want(1024, *args)
        dv, df = cu(v), cu(f.astype(np.int32))
        pc, rc, h = (C.c_int64 * 7)(), (C.c_int64 * 7)(), C.c_void_p()
        N.check(L.surfd_meshfill_plan(N.ptr(dv), len(v), N.ptr(df), len(f), 1024, pc, N.stream(), C.byref(h)))
        planned = dict(zip(R.COUNT_KEYS, pc))
        assert planned["loops_filled"] == ws["loops_filled"] + ws["loops_nonfinite"] and planned["loops_nonfinite"] == 0
        assert planned["caps"] >= ws["caps"] and planned["border_edges"] == ws["border_edges"] and planned["irregular_border_edges"] == ws["irregular_border_edges"]
        rows = planned["caps"]
        for _ in range(2):
            caps = torch.full((rows + TAIL, 3), SENT, dtype=torch.int32, device="cuda")
            loop = torch.full((rows + TAIL,), SENT, dtype=torch.int32, device="cuda")
            N.check(L.surfd_meshfill_run(h, N.ptr(caps), rows + TAIL, N.ptr(loop), rc, N.stream()))
            assert dict(zip(R.COUNT_KEYS, rc)) == ws
            n = ws["caps"]
            assert np.array_equal(caps[:n].cpu().numpy(), wf[len(f):]) and np.array_equal(loop[:n].cpu().numpy(), wl)
            assert bool((caps[n:] == SENT).all()) and bool((loop[n:] == SENT).all())
        caps = torch.full((rows + TAIL, 3), SENT, dtype=torch.int32, device="cuda")
        N.check(L.surfd_meshfill_run(h, N.ptr(caps), rows, None, rc, N.stream()))           # cap_loop is optional
        assert np.array_equal(caps[:ws["caps"]].cpu().numpy(), wf[len(f):]) and bool((caps[ws["caps"]:] == SENT).all())
        caps.fill_(SENT)
        assert L.surfd_meshfill_run(h, N.ptr(caps), rows - 1, None, rc, N.stream()) == -1 and bool((caps == SENT).all())      # SURFD_ERR_ARG
        sizes = torch.full((len(R.hole_sizes(f)) + TAIL,), SENT, dtype=torch.int32, device="cuda")
        N.check(L.surfd_meshfill_loop_sizes(h, N.ptr(sizes), len(sizes), N.stream()))
        assert sorted(sizes[:-TAIL].tolist()) == R.hole_sizes(f) and bool((sizes[-TAIL:] == SENT).all())
        L.surfd_meshfill_destroy(h)
    h = C.c_void_p(123)
    for bad in (2, 1025):
        assert L.surfd_meshfill_plan(N.ptr(dv), len(v), N.ptr(df), len(f), bad, pc, N.stream(), C.byref(h)) == -1 and h.value is None


def test_refusals():
    from surfd_amd import meshfill as MF
    v, f = mesh("ring", 8, 8)
    dv, df = cu(v), cu(f)
    for call in (lambda v, f: MF.fill_holes(v, f), lambda v, f: MF.hole_sizes(v, f)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(torch.from_numpy(v), torch.from_numpy(f))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(dv, torch.from_numpy(f))
        with pytest.raises(ValueError):
            call(dv[:, :2], df)
        with pytest.raises(ValueError):
            call(dv, df.reshape(-1))
        with pytest.raises(TypeError):
            call(dv.half(), df)
        with pytest.raises(TypeError):
            call(dv, df.float())
    for bad in (2, 1025, 0, -1, 64.0, True):
        with pytest.raises(ValueError, match="max_edges"):
            MF.fill_holes(dv, df, max_edges=bad)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="one device"):
            MF.fill_holes(dv, df.to("cuda:1"))
    # an index outside [0, V): the library's SURFD_ERR_ARG (-1), raised and not a fault; the device still answers afterwards
    for bad_index in (len(v), -1, 2 ** 31 - 1):
        bad = f.copy(); bad[3, 1] = bad_index
        with pytest.raises(RuntimeError, match=r"libsurfd_hip error -1:.*outside \[0, 9\)"):
            MF.fill_holes(dv, cu(bad))
    same(run(v, f, 128), want(128, "ring", 8, 8))


def test_empty_meshes():
    from surfd_amd import meshfill as MF
    v, f = mesh("ring", 8, 8)
    no_v, no_f = cu(np.zeros((0, 3))), cu(np.zeros((0, 3), dtype=np.int64))
    zero = dict.fromkeys(R.COUNT_KEYS, 0)
    for dv, df in ((no_v, no_f), (cu(v), no_f), (no_v, cu(f))):
        gf, gl, st = MF.fill_holes(dv, df, return_cap_loop=True, return_stats=True)
        assert torch.equal(gf, df) and tuple(gl.shape) == (0,) and gl.dtype == torch.int64 and st == zero
        assert MF.hole_sizes(dv, df) == []
    closed = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])          # nothing to fill: the faces as they came
    gf, gl, st = MF.fill_holes(cu(v[:4]), cu(closed), return_cap_loop=True, return_stats=True)
    assert np.array_equal(gf.cpu().numpy(), closed) and len(gl) == 0 and st == zero


def test_get_mesh_from_udf_fill_holes(monkeypatch):
    """fill_holes=N runs surfd_amd.meshfill.fill_holes on the device_clean=True mesh, right after the cleaning: with the border
    smoothing off the vertices are those of device_clean=True and the faces are fill_holes' of them.  The decoder, latent seed
    and arguments of test_get_mesh_from_udf_device_clean_is_bit_identical (tests/test_gpu_meshclean.py)."""
    from surfd_amd import meshfill as MF, synth
    from surfd_amd.cbndec import CbnDecoder, make_udf_func
    from surfd_amd.meshudf import get_mesh_from_udf
    from surfd_amd.spec import DecoderConfig
    dec = CbnDecoder(63, 32, 512, 5)
    dec.load_state_dict(synth.synth_decoder_state_dict(DecoderConfig(latent_dim=32)), strict=True)
    dec = dec.cuda().eval()
    lat = (torch.randn(1, 32, generator=torch.Generator().manual_seed(2)) * 0.8).cuda()
    field = make_udf_func(dec, lat)
    kw = dict(coords_range=(-1, 1), max_dist=0.1, N=64, max_batch=2 ** 16, differentiable=False, smooth_borders=False)
    v0, t0 = get_mesh_from_udf(field, device_clean=True, **kw)
    seen = []
    real = MF.fill_holes

    def spy(vertices, faces, **kwargs):
        out = real(vertices, faces, **kwargs)
        seen.append((vertices, faces, kwargs, out))
        return out
    monkeypatch.setattr(MF, "fill_holes", spy)
    v2, t2 = get_mesh_from_udf(field, device_clean=True, fill_holes=64, **kw)
    v1, t1, stats = get_mesh_from_udf(field, device_clean=True, fill_holes=64, return_fill_stats=True, **kw)
    assert torch.equal(v1, v2) and torch.equal(t1, t2)
    del seen[0]
    (sv, sf, skw, sout), = seen
    assert skw == {"max_edges": 64, "return_stats": True} and sv.dtype == torch.float64 and torch.equal(sv.float(), v0) and torch.equal(sf, t0)
    assert torch.equal(v1, v0) and torch.equal(t1, sout[0]) and torch.equal(t1[:len(t0)], t0)
    ref = R.fill_holes(sv.cpu().numpy(), sf.cpu().numpy(), 64)
    assert np.array_equal(t1.cpu().numpy(), ref[0]) and stats == ref[2] == sout[1]
    for bad in (dict(device_clean=False), dict(device_clean=True, differentiable=True)):
        with pytest.raises(ValueError, match="fill_holes"):
            get_mesh_from_udf(field, fill_holes=64, **{**kw, **bad})
    with pytest.raises(ValueError, match="return_fill_stats"):
        get_mesh_from_udf(field, device_clean=True, return_fill_stats=True, **kw)
    with pytest.raises(ValueError, match="fill_holes must be"):
        get_mesh_from_udf(field, device_clean=True, fill_holes=2, **kw)
