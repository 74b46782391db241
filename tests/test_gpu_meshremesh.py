"""The device remeshing (surfd_amd/meshremesh.py: remesh_isotropic, csrc/meshremesh.hip) against tests/meshremesh_ref.py, bit for
bit and in the same order: vertices as int64 views, faces, origin and every count of every iteration.  The meshes of the CPU tests,
sheets whose edges, vertices and faces cross the 64- and 256-lane boundaries, runs longer than a wave, each stage alone, growth of
the handle, the knobs, input variants, unkept faces, 100 random soups, the projection, repeated runs, the C ABI with sentinels behind
its outputs, the refusals and the consumer."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshremesh_ref as R  # noqa: E402
import meshsimplify_ref as MS  # noqa: E402

pytestmark = pytest.mark.gpu


def cu(x, dtype=None):
    t = torch.from_numpy(np.array(x))                         # a copy: the shared references are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "sheet17_flat":
        v, f = R.sheet_mesh(17, 17)
    elif name == "sheet17":
        v, f = R.sheet_mesh(17, 17, bump=0.3)
    elif name == "sheet40":                                     # 3 200 faces, 1 681 vertices, 4 880 edges
        v, f = R.sheet_mesh(40, 40, bump=0.3)
    elif name == "sheet2x130":                                  # rows of 131 vertices: runs longer than a wave along one axis
        v, f = R.sheet_mesh(2, 130, bump=0.3)
    elif name == "cube24":
        v, f = MS.cube_mesh(24)
    elif name == "icosphere":
        v, f = R.icosphere(3)
    elif name == "icosphere1":
        v, f = R.icosphere(1)
    elif name == "triangle":
        v, f = np.eye(3), np.array([[0, 1, 2]])
    elif name.startswith("rough_"):                             # a mesh with uneven valences: one pass of collapses alone over a named mesh
        bv, bf = mesh(name[6:])
        v, f, _, _ = R.remesh(bv, bf, 1.6 * R.mean_edge_length(bv, bf), iterations=1, split_rounds=0, flip_rounds=0, relax_sweeps=0)
    else:
        v, f = getattr(R, name if name in ("tetrahedron", "octahedron", "cube12", "two_spheres") else name + "_mesh")()
    v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int64)
    v.setflags(write=False); f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def length(name):
    return R.mean_edge_length(*mesh(name))


@functools.lru_cache(maxsize=None)
def want(name, scale, **kw):
    """the restatement on a named mesh at scale times its mean edge length, worked out once and shared"""
    out = R.remesh(*mesh(name), scale * length(name), **kw)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def same(got, ref):
    gv, gf, go, gs = got
    wv, wf, wo, ws = ref
    assert gv.is_cuda and gf.is_cuda and go.is_cuda and gv.dtype == torch.float64 and gf.dtype == torch.int64 and go.dtype == torch.int64
    assert gs == ws, [(i, k, a[k], b[k]) for i, (a, b) in enumerate(zip(gs, ws)) for k in b if a[k] != b[k]] or (len(gs), len(ws))
    assert tuple(gv.shape) == wv.shape and tuple(gf.shape) == wf.shape and tuple(go.shape) == wo.shape
    assert np.array_equal(gf.cpu().numpy(), wf), f"{int((gf.cpu().numpy() != wf).any(axis=1).sum())} faces differ"
    assert np.array_equal(go.cpu().numpy(), wo), f"{int((go.cpu().numpy() != wo).sum())} origins differ"
    a, b = gv.cpu().numpy().view(np.int64), np.ascontiguousarray(wv).view(np.int64)
    assert np.array_equal(a, b), f"{int((a != b).sum())} of {a.size} doubles differ"


def run(v, f, L, **kw):
    from surfd_amd.meshremesh import remesh_isotropic
    return remesh_isotropic(v if isinstance(v, torch.Tensor) else cu(v), f if isinstance(f, torch.Tensor) else cu(f), L, return_origin=True,
                            return_stats=True, **kw)


NAMES = ["tetrahedron", "octahedron", "cube12", "triangle", "two_spheres", "icosphere", "torus", "sheet17", "sheet17_flat", "sheet40", "sheet2x130",
         "cube24"]


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_restatement(name, scale):
    same(run(*mesh(name), scale * length(name), iterations=3), want(name, scale, iterations=3))


STAGES = {"split": (0.5, dict(collapse_rounds=0, flip_rounds=0, relax_sweeps=0)), "collapse": (1.6, dict(split_rounds=0, flip_rounds=0, relax_sweeps=0)),
          "flip": (1.0, dict(split_rounds=0, collapse_rounds=0, relax_sweeps=0)), "relax": (1.0, dict(split_rounds=0, collapse_rounds=0, flip_rounds=0))}


@pytest.mark.parametrize("stage", list(STAGES))
@pytest.mark.parametrize("name", ["sheet40", "icosphere"])
def test_each_stage_alone(name, stage):
    scale, kw = STAGES[stage]
    name = ("rough_" + name) if stage in ("flip", "relax") else name      # flips need uneven valences to find anything
    ref = want(name, scale, iterations=2, **kw)
    moved = {"split": "splits", "collapse": "collapses", "flip": "flips", "relax": "relaxed"}[stage]
    assert ref[3][0][moved] > 0 and all(ref[3][0][k] == 0 for k in ("splits", "collapses", "flips", "relaxed") if k != moved)
    same(run(*mesh(name), scale * length(name), iterations=2, **kw), ref)


def test_the_handle_grows_and_is_reused():
    """the level-1 icosphere at an eighth of its edge: at least sixteen times the faces, through several re-allocations; then a
    handle stepped eight times, compared after every step"""
    from surfd_amd.meshremesh import MeshRemesher
    v, f = mesh("icosphere1")
    ref = want("icosphere1", 0.125)
    assert len(ref[1]) >= 16 * len(f)
    same(run(v, f, 0.125 * length("icosphere1")), ref)
    low2, high2 = R.bounds2(0.25 * length("icosphere1"))
    dev, host = MeshRemesher(cu(v), cu(f), low2, high2, seed=3), R.Remesher(v, f, low2, high2, seed=3)
    sizes = []
    for it in range(8):
        gs, ws = dev.iterate(), host.iterate()
        assert gs == ws, (it, [(k, gs[k], ws[k]) for k in ws if gs[k] != ws[k]])
        gv, gf, go = dev.emit()
        wv, wf, wo = host.emit()
        assert np.array_equal(gf.cpu().numpy(), wf) and np.array_equal(go.cpu().numpy(), wo), it
        assert np.array_equal(gv.cpu().numpy().view(np.int64), np.ascontiguousarray(wv).view(np.int64)), it
        assert dev.sizes() == (len(host.X), len(host.fa))
        x, o = dev.positions()
        assert np.array_equal(x.cpu().numpy().view(np.int64), np.ascontiguousarray(host.X).view(np.int64)) and np.array_equal(o.cpu().numpy(), host.origin)
        sizes.append(dev.sizes())
    assert sizes[0][1] > 4 * len(f)


KNOBS = [dict(seed=7), dict(seed=2 ** 64 - 1), dict(flip_cos=0.0), dict(flip_cos=0.9), dict(relax=0.5), dict(relax_sweeps=3), dict(low=0.5, high=2.0),
         dict(split_rounds=0), dict(split_rounds=1), dict(collapse_rounds=0), dict(collapse_rounds=1), dict(flip_rounds=0), dict(flip_rounds=1),
         dict(relax_sweeps=0), dict(iterations=0), dict(iterations=1)]


@pytest.mark.parametrize("kw", KNOBS, ids=str)
def test_knobs(kw):
    for name, scale in (("torus", 0.7), ("rough_sheet40", 1.3)):
        kw3 = dict(dict(iterations=3), **kw)
        same(run(*mesh(name), scale * length(name), **kw3), want(name, scale, **kw3))


def test_input_variants():
    v, f = mesh("sheet17")
    L = 0.7 * length("sheet17")
    ref = want("sheet17", 0.7, iterations=2)
    v32 = v.astype(np.float32)
    ref32 = R.remesh(v32.astype(np.float64), f, L, iterations=2)
    same(run(cu(v32), cu(f, torch.int32), L, iterations=2), ref32)
    same(run(cu(v32), cu(f), L, iterations=2), ref32)
    same(run(cu(v), cu(f, torch.int32), L, iterations=2), ref)
    wide_v, wide_f = torch.zeros(len(v), 6, dtype=torch.float64, device="cuda"), torch.zeros(len(f), 5, dtype=torch.int64, device="cuda")
    wide_v[:, ::2], wide_f[:, 1:4] = cu(v), cu(f)
    assert not wide_v[:, ::2].is_contiguous() and not wide_f[:, 1:4].is_contiguous()
    same(run(wide_v[:, ::2], wide_f[:, 1:4], L, iterations=2), ref)
    order = np.random.default_rng(5).permutation(len(f))
    for g in (f[::-1], f[order], f[order][:, [1, 2, 0]]):
        same(run(v, np.ascontiguousarray(g), L, iterations=2), R.remesh(v, g, L, iterations=2))
    from surfd_amd.meshremesh import remesh_isotropic
    two = remesh_isotropic(cu(v), cu(f), L, iterations=2)
    assert len(two) == 2 and np.array_equal(two[0].cpu().numpy().view(np.int64), ref[0].view(np.int64)) and np.array_equal(two[1].cpu().numpy(), ref[1])


def test_unkept_faces_and_empty_meshes():
    nan, inf = float("nan"), float("inf")
    v, f = mesh("octahedron")
    for vv, ff in ((np.zeros((0, 3)), np.zeros((0, 3), np.int64)), (v, np.zeros((0, 3), np.int64)), (np.full((4, 3), nan), np.array([[0, 1, 2], [1, 2, 3]])),
                   (np.array([[0, 0, 0], [inf, 0, 0], [0, 1, 0.]]), np.array([[0, 1, 2]])), (np.eye(3), np.array([[0, 1, 1], [2, 2, 2]]))):
        for L in (0.3, 5.0):
            same(run(vv, ff, L, iterations=2), R.remesh(vv, ff, L, iterations=2))
    # a NaN vertex, an unreferenced vertex, a face that names a vertex twice, -0.0
    v2 = np.concatenate((v, [[nan, 0, 0], [9.0, 9, 9], [0.5, -0.0, 0.5]]))
    f2 = np.concatenate(([[0, 6, 2]], f[:4], [[8, 8, 1], [3, 8, 3]], f[4:]))
    for L in (0.4, 1.0, 3.0):
        same(run(v2, f2, L, iterations=2), R.remesh(v2, f2, L, iterations=2))


def soup(seed):
    g = np.random.default_rng(seed)
    v = g.integers(-3, 4, size=(24, 3)).astype(np.float64) if seed % 3 == 0 else g.normal(size=(24, 3))
    f = g.integers(0, 24, size=(40, 3))                         # repeated indices happen by themselves
    f[g.integers(0, 40)] = f[g.integers(0, 40)]                 # a duplicate face
    f[g.integers(0, 40)] = f[g.integers(0, 40)][::-1]           # and one turned over
    for value in (float("nan"), float("inf"), -0.0):
        if g.random() < 0.4:
            v[g.integers(0, 24), g.integers(0, 3)] = value
    return v, f


@pytest.mark.parametrize("block", range(4))
def test_random_soups_are_equal_and_clean(block):
    """non-manifold input: nothing is promised of its shape, but the device equals the restatement and the output is clean"""
    for seed in range(25 * block, 25 * block + 25):
        v, f = soup(seed)
        L = (0.8, 2.0, 5.0)[seed % 3]
        got = run(v, f, L, iterations=2, seed=seed)
        same(got, R.remesh(v, f, L, iterations=2, seed=seed))
        gv, gf = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert np.isfinite(gv).all() and (len(gf) == 0 or (gf.min() >= 0 and gf.max() == len(gv) - 1))
        assert ((gf[:, 0] != gf[:, 1]) & (gf[:, 1] != gf[:, 2]) & (gf[:, 0] != gf[:, 2])).all() and len(np.unique(gf)) == len(gv)


@pytest.mark.parametrize("name", ["icosphere", "sheet17"])
@pytest.mark.parametrize("accel", ["tiles", "bvh"])
def test_projection_onto_the_input(name, accel):
    from surfd_amd.meshprep import closest_points
    v, f = mesh(name)
    dv, df = cu(v, torch.float32), cu(f)

    def project(points):
        return closest_points(dv, df, cu(points, torch.float32), accel=accel)[1].double().cpu().numpy()

    L = 0.6 * length(name)
    got = run(v, f, L, iterations=3, project=True, accel=accel)
    same(got, R.remesh(v, f, L, iterations=3, project=project))
    gv, go = got[0].cpu().numpy(), got[2].cpu().numpy()
    kept = go >= 0
    assert (~kept).any() and np.array_equal(gv[kept].view(np.int64), v[go[kept]].view(np.int64))
    assert kept.any() == (name == "sheet17")                    # on the closed sphere every vertex relaxes; the sheet's border stays
    if name == "icosphere":                                      # projected vertices lie on the input's facets: inside the unit sphere
        r = np.sqrt((gv ** 2).sum(axis=1))
        assert r.max() <= 1 + 1e-6 and r.min() >= np.cos(0.2)


def test_ten_runs_are_identical():
    v, f = mesh("rough_sheet40")
    dv, df = cu(v), cu(f)
    L = 1.2 * length("rough_sheet40")
    first = run(dv, df, L, iterations=3)
    assert sum(s["flips"] for s in first[3]) > 0                # the atomicMin path is taken
    for _ in range(9):
        again = run(dv, df, L, iterations=3)
        assert torch.equal(again[0].view(torch.int64), first[0].view(torch.int64)) and torch.equal(again[1], first[1])
        assert torch.equal(again[2], first[2]) and again[3] == first[3]


def test_raw_abi_writes_stop_at_the_counts():
    """the C ABI as it is: outputs of the handle's sizes and TAIL rows more, filled with a sentinel; nothing behind the counts is
    written, everything before them is"""
    from surfd_amd import _native as N
    TAIL = 64
    v, f = mesh("sheet40")
    L = 0.7 * length("sheet40")
    low2, high2 = R.bounds2(L)
    host = R.Remesher(v, f, low2, high2)
    wc = host.iterate()
    wv, wf, wo = host.emit()
    dv, df = cu(v), cu(f, torch.int32)
    lib, st = N.lib(), N.stream()
    h = C.c_void_p()

    def create(V=len(v), F=len(f), lo=low2, hi=high2, fc=0.2, faces=df):
        return lib.surfd_meshremesh_create(N.ptr(dv), V, N.ptr(faces), F, lo, hi, fc, 0, st, C.byref(h))
    nan, inf = float("nan"), float("inf")
    for kw in (dict(lo=0.0), dict(lo=nan), dict(hi=inf), dict(lo=high2, hi=low2), dict(fc=1.0), dict(fc=-0.1), dict(fc=nan), dict(F=-1), dict(V=-1)):
        assert create(**kw) == -1 and not h.value, kw
    assert create(V=0) == -1 and not h.value and b"outside [0, 0)" in lib.surfd_last_error()      # no vertices: every index is outside
    assert create(F=2 ** 30) == -4 and not h.value                 # 3 F >= 2^31: by the size arguments alone
    bad = f.copy(); bad[77, 2] = len(v)
    assert create(faces=cu(bad, torch.int32)) == -1 and not h.value and b"outside [0, 1681)" in lib.surfd_last_error()
    N.check(create())
    try:
        counts = (C.c_int64 * 26)(*([-5] * 26))
        for kw in (dict(s=-1), dict(c=-1), dict(fl=-1), dict(r=-1), dict(relax=0.0), dict(relax=1.5), dict(relax=nan)):
            assert lib.surfd_meshremesh_iterate(h, kw.get("s", 4), kw.get("c", 16), kw.get("fl", 4), kw.get("r", 1), kw.get("relax", 1.0), counts, st) == -1, kw
        counts = (C.c_int64 * 26)(*([-5] * 26))
        N.check(lib.surfd_meshremesh_iterate(h, 4, 16, 4, 1, 1.0, counts, st))
        assert list(counts) == [wc[k] for k in R.COUNT_NAMES] + [-5, -5]
        nv, nf = C.c_int64(), C.c_int64()
        N.check(lib.surfd_meshremesh_sizes(h, C.byref(nv), C.byref(nf)))
        assert (nv.value, nf.value) == (len(host.X), len(host.fa))
        V, F = nv.value, nf.value
        ov = torch.full((V + TAIL, 3), -7.5e300, dtype=torch.float64, device="cuda")
        of = torch.full((F + TAIL, 3), -77, dtype=torch.int32, device="cuda")
        oo = torch.full((V + TAIL,), -77, dtype=torch.int32, device="cuda")
        px = torch.full((V + TAIL, 3), -7.5e300, dtype=torch.float64, device="cuda")
        po = torch.full((V + TAIL,), -77, dtype=torch.int32, device="cuda")
        two = (C.c_int64 * 4)(*([-5] * 4))
        N.check(lib.surfd_meshremesh_emit(h, N.ptr(ov), N.ptr(of), N.ptr(oo), two, st))
        N.check(lib.surfd_meshremesh_get_positions(h, N.ptr(px), N.ptr(po), st))
        torch.cuda.synchronize()
        assert list(two) == [len(wv), len(wf), -5, -5]
        n = len(wv)
        assert bool((ov[n:] == -7.5e300).all()) and bool((of[F:] == -77).all()) and bool((oo[n:] == -77).all())
        assert bool((px[V:] == -7.5e300).all()) and bool((po[V:] == -77).all())
        assert np.array_equal(ov[:n].cpu().numpy().view(np.int64), wv.view(np.int64)) and np.array_equal(of[:F].cpu().numpy(), wf)
        assert np.array_equal(oo[:n].cpu().numpy(), wo) and np.array_equal(po[:V].cpu().numpy(), host.origin)
        assert np.array_equal(px[:V].cpu().numpy().view(np.int64), np.ascontiguousarray(host.X).view(np.int64))
        # positions set and read back; emit without the origin
        moved = px[:V].clone() + 1.0
        N.check(lib.surfd_meshremesh_set_positions(h, N.ptr(moved), st))
        N.check(lib.surfd_meshremesh_get_positions(h, N.ptr(px), None, st))
        N.check(lib.surfd_meshremesh_emit(h, N.ptr(ov), N.ptr(of), None, two, st))
        torch.cuda.synchronize()
        assert torch.equal(px[:V], moved) and bool((px[V:] == -7.5e300).all()) and list(two)[:2] == [len(wv), len(wf)]
    finally:
        lib.surfd_meshremesh_destroy(h)


def test_refusals_come_back_as_errors_and_the_stream_goes_on():
    from surfd_amd.meshremesh import remesh_isotropic
    v, f = mesh("octahedron")
    dv, df = cu(v), cu(f)
    for bad_index in (len(v), -1, 2 ** 31 - 1):
        bad = f.copy(); bad[5, 1] = bad_index
        with pytest.raises(RuntimeError, match=r"libsurfd_hip error -1:.*outside \[0, 6\)"):
            remesh_isotropic(dv, cu(bad), 1.0)
        same(run(dv, df, 0.8, iterations=2), want("octahedron", 0.8 / length("octahedron"), iterations=2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        remesh_isotropic(torch.from_numpy(np.array(v)), torch.from_numpy(np.array(f)), 1.0)
    nan = float("nan")
    for kw in (dict(target_edge_length=0.0), dict(target_edge_length=nan), dict(target_edge_length=float("inf")), dict(target_edge_length=1.0, low=0.0),
               dict(target_edge_length=1.0, low=2.0), dict(target_edge_length=1.0, high=nan), dict(target_edge_length=1.0, relax=0.0),
               dict(target_edge_length=1.0, relax=1.1), dict(target_edge_length=1.0, flip_cos=1.0), dict(target_edge_length=1.0, flip_cos=nan),
               dict(target_edge_length=1.0, iterations=-1), dict(target_edge_length=1.0, split_rounds=1.5), dict(target_edge_length=1.0, flip_rounds=-1),
               dict(target_edge_length=1.0, project=True, accel="grid")):
        with pytest.raises(ValueError):
            remesh_isotropic(dv, df, **kw)
    with pytest.raises(ValueError):
        remesh_isotropic(dv[:, :2], df, 1.0)
    with pytest.raises(TypeError):
        remesh_isotropic(dv.half(), df, 1.0)
    with pytest.raises(TypeError):
        remesh_isotropic(dv, df.float(), 1.0)


def test_the_torch_measures():
    from surfd_amd.meshremesh import mean_edge_length, triangle_quality
    v, f = mesh("rough_sheet40")
    L = length("rough_sheet40")
    assert abs(mean_edge_length(cu(v), cu(f)) - L) <= 1e-12 * L
    a, b = R.triangle_quality(v, f, L), triangle_quality(cu(v), cu(f), L)
    assert a.keys() == b.keys() and all(abs(a[k] - b[k]) <= 1e-9 * max(1.0, abs(a[k])) for k in a)


def test_get_mesh_from_udf_remesh_edge(monkeypatch):
    """the decoder, latent seed and arguments of test_get_mesh_from_udf_simplify_faces (tests/test_gpu_meshdecimate.py): the flag gives
    remesh_isotropic of the mesh the same call gives without it.  That mesh is float64 inside the call and comes back as float32, so
    the call's own remesh_isotropic is watched: what goes in is the mesh of the call without the flag, what comes out is returned
    (borders are not smoothed here: the smoothing comes after)."""
    from surfd_amd import meshremesh, synth
    from surfd_amd.cbndec import CbnDecoder, make_udf_func
    from surfd_amd.meshudf import get_mesh_from_udf
    from surfd_amd.spec import DecoderConfig
    dec = CbnDecoder(63, 32, 512, 5)
    dec.load_state_dict(synth.synth_decoder_state_dict(DecoderConfig(latent_dim=32)), strict=True)
    dec = dec.cuda().eval()
    lat = (torch.randn(1, 32, generator=torch.Generator().manual_seed(2)) * 0.8).cuda()
    field = make_udf_func(dec, lat)
    kw = dict(coords_range=(-1, 1), max_dist=0.1, N=64, max_batch=2 ** 16)
    with pytest.raises(ValueError, match="remesh_edge.*differentiable"):
        get_mesh_from_udf(field, device_clean=True, remesh_edge=0.05, **kw)
    with pytest.raises(ValueError, match="remesh_edge.*device_clean"):
        get_mesh_from_udf(field, differentiable=False, remesh_edge=0.05, **kw)
    with pytest.raises(ValueError, match="remesh_edge"):
        get_mesh_from_udf(field, differentiable=False, device_clean=True, remesh_edge=0.0, **kw)
    v0, t0 = get_mesh_from_udf(field, differentiable=False, device_clean=True, smooth_borders=False, **kw)
    L = 0.5 * meshremesh.mean_edge_length(v0, t0)
    calls, real = [], meshremesh.remesh_isotropic

    def watched(v, f, length, **kwargs):
        out = real(v, f, length, **kwargs)
        calls.append((v, f, length, kwargs, out))
        return out

    monkeypatch.setattr(meshremesh, "remesh_isotropic", watched)
    v1, t1 = get_mesh_from_udf(field, differentiable=False, device_clean=True, smooth_borders=False, remesh_edge=L, remesh_iterations=2, **kw)
    (v, f, length, kwargs, (wv, wt)), = calls
    print(f"{len(t0)} faces -> {len(t1)} at L = {L}")
    assert v.dtype == torch.float64 and torch.equal(v.float(), v0) and torch.equal(f.long(), t0) and length == L
    assert kwargs == dict(iterations=2)
    assert len(t1) > len(t0) and v1.dtype == torch.float32 and t1.dtype == torch.int64 and v1.is_cuda
    assert torch.equal(t1, wt) and torch.equal(v1, wv.float())
