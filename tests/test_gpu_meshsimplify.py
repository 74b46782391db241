"""The device simplification (surfd_amd/meshsimplify.py, csrc/meshsimplify.hip) against tests/meshsimplify_ref.py, bit for bit and in
the same order: vertices as int64 views, faces, the map and the counts, for both representatives.  The hand-made shapes of the CPU
tests, the cube and the sphere, one cluster only (a corner sort over zero key bits), one cell of 70 000 vertices, keys that differ
in their top and in their lowest bit, edge sizes, input variants, 200 random soups, repeated runs, the C ABI with sentinels behind
its outputs, the refusals and the two consumers."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshsimplify_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
REPS = ("mean", "quadric")
CELLS = (0.071, 0.1, 0.13, 0.21)


def cu(x, dtype=None):
    t = torch.from_numpy(np.array(x))                         # a copy: the shared references are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "cube":
        v, f = R.cube_mesh(24)
    elif name == "sphere":
        v, f = R.sphere_mesh()
    elif name == "sphere_faces_shuffled":
        v, f = mesh("sphere")
        f = f[np.random.default_rng(5).permutation(len(f))]
    elif name == "sphere_vertices_shuffled":
        v, f = mesh("sphere")
        p = np.random.default_rng(6).permutation(len(v))      # new index i holds the old vertex p[i]
        inv = np.empty_like(p); inv[p] = np.arange(len(p))
        v, f = v[p], inv[f]
    elif name == "crowd":
        # 70 000 vertices in ONE cell of side 2 and 23 334 faces among them that name every one (70 002 corner records for that
        # cell), three more cells with one vertex each and four faces to them
        g = np.random.default_rng(7)
        v = np.concatenate((g.random((70000, 3)), [[2.5, 0.5, 0.5], [0.5, 2.5, 0.5], [0.5, 0.5, 2.5]]))
        f = np.concatenate((np.append(g.permutation(70000), [1, 2]).reshape(-1, 3), [[5, 70000, 70001], [9, 70001, 70002], [70002, 70000, 17], [70000, 70001, 70002]]))
    else:
        raise KeyError(name)
    v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int64)
    v.setflags(write=False); f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def want(name, cell, rep, origin=None):
    """the restatement on a named mesh, worked out once and shared (callers do not write to it)"""
    out = R.simplify(*mesh(name), cell, origin=origin, representative=rep)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def same(got, ref):
    gv, gf, gm, gs = got
    wv, wf, wm, wc = ref
    assert gv.is_cuda and gf.is_cuda and gm.is_cuda and gv.dtype == torch.float64 and gf.dtype == torch.int64 and gm.dtype == torch.int64
    assert gs == wc, (gs, wc)
    assert tuple(gv.shape) == wv.shape and tuple(gf.shape) == wf.shape and tuple(gm.shape) == wm.shape
    assert np.array_equal(gm.cpu().numpy(), wm), f"{int((gm.cpu().numpy() != wm).sum())} map entries differ"
    assert np.array_equal(gf.cpu().numpy(), wf), f"{int((gf.cpu().numpy() != wf).any(axis=1).sum())} faces differ"
    a, b = gv.cpu().numpy().view(np.int64), np.ascontiguousarray(wv).view(np.int64)
    assert np.array_equal(a, b), f"{int((a != b).sum())} of {a.size} doubles differ"


def run(v, f, cell, rep, **kw):
    from surfd_amd.meshsimplify import simplify_vertex_clustering
    return simplify_vertex_clustering(v if isinstance(v, torch.Tensor) else cu(v), f if isinstance(f, torch.Tensor) else cu(f), cell,
                                      representative=rep, return_map=True, return_stats=True, **kw)


def check(v, f, cell, rep, origin=None, rank_tol=1e-3):
    with np.errstate(all="ignore"):
        ref = R.simplify(v, f, cell, origin=origin, representative=rep, rank_tol=rank_tol)
    same(run(v, f, cell, rep, origin=origin, rank_tol=rank_tol), ref)
    return ref


@pytest.mark.parametrize("rep", REPS)
def test_hand_made_shapes(rep):
    v, f = R.hand_mesh()
    assert check(v, f, 1.0, rep, origin=(0.0, 0.0, 0.0))[3]["clusters"] == 4
    check(v, f, 1.0, rep)
    check(v, f, 0.3, rep)
    for xs in ([1e16, 1.0, -1e16], [1e16, -1e16, 1.0], [1.0, 1e16, -1e16]):
        check(*R.order_mesh(xs), 4e16, rep, origin=(-2e16, 0.0, 0.0))
    check(*R.edge_triangle(2.0 ** 21 - 0.5), 1.0, rep, origin=(0.0, 0.0, 0.0))
    check(*R.edge_triangle(2.5), 1.0, rep, origin=(0.5, 0.5, 0.5))
    flat, par = R.flat_and_parallel_meshes()
    check(*flat, 1.0, rep, origin=(0.0, 0.0, 0.0))
    ref = check(*par, 1.0, rep, origin=(0.0, 0.0, 0.0), rank_tol=1e-12)
    assert rep == "mean" or ref[3]["fallbacks"] >= 1
    check(*par, 1.0, rep, origin=(0.0, 0.0, 0.0))


@pytest.mark.parametrize("rep", REPS)
@pytest.mark.parametrize("cell", CELLS + (0.04,))
def test_cube(cell, rep):
    same(run(*mesh("cube"), cell, rep), want("cube", cell, rep))


@pytest.mark.parametrize("rep", REPS)
@pytest.mark.parametrize("name", ["sphere", "sphere_faces_shuffled", "sphere_vertices_shuffled"])
def test_sphere_and_its_shuffles(name, rep):
    ref = want(name, 0.1, rep)
    assert ref[3]["faces"] > 2000
    same(run(*mesh(name), 0.1, rep), ref)


@pytest.mark.parametrize("rep", REPS)
def test_one_cluster_only(rep):
    """every vertex in one cell: one cluster, every face collapses, and the corner records are sorted over ZERO key bits"""
    ref = want("cube", 4.0, rep)
    assert ref[3]["clusters"] == 1 and ref[3]["faces"] == 0 and ref[3]["collapsed_faces"] == 6912
    same(run(*mesh("cube"), 4.0, rep), ref)
    v, f = R.edge_triangle(0.75)
    check(v * [1.0, 0.1, 1.0], f, 1.0, rep, origin=(0.0, 0.0, 0.0))


@pytest.mark.parametrize("rep", REPS)
def test_one_cell_of_70000_vertices(rep):
    """a run longer than any workgroup, sums of thousands of terms in one lane's order"""
    ref = want("crowd", 2.0, rep, (0.0, 0.0, 0.0))
    assert ref[3]["clusters"] == 4 and ref[3]["faces"] == 4 and ref[3]["collapsed_faces"] == 23334 and ref[3]["duplicate_faces"] == 0
    same(run(*mesh("crowd"), 2.0, rep, origin=(0.0, 0.0, 0.0)), ref)


@pytest.mark.parametrize("rep", REPS)
def test_keys_that_differ_in_the_top_and_in_the_lowest_bit(rep):
    cells = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (2 ** 20, 0, 0), (2 ** 20, 0, 1), (2 ** 21 - 1, 0, 0), (2 ** 21 - 1, 2 ** 21 - 1, 2 ** 21 - 1),
             (2 ** 21 - 1, 2 ** 21 - 1, 2 ** 21 - 2), (0, 2 ** 21 - 1, 0), (0, 0, 2 ** 21 - 1), (2 ** 20, 2 ** 20, 2 ** 20)]
    g = np.random.default_rng(11)
    v = np.array(cells, np.float64) + 0.25 + 0.5 * g.random((len(cells), 3))
    f = np.array([g.permutation(len(cells))[:3] for _ in range(24)])
    ref = check(v, f, 1.0, rep, origin=(0.0, 0.0, 0.0))
    assert ref[3]["clusters"] == len(cells) and ref[3]["collapsed_faces"] == 0
    v2 = np.concatenate((v, v + 0.125))                       # two members per cell
    check(v2, np.concatenate((f, f + len(v))), 1.0, rep, origin=(0.0, 0.0, 0.0))


@pytest.mark.parametrize("rep", REPS)
def test_edge_sizes(rep):
    no_v, no_f = np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    v, f = R.edge_triangle(2.5)
    for a, b in ((no_v, no_f), (v, no_f), (no_v, f[:0])):
        check(a, b, 1.0, rep)
    ref = check(v, f, 1.0, rep)                               # one triangle
    assert ref[3]["vertices"] == 3 and ref[3]["faces"] == 1
    check(np.full((3, 3), np.nan), f, 1.0, rep)               # no face is kept: no cluster
    check(np.full((3, 3), np.inf), f, 1.0, rep)


@pytest.mark.parametrize("rep", REPS)
def test_float32_vertices_and_int32_faces(rep):
    v, f = mesh("sphere")
    v32 = v.astype(np.float32)
    ref = R.simplify(v32.astype(np.float64), f, 0.1, representative=rep)
    same(run(cu(v32), cu(f, torch.int32), 0.1, rep), ref)


@pytest.mark.parametrize("rep", REPS)
def test_random_soups(rep):
    """200 soups of at most 64 faces over at most 40 vertices whose coordinates repeat (a lattice of quarters, exact copies),
    with NaN and Inf among them, at cells from below the spacing to above the whole soup"""
    g = np.random.default_rng(2024)
    for i in range(200):
        V, F = int(g.integers(3, 41)), int(g.integers(1, 65))
        v = g.integers(-8, 9, (V, 3)) * 0.25
        if i % 3 == 0:
            v = v + g.random((V, 3)) * 0.1
        if i % 4 == 1:
            v[g.integers(0, V, 3)] = v[g.integers(0, V, 3)]           # exact copies of other vertices
        if i % 5 == 2:
            v[g.integers(0, V), g.integers(0, 3)] = [np.nan, np.inf, -np.inf][i % 3]
        if i % 7 == 3:
            v[g.integers(0, V), g.integers(0, 3)] = -0.0
        f = g.integers(0, V, (F, 3))
        cell = [0.2, 0.25, 0.5, 0.77, 1.0, 2.5, 9.0][i % 7]
        origin = None if i % 2 else (-2.5, -2.25, -2.0)
        check(v, f, cell, rep, origin=origin, rank_tol=[1e-3, 1e-6, 0.5][i % 3])


def test_repeated_runs_are_bit_identical():
    v, f = cu(mesh("sphere")[0]), cu(mesh("sphere")[1])
    for rep in REPS:
        first = run(v, f, 0.1, rep)
        same(first, want("sphere", 0.1, rep))
        for _ in range(9):
            again = run(v, f, 0.1, rep)
            assert torch.equal(again[0].view(torch.int64), first[0].view(torch.int64)) and torch.equal(again[1], first[1])
            assert torch.equal(again[2], first[2]) and again[3] == first[3]


@pytest.mark.parametrize("rep", REPS)
def test_raw_abi_writes_stop_at_the_counts(rep):
    """the C ABI as it is: outputs of the input's size and TAIL rows more, filled with a sentinel; nothing behind the counts (the map:
    behind V) is written, everything before them is"""
    from surfd_amd import _native as N
    from surfd_amd.meshsimplify import REPRESENTATIVES
    TAIL = 64
    v, f = mesh("sphere")
    wv, wf, wm, wc = want("sphere", 0.1, rep)
    dv, df = cu(v), cu(f, torch.int32)
    ov = torch.full((len(v) + TAIL, 3), -7.5e300, dtype=torch.float64, device="cuda")
    of = torch.full((len(f) + TAIL, 3), -77, dtype=torch.int32, device="cuda")
    om = torch.full((len(v) + TAIL,), -77, dtype=torch.int32, device="cuda")
    counts = (C.c_int64 * 8)(*([-5] * 8))
    N.check(N.lib().surfd_meshsimplify_cluster(N.ptr(dv), len(v), N.ptr(df), len(f), None, 0.1, REPRESENTATIVES[rep], 1e-3, N.ptr(ov), N.ptr(of), N.ptr(om),
                                               counts, N.stream()))
    torch.cuda.synchronize()
    assert list(counts) == [wc[k] for k in R.COUNT_NAMES] + [-5, -5]
    nv, nf = wc["vertices"], wc["faces"]
    assert bool((ov[nv:] == -7.5e300).all()) and bool((of[nf:] == -77).all()) and bool((om[len(v):] == -77).all())
    assert np.array_equal(ov[:nv].cpu().numpy().view(np.int64), wv.view(np.int64))
    assert np.array_equal(of[:nf].cpu().numpy(), wf) and np.array_equal(om[:len(v)].cpu().numpy(), wm)
    # without a map
    ov2 = torch.full_like(ov, -7.5e300)
    N.check(N.lib().surfd_meshsimplify_cluster(N.ptr(dv), len(v), N.ptr(df), len(f), None, 0.1, REPRESENTATIVES[rep], 1e-3, N.ptr(ov2), N.ptr(of), None,
                                               counts, N.stream()))
    assert torch.equal(ov2.view(torch.int64), ov.view(torch.int64))
    # refusals of the host side: nothing is launched
    lib = N.lib()
    for cell, tol, which in ((0.0, 1e-3, 0), (-1.0, 1e-3, 0), (float("nan"), 1e-3, 0), (float("inf"), 1e-3, 0), (0.1, 0.0, 0), (0.1, float("nan"), 1), (0.1, 1e-3, 2)):
        assert lib.surfd_meshsimplify_cluster(N.ptr(dv), len(v), N.ptr(df), len(f), None, cell, which, tol, N.ptr(ov), N.ptr(of), None, counts, N.stream()) == -1
    assert lib.surfd_meshsimplify_cluster(N.ptr(dv), len(v), N.ptr(df), 2 ** 30, None, 0.1, 0, 1e-3, N.ptr(ov), N.ptr(of), None, counts, N.stream()) == -4
    bad_origin = (C.c_double * 3)(0.0, float("nan"), 0.0)
    assert lib.surfd_meshsimplify_cluster(N.ptr(dv), len(v), N.ptr(df), len(f), bad_origin, 0.1, 0, 1e-3, N.ptr(ov), N.ptr(of), None, counts, N.stream()) == -1


def test_refusals_come_back_as_errors_and_the_stream_goes_on():
    from surfd_amd.meshsimplify import simplify_vertex_clustering as simplify
    v, f = R.hand_mesh()
    dv, df = cu(v), cu(f)
    for rep in REPS:
        for bad_index in (len(v), -1, 2 ** 31 - 1):
            bad = f.copy(); bad[2, 1] = bad_index
            with pytest.raises(RuntimeError, match=r"libsurfd_hip error -1:.*outside \[0, 11\)"):
                simplify(dv, cu(bad), 1.0, representative=rep)
            with pytest.raises(RuntimeError, match=r"libsurfd_hip error -1:.*outside \[0, 11\)"):
                simplify(dv, cu(bad), cells=4, representative=rep)
            same(run(dv, df, 1.0, rep), R.simplify(v, f, 1.0, representative=rep))
        for tri, origin in ((R.edge_triangle(2.0 ** 21 + 0.5), (0.0, 0.0, 0.0)), (R.edge_triangle(2.5), (1.0, 0.0, 0.0)), (R.edge_triangle(1e300), (-1e300, 0.0, 0.0))):
            with pytest.raises(RuntimeError, match=r"libsurfd_hip error -1:.*2\^21"):
                simplify(cu(tri[0]), cu(tri[1]), 1.0, origin=origin, representative=rep)
            same(run(dv, df, 1.0, rep), R.simplify(v, f, 1.0, representative=rep))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        simplify(torch.from_numpy(v), torch.from_numpy(f), 1.0)
    for kw in (dict(), dict(cell=1.0, cells=4), dict(cell=0.0), dict(cell=-1.0), dict(cells=0), dict(cells=2 ** 21), dict(cell=1.0, representative="median"),
               dict(cell=1.0, rank_tol=0.0), dict(cell=1.0, origin=(0.0, 0.0)), dict(cell=1.0, origin=(0.0, float("inf"), 0.0))):
        with pytest.raises(ValueError):
            simplify(dv, df, **kw)
    with pytest.raises(ValueError):
        simplify(dv[:, :2], df, 1.0)
    with pytest.raises(TypeError):
        simplify(dv.half(), df, 1.0)
    with pytest.raises(TypeError):
        simplify(dv, df.float(), 1.0)


@pytest.mark.parametrize("rep", REPS)
def test_cells_divides_the_largest_extent_of_the_referenced_vertices(rep):
    from surfd_amd.meshsimplify import simplify_vertex_clustering as simplify
    v, f = R.hand_mesh()                                      # referenced: x in [0.25, 2.75], y and z in [0.25, 1.5]; the NaN and the stray vertices do not count
    cell = float(torch.tensor(2.75, dtype=torch.float64) - torch.tensor(0.25, dtype=torch.float64)) / 5
    got = simplify(cu(v), cu(f), cells=5, representative=rep, return_map=True, return_stats=True)
    same(got, R.simplify(v, f, cell, representative=rep))
    sv, sf = mesh("sphere")
    got = simplify(cu(sv), cu(sf), cells=20, representative=rep, return_map=True, return_stats=True)
    same(got, want("sphere", 0.1, rep))                      # extent 2, 20 cells
    out = simplify(cu(sv), cu(sf), cells=20, representative=rep)
    assert len(out) == 2 and torch.equal(out[0], got[0]) and torch.equal(out[1], got[1])


class ShellField:
    """the analytic field of mcubes.bench_e2: a sphere shell above z = 0, a rim below"""

    def __call__(self, c):
        x, y, z = c[:, 0], c[:, 1], c[:, 2]
        up = (torch.sqrt(x * x + y * y + z * z) - 0.6).abs()
        rho = torch.sqrt(x * x + y * y) - 0.6
        return torch.clamp(torch.where(z >= 0, up, torch.sqrt(rho * rho + z * z)), max=0.1)


def test_watertight_mesh_on_the_device_then_simplified():
    """the 64^3 shell of get_watertight_mesh(device=True, min_faces=...) goes through simplify_vertex_clustering(cells=K) where it
    lies, as examples/generate.py --watertight --device_mc --simplify_cells K does"""
    from surfd_amd.meshsimplify import simplify_vertex_clustering as simplify
    from surfd_amd.meshudf import get_watertight_mesh
    v, f = get_watertight_mesh(ShellField(), 64, device=True, min_faces=50)
    for rep in REPS:
        sv, sf, sm, st = simplify(v, f, cells=16, representative=rep, return_map=True, return_stats=True)
        assert 0 < len(sf) < len(f) // 4 and sv.is_cuda and sv.dtype == torch.float64 and sf.dtype == torch.int64
        cell = float((v.max(dim=0).values - v.min(dim=0).values).max()) / 16
        same((sv, sf, sm, st), R.simplify(v.cpu().numpy(), f.cpu().numpy(), cell, representative=rep))


def test_get_mesh_from_udf_simplify_cells():
    """the decoder, latent seed and arguments of test_get_mesh_from_udf_device_clean_is_bit_identical (tests/test_gpu_meshclean.py)"""
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
    with pytest.raises(ValueError, match="simplify_cells.*differentiable"):
        get_mesh_from_udf(field, device_clean=True, simplify_cells=16, **kw)
    with pytest.raises(ValueError, match="simplify_cells.*device_clean"):
        get_mesh_from_udf(field, differentiable=False, simplify_cells=16, **kw)
    v0, t0 = get_mesh_from_udf(field, differentiable=False, device_clean=True, **kw)
    v1, t1 = get_mesh_from_udf(field, differentiable=False, device_clean=True, simplify_cells=16, **kw)
    assert 0 < len(t1) < len(t0) and len(v1) < len(v0) and v1.dtype == torch.float32 and t1.dtype == torch.int64 and v1.is_cuda
    assert int(t1.max()) == len(v1) - 1 and bool(torch.isfinite(v1).all())
    # without the border smoothing the vertices are the simplification's own, rounded to fp32: inside the box of the unsimplified mesh
    v2, t2 = get_mesh_from_udf(field, differentiable=False, smooth_borders=False, device_clean=True, simplify_cells=16, **kw)
    v3, _ = get_mesh_from_udf(field, differentiable=False, smooth_borders=False, device_clean=True, **kw)
    assert torch.equal(t1, t2)
    lo, hi = v3.min(dim=0).values, v3.max(dim=0).values
    cell = float((hi - lo).max()) / 16
    assert bool((v2 >= lo - cell).all()) and bool((v2 <= hi + cell).all())
