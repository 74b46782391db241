"""The device decimation (surfd_amd/meshsimplify.py: simplify_quadric_decimation, csrc/meshdecimate.hip) against
tests/meshdecimate_ref.py, bit for bit and in the same order: vertices as int64 views, faces, the map and every count.  The meshes of
the CPU tests, sheets whose edges, vertices and faces cross the 64- and 256-lane boundaries, runs longer than a wave, the knobs,
intermediate states, edge targets and sizes, input variants, 100 random soups, repeated runs, the C ABI with sentinels behind its
outputs, the refusals and the consumers."""
import ctypes as C
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshdecimate_ref as R  # noqa: E402
import meshsimplify_ref as MS  # noqa: E402
import meshtopo_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cu(x, dtype=None):
    t = torch.from_numpy(np.array(x))                         # a copy: the shared references are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


@functools.lru_cache(maxsize=None)
def mesh(name):
    rules = R.rule_meshes()
    if name in rules:
        v, f = rules[name][:2]
    elif name == "sheet17_flat":
        v, f = R.sheet_mesh(17, 17)
    elif name == "sheet17":
        v, f = R.sheet_mesh(17, 17, bump=0.3)
    elif name == "sheet40":                                     # 3 200 faces, 1 681 vertices, 4 880 edges
        v, f = R.sheet_mesh(40, 40, bump=0.3)
    elif name == "sheet2x130":                                  # rows of 131 vertices: runs longer than a wave along one axis
        v, f = R.sheet_mesh(2, 130, bump=0.3)
    elif name == "cube24":
        v, f = MS.cube_mesh(24)
    elif name == "sphere":
        v, f = MS.sphere_mesh()
    elif name == "icosphere":
        v, f = R.icosphere(3)
    elif name == "triangle":
        v, f = np.eye(3), np.array([[0, 1, 2]])
    else:
        v, f = getattr(R, name if name in ("tetrahedron", "octahedron", "cube12", "two_spheres") else name + "_mesh")()
    v, f = np.ascontiguousarray(v, np.float64), np.ascontiguousarray(f, np.int64)
    v.setflags(write=False); f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def want(name, target, **kw):
    """the restatement on a named mesh, worked out once and shared (callers do not write to it)"""
    out = R.decimate(*mesh(name), target, **kw)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def as_counts(stats):
    from surfd_amd.meshsimplify import DECIMATE_STOPS
    return dict(stats, stop=DECIMATE_STOPS.index(stats["stop"]))


def same(got, ref):
    gv, gf, gm, gs = got
    wv, wf, wm, wc = ref
    assert gv.is_cuda and gf.is_cuda and gm.is_cuda and gv.dtype == torch.float64 and gf.dtype == torch.int64 and gm.dtype == torch.int64
    assert as_counts(gs) == wc, (gs, wc)
    assert tuple(gv.shape) == wv.shape and tuple(gf.shape) == wf.shape and tuple(gm.shape) == wm.shape
    assert np.array_equal(gm.cpu().numpy(), wm), f"{int((gm.cpu().numpy() != wm).sum())} map entries differ"
    assert np.array_equal(gf.cpu().numpy(), wf), f"{int((gf.cpu().numpy() != wf).any(axis=1).sum())} faces differ"
    a, b = gv.cpu().numpy().view(np.int64), np.ascontiguousarray(wv).view(np.int64)
    assert np.array_equal(a, b), f"{int((a != b).sum())} of {a.size} doubles differ"


def run(v, f, target, **kw):
    from surfd_amd.meshsimplify import simplify_quadric_decimation
    return simplify_quadric_decimation(v if isinstance(v, torch.Tensor) else cu(v), f if isinstance(f, torch.Tensor) else cu(f), target,
                                       return_map=True, return_stats=True, **kw)


CASES = [("tetrahedron", 2), ("octahedron", 4), ("octahedron", 6), ("cube12", 6), ("two_spheres", 40), ("icosphere", 128), ("sheet17", 144),
         ("sheet17_flat", 144), ("torus", 144), ("cube24", 691), ("sphere", 2816), ("sheet40", 400), ("sheet2x130", 130), ("triangle", 0),
         ("refused_valence", 0), ("refused_link", 0), ("refused_border", 0), ("refused_flip", 0)]


@pytest.mark.parametrize("name,target", CASES)
def test_device_equals_the_restatement(name, target):
    same(run(*mesh(name), target), want(name, target))


@pytest.mark.parametrize("kw", [dict(spread=1), dict(spread=16), dict(max_rounds=1), dict(max_rounds=2), dict(seed=7), dict(seed=2 ** 64 - 1),
                                dict(flip_cos=0.0), dict(flip_cos=0.9), dict(border_weight=0.0), dict(rank_tol=0.5)], ids=str)
def test_knobs_and_intermediate_states(kw):
    for name, target in (("sheet40", 400), ("icosphere", 128)):
        same(run(*mesh(name), target, **kw), want(name, target, **kw))


@pytest.mark.parametrize("name", ["sheet17", "torus", "octahedron"])
def test_edge_targets(name):
    v, f = mesh(name)
    for target in (0, 1, len(f) - 1, len(f), len(f) + 5):
        same(run(v, f, target), want(name, target))
    got = run(v, f, None, ratio=0.25)
    same(got, want(name, int(len(f) * 0.25)))
    out = run(v, f, len(f))
    assert torch.equal(out[0].view(torch.int64), cu(v).view(torch.int64)) and torch.equal(out[1], cu(f))


def test_empty_and_degenerate_inputs():
    nan, inf = float("nan"), float("inf")
    v, f = mesh("octahedron")
    for vv, ff in ((np.zeros((0, 3)), np.zeros((0, 3), np.int64)), (v, np.zeros((0, 3), np.int64)), (np.full((4, 3), nan), np.array([[0, 1, 2], [1, 2, 3]])),
                   (np.array([[0, 0, 0], [inf, 0, 0], [0, 1, 0.]]), np.array([[0, 1, 2]])), (np.eye(3), np.array([[0, 1, 1], [2, 2, 2]]))):
        for target in (0, 5):
            same(run(vv, ff, target), R.decimate(vv, ff, target))
    # a NaN vertex, an unreferenced vertex, a face that names a vertex twice, -0.0
    v2 = np.concatenate((v, [[nan, 0, 0], [9.0, 9, 9], [0.5, -0.0, 0.5]]))
    f2 = np.concatenate(([[0, 6, 2]], f[:4], [[8, 8, 1], [3, 8, 3]], f[4:]))
    for target in (4, 100):
        same(run(v2, f2, target), R.decimate(v2, f2, target))


def test_float32_and_int32_input():
    v, f = mesh("sheet17")
    v32 = v.astype(np.float32)
    ref = R.decimate(v32.astype(np.float64), f, 144)
    same(run(cu(v32), cu(f, torch.int32), 144), ref)
    same(run(cu(v32), cu(f), 144), ref)
    out = run(cu(v), cu(f, torch.int32), 144)
    same(out, want("sheet17", 144))
    from surfd_amd.meshsimplify import simplify_quadric_decimation
    two = simplify_quadric_decimation(cu(v), cu(f), 144)
    assert len(two) == 2 and torch.equal(two[0], out[0]) and torch.equal(two[1], out[1])


def soup(seed):
    g = np.random.default_rng(seed)
    V, F = int(g.integers(3, 25)), int(g.integers(1, 61))
    v = g.integers(-3, 4, size=(V, 3)).astype(np.float64) if seed % 3 == 0 else g.normal(size=(V, 3))
    f = g.integers(0, V, size=(F, 3))                           # repeated indices happen by themselves
    if F > 4:
        f[g.integers(0, F)] = f[g.integers(0, F)]               # a duplicate face
        f[g.integers(0, F)] = f[g.integers(0, F)][::-1]         # and one turned over
    for value in (float("nan"), float("inf"), -0.0):
        if g.random() < 0.4:
            v[g.integers(0, V), g.integers(0, 3)] = value
    return v, f


@pytest.mark.parametrize("block", range(4))
def test_random_soups_are_equal_and_clean(block):
    """non-manifold input: nothing is promised of its shape, but the device equals the restatement and the output is clean"""
    for seed in range(25 * block, 25 * block + 25):
        v, f = soup(seed)
        got = run(v, f, int(seed % 7) * len(f) // 8, seed=seed)
        same(got, R.decimate(v, f, int(seed % 7) * len(f) // 8, seed=seed))
        gv, gf = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert np.isfinite(gv).all() and (len(gf) == 0 or (gf.min() >= 0 and gf.max() == len(gv) - 1))
        assert ((gf[:, 0] != gf[:, 1]) & (gf[:, 1] != gf[:, 2]) & (gf[:, 0] != gf[:, 2])).all() and len(np.unique(gf)) == len(gv)


def test_ten_runs_are_identical():
    v, f = mesh("sheet40")
    dv, df = cu(v), cu(f)
    first = run(dv, df, 400)
    for _ in range(9):
        again = run(dv, df, 400)
        assert torch.equal(again[0].view(torch.int64), first[0].view(torch.int64)) and torch.equal(again[1], first[1])
        assert torch.equal(again[2], first[2]) and again[3] == first[3]


def test_raw_abi_writes_stop_at_the_counts():
    """the C ABI as it is: outputs of the input's size and TAIL rows more, filled with a sentinel; nothing behind the counts (the map:
    behind V) is written, everything before them is"""
    from surfd_amd import _native as N
    TAIL = 64
    v, f = mesh("sheet40")
    wv, wf, wm, wc = want("sheet40", 400)
    dv, df = cu(v), cu(f, torch.int32)
    ov = torch.full((len(v) + TAIL, 3), -7.5e300, dtype=torch.float64, device="cuda")
    of = torch.full((len(f) + TAIL, 3), -77, dtype=torch.int32, device="cuda")
    om = torch.full((len(v) + TAIL,), -77, dtype=torch.int32, device="cuda")
    counts = (C.c_int64 * 14)(*([-5] * 14))
    lib = N.lib()

    def call(F=len(f), target=400, bw=1000.0, fc=0.2, tol=1e-3, spread=4, rounds=512, vmap=om):
        return lib.surfd_meshsimplify_decimate(N.ptr(dv), len(v), N.ptr(df), F, target, bw, fc, tol, spread, rounds, 0, N.ptr(ov), N.ptr(of),
                                               N.ptr(vmap) if vmap is not None else None, counts, N.stream())
    N.check(call())
    torch.cuda.synchronize()
    assert list(counts) == [wc[k] for k in R.COUNT_NAMES] + [-5, -5]
    nv, nf = wc["vertices"], wc["faces"]
    assert bool((ov[nv:] == -7.5e300).all()) and bool((of[nf:] == -77).all()) and bool((om[len(v):] == -77).all())
    assert np.array_equal(ov[:nv].cpu().numpy().view(np.int64), wv.view(np.int64))
    assert np.array_equal(of[:nf].cpu().numpy(), wf) and np.array_equal(om[:len(v)].cpu().numpy(), wm)
    keep = ov.clone()
    ov.fill_(-7.5e300)
    N.check(call(vmap=None))                                    # without a map
    assert torch.equal(ov.view(torch.int64), keep.view(torch.int64))
    # refusals of the host side: nothing is launched, nothing allocated
    nan, inf = float("nan"), float("inf")
    for kw in (dict(target=-1), dict(bw=nan), dict(bw=inf), dict(bw=-1.0), dict(fc=nan), dict(fc=1.0), dict(fc=-0.1), dict(tol=0.0), dict(tol=nan),
               dict(tol=inf), dict(spread=0), dict(rounds=0), dict(F=-1)):
        assert call(**kw) == -1, kw
    assert call(F=2 ** 30) == -4                                 # 3 F >= 2^31: by the size arguments alone
    N.check(call())
    assert list(counts)[:12] == [wc[k] for k in R.COUNT_NAMES]


def test_refusals_come_back_as_errors_and_the_stream_goes_on():
    from surfd_amd.meshsimplify import simplify_quadric_decimation as decimate
    v, f = mesh("octahedron")
    dv, df = cu(v), cu(f)
    for bad_index in (len(v), -1, 2 ** 31 - 1):
        bad = f.copy(); bad[5, 1] = bad_index
        with pytest.raises(RuntimeError, match=r"libsurfd_hip error -1:.*outside \[0, 6\)"):
            decimate(dv, cu(bad), 4)
        same(run(dv, df, 4), want("octahedron", 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decimate(torch.from_numpy(np.array(v)), torch.from_numpy(np.array(f)), 4)
    nan = float("nan")
    for kw in (dict(), dict(target_faces=4, ratio=0.5), dict(target_faces=-1), dict(target_faces=2.5), dict(ratio=1.5), dict(ratio=nan),
               dict(target_faces=4, border_weight=nan), dict(target_faces=4, border_weight=-1.0), dict(target_faces=4, flip_cos=1.0),
               dict(target_faces=4, flip_cos=nan), dict(target_faces=4, rank_tol=0.0), dict(target_faces=4, rank_tol=float("inf")),
               dict(target_faces=4, spread=0), dict(target_faces=4, max_rounds=0), dict(target_faces=4, spread=1.5)):
        with pytest.raises(ValueError):
            decimate(dv, df, **kw)
        same(run(dv, df, 4), want("octahedron", 4))
    with pytest.raises(ValueError):
        decimate(dv[:, :2], df, 4)
    with pytest.raises(TypeError):
        decimate(dv.half(), df, 4)
    with pytest.raises(TypeError):
        decimate(dv, df.float(), 4)


class ShellField:
    """the analytic field of mcubes.bench_e2: a sphere shell above z = 0, a rim below"""

    def __call__(self, c):
        x, y, z = c[:, 0], c[:, 1], c[:, 2]
        up = (torch.sqrt(x * x + y * y + z * z) - 0.6).abs()
        rho = torch.sqrt(x * x + y * y) - 0.6
        return torch.clamp(torch.where(z >= 0, up, torch.sqrt(rho * rho + z * z)), max=0.1)


def test_watertight_mesh_on_the_device_then_decimated():
    """the 64^3 shell of get_watertight_mesh(device=True, min_faces=...) goes through simplify_quadric_decimation where it lies, as
    examples/generate.py --watertight --device_mc --simplify_faces N does.  At this resolution the two sheets of the shell are joined
    by some two hundred tunnels (12 496 faces, Euler characteristic -408), and decimation keeps every one: a third of the faces is reached, a tenth is
    not (the call stalls near 2 770 faces, every edge left being refused), and both results are the restatement's, closed as before."""
    from surfd_amd.meshudf import get_watertight_mesh
    v, f = get_watertight_mesh(ShellField(), 64, device=True, min_faces=50)
    before = T.summary(T.build(f.cpu().numpy(), len(v)))
    for N, stop in ((len(f) // 3, "target"), (len(f) // 10, None)):
        got = run(v, f, N)
        same(got, R.decimate(v.cpu().numpy(), f.cpu().numpy(), N))
        after = T.summary(T.build(got[1].cpu().numpy(), len(got[0])))
        print(f"{len(f)} faces -> {len(got[1])} (asked for {N}), {got[3]}")
        assert len(got[1]) < len(f) and (stop is None or (got[3]["stop"] == stop and N - 1 <= len(got[1]) <= N))
        for k in ("closed", "edge_manifold", "components_vertex", "euler_characteristic", "border_loops"):
            assert before[k] == after[k], k


def border_loops(v, f):
    return T.summary(T.build(f.cpu().numpy(), len(v)))["border_loops"]


def test_get_mesh_from_udf_simplify_faces():
    """the decoder, latent seed and arguments of test_get_mesh_from_udf_simplify_cells (tests/test_gpu_meshsimplify.py)"""
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
    with pytest.raises(ValueError, match="simplify_faces.*differentiable"):
        get_mesh_from_udf(field, device_clean=True, simplify_faces=500, **kw)
    with pytest.raises(ValueError, match="simplify_faces.*device_clean"):
        get_mesh_from_udf(field, differentiable=False, simplify_faces=500, **kw)
    with pytest.raises(ValueError, match="simplify_faces and simplify_cells"):
        get_mesh_from_udf(field, differentiable=False, device_clean=True, simplify_faces=500, simplify_cells=16, **kw)
    v0, t0 = get_mesh_from_udf(field, differentiable=False, device_clean=True, **kw)
    N = 8              # the field gives 11 faces in 4 pieces at this resolution, and a piece does not go below one triangle (rule (d))
    v1, t1 = get_mesh_from_udf(field, differentiable=False, device_clean=True, simplify_faces=N, **kw)
    print(f"{len(t0)} faces -> {len(t1)} (asked for {N})")
    assert 0 < len(t1) <= N < len(t0) and len(v1) < len(v0) and v1.dtype == torch.float32 and t1.dtype == torch.int64 and v1.is_cuda
    assert int(t1.max()) == len(v1) - 1 and bool(torch.isfinite(v1).all())
    assert border_loops(v1, t1) == border_loops(v0, t0)


def _obj_faces(path):
    return sum(1 for line in open(path) if line.startswith("f "))


def test_example_flags(tmp_path):
    """--simplify_faces on both drivers, on their smallest settings (in process, as tests/test_gpu_decoder_grid.py runs generate.py): the
    flag is accepted, the run ends and no mesh has more faces than asked for, or than it has without the flag where the call stalls
    (the synthetic checkpoints give empty meshes or crumbs of lone triangles, which decimation leaves alone).  What the flag computes
    is the matter of test_watertight_mesh_on_the_device_then_decimated and test_get_mesh_from_udf_simplify_faces."""
    mods = {}
    for name in ("generate", "reconstruct"):
        spec = importlib.util.spec_from_file_location(name + "_driver", os.path.join(ROOT, "examples", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    base = ["uncond", "--synthetic", "--num_samples", "1", "--resolution", "64", "--respacing", "ddim20"]
    for extra, out in ((["--device_clean"], "gen"), (["--watertight", "--device_mc"], "genw")):
        _, written = mods["generate"].main(base + extra + ["--simplify_faces", "300", "--output_dir", str(tmp_path / out)])
        assert len(written) == 1 and _obj_faces(written[0][0]) <= 300
    faces = {}
    for extra, out in (([], "rec0"), (["--simplify_faces", "300"], "rec")):
        mods["reconstruct"].main(["--synthetic", "--resolution", "64", "--num_points_pcd", "4000", "--output_dir", str(tmp_path / out)] + extra)
        faces[out] = {n: _obj_faces(tmp_path / out / n) for n in sorted(os.listdir(tmp_path / out)) if n.endswith(".obj")}
    print(faces)
    assert faces["rec"] and sorted(faces["rec"]) == sorted(faces["rec0"])
    assert all(faces["rec"][n] <= 300 or faces["rec"][n] < faces["rec0"][n] for n in faces["rec"])
