"""The fast path of csrc/winding.hip on the GPU against the numpy restatement tests/winding_fast_ref.py:
the records bit for bit at every tree shape from one leaf to five levels, values within max(T, 1) 2^-50 and equal term counts
through the raw ABI and through WindingScene, bit identity of a query's value across batches, positions and repeats, beta = +inf
against the exact GPU path, special queries, refusals, a mesh with a vertex beyond 2^20, occupancy and voxel grids against the
exact path's, and the two drivers."""
import functools
import os
import sys

import ctypes as C
import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raycast_ref as rr  # noqa: E402
import winding_fast_ref as wf  # noqa: E402
import winding_ref as wr  # noqa: E402
import mesh_udf_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_FS = (1, 3, 4, 5, 16, 17, 64, 65, 257, 1025)     # one leaf, a partial leaf, one level, a partial node, two to five levels
QS = (1, 63, 64, 65, 257)                             # each side of a wave and of a workgroup
BETAS = (1.0, 2.0, 3.0, float("inf"))
COUNT_VISITS = 2
ERR_ARG, ERR_STATE = -1, -2


def cu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


class RawWinding:
    """the C ABI as it is"""

    def __init__(self, v, f, build=True):
        from surfd_amd import _native as N
        self.N = N
        self.v, self.f = cu(v), cu(f, torch.int32)
        self.h = C.c_void_p()
        N.check(N.lib().surfd_winding_create(N.ptr(self.v), len(v), N.ptr(self.f), len(f), N.stream(), C.byref(self.h)))
        if build:
            N.check(N.lib().surfd_winding_build_bvh(self.h, N.stream()))
            N.check(N.lib().surfd_winding_build_bvh(self.h, N.stream()))                     # idempotent

    def fast_rc(self, p, Q, beta, flags, w):
        N = self.N
        return N.lib().surfd_winding_eval_fast(self.h, N.ptr(p), Q, beta, flags, N.ptr(w), N.stream())

    def fast(self, points, beta):
        """-> (w, cluster terms, triangle terms of the call)"""
        N, Q = self.N, len(points)
        p = cu(np.asarray(points, dtype=np.float32))
        w = torch.full((Q,), -7.0, device="cuda", dtype=torch.float64)
        N.check(self.fast_rc(p, Q, beta, COUNT_VISITS, w))
        a, b = C.c_int64(-1), C.c_int64(-1)
        N.check(N.lib().surfd_winding_visits(self.h, C.byref(a), C.byref(b), N.stream()))
        return w.cpu().numpy(), a.value, b.value

    def exact(self, points):
        N, Q = self.N, len(points)
        p = cu(np.asarray(points, dtype=np.float32))
        w = torch.empty(Q, device="cuda", dtype=torch.float64)
        N.check(N.lib().surfd_winding_eval(self.h, N.ptr(p), Q, 0, N.ptr(w), N.stream()))
        return w.cpu().numpy()

    def __del__(self):
        self.N.lib().surfd_winding_destroy(self.h)


# ---- the cases: meshes, queries, and reference values computed once ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def holed():
    return wr.holed_sphere()


@functools.lru_cache(maxsize=None)
def big_torus():
    v, f = rr.torus(132, 64)
    assert len(f) == 16896
    return v, f


def uniform_queries(n, seed=1):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "holed_sphere":
        return holed()[:2]
    if name == "big_torus":
        return big_torus()
    return rr.MESHES[name]()


MESH_NAMES = sorted(rr.MESHES) + ["holed_sphere"]


@functools.lru_cache(maxsize=None)
def tree(name):
    return wf.build(*mesh(name))


@functools.lru_cache(maxsize=None)
def reference(name, beta, n=300):
    out = wf.walk(tree(name), uniform_queries(n), beta)
    for x in out:
        x.setflags(write=False)
    return out


def close(got, ref, terms, what):
    bound = wf.tolerance(terms)
    err = np.abs(got - ref)
    print(f"{what}: Q = {len(ref)}, max |w - w_ref| = {err.max():.3e}, smallest bound {bound.min():.3e}, most terms {int(terms.max())}")
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert (err <= bound).all(), (what, float((err - bound).max()))


# ---- 1. the tree and its records ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", TREE_FS + (16896,))
def test_records_equal_the_restatement(F):
    from surfd_amd.winding import WindingScene
    v, f = rr.first_faces(big_torus(), F)
    want = wf.build(v, f)
    scene = WindingScene(cu(v), cu(f), accel="bvh")
    got = scene.read_bvh()
    assert got["level_sizes"] == want["lay"]["size"] and got["perm"] is None
    assert np.array_equal(got["leaves"].cpu().numpy(), want["leaves"])
    assert np.array_equal(got["boxes"].cpu().numpy(), want["boxes"])
    rec = got["records"]
    assert rec.dtype == torch.float64 and tuple(rec.shape) == (want["lay"]["nodes"], 4, 7)
    assert np.array_equal(rec.cpu().numpy(), want["records"])
    lazy = WindingScene(cu(v), cu(f))                                    # built on demand, once
    assert torch.equal(lazy.read_bvh()["records"], rec) and lazy.accel == "exact"
    # the exact path does not notice the hierarchy
    q = cu(uniform_queries(65, 40 + F))
    assert torch.equal(scene.winding_number(q, accel="exact"), WindingScene(cu(v), cu(f)).winding_number(q))


# ---- 2. values and term counts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("name", MESH_NAMES)
def test_values_and_term_counts_against_the_restatement(name, beta):
    from surfd_amd.winding import WindingScene
    v, f = mesh(name)
    q = uniform_queries(300)
    ref, ncl, ntri = reference(name, beta)
    raw = RawWinding(v, f)
    scene = WindingScene(cu(v), cu(f), accel="bvh", beta=beta)
    for Q in QS + (300,):
        w, a, b = raw.fast(q[:Q], beta)
        close(w, ref[:Q], (ncl + ntri)[:Q], f"{name} beta-{beta} Q-{Q} raw")
        assert (a, b) == (int(ncl[:Q].sum()), int(ntri[:Q].sum())), (name, beta, Q)
        ws = scene.winding_number(cu(q[:Q]), count_visits=True)
        assert ws.dtype == torch.float64 and ws.is_cuda
        assert np.array_equal(ws.cpu().numpy().view(np.uint64), w.view(np.uint64))
        assert scene.last_visits == (a, b)
    if beta == float("inf"):
        assert not ncl.any() and (ntri == len(f)).all()


@pytest.mark.parametrize("F", TREE_FS + (16896,))
def test_values_at_every_tree_shape(F):
    from surfd_amd.winding import WindingScene, winding_number
    v, f = rr.first_faces(big_torus(), F)
    q = uniform_queries(257, 200 + F)
    t = wf.build(v, f)
    scene = WindingScene(cu(v), cu(f))
    for beta in (1.0, 2.0, 3.0):
        ref, ncl, ntri = wf.walk(t, q, beta)
        w = scene.winding_number(cu(q), accel="bvh", beta=beta, count_visits=True)
        close(w.cpu().numpy(), ref, ncl + ntri, f"F-{F} beta-{beta}")
        assert scene.last_visits == (int(ncl.sum()), int(ntri.sum()))
        if beta == 2.0:
            assert torch.equal(winding_number(cu(v), cu(f, torch.int32), cu(q), accel="bvh"), w)
    assert scene.last_visits[0] > 0 or F <= 5


# ---- 3. bit identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [2.0, float("inf")])
def test_bits_do_not_depend_on_batch_position_or_repeat(beta):
    from surfd_amd.winding import WindingScene
    v, f = big_torus() if beta == 2.0 else mesh("torus")
    scene = WindingScene(cu(v), cu(f), accel="bvh", beta=beta)
    qd = cu(uniform_queries(300, 300))
    among = scene.winding_number(qd)
    again = scene.winding_number(qd)
    alone = scene.winding_number(qd[:5].contiguous())
    rev = scene.winding_number(qd.flip(0).contiguous()).flip(0)
    assert among.dtype == torch.float64
    assert torch.equal(among, again)
    assert torch.equal(alone, among[:5])
    assert torch.equal(rev, among)
    one_by_one = torch.cat([scene.winding_number(qd[i:i + 1].contiguous()) for i in (0, 7, 299)])
    assert torch.equal(one_by_one, among[[0, 7, 299]])
    assert torch.equal(WindingScene(cu(v), cu(f)).winding_number(qd, accel="bvh", beta=beta), among)


# ---- 4. beta = +inf is the exact sum in another order ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "wavy_sheet", "holed_sphere", "big_torus"])
def test_beta_inf_against_the_exact_gpu_path(name):
    v, f = mesh(name)
    q = uniform_queries(64 if name == "big_torus" else 300, 9)
    raw = RawWinding(v, f)
    w, a, b = raw.fast(q, float("inf"))
    assert (a, b) == (0, len(q) * len(f))
    err = float(np.abs(w - raw.exact(q)).max())
    print(f"{name}: F = {len(f)}, max |w_inf - w_exact| = {err:.3e}, bound {wr.tolerance(len(f)):.3e}")
    assert err <= wr.tolerance(len(f))


# ---- 5. special queries and refusals -----------------------------------------------------------------------------------------------
def test_non_finite_queries_give_nan_and_no_terms():
    from surfd_amd.winding import WindingScene
    v, f = rr.octahedron()
    q = np.array([(0.1, 0.1, 0.1), (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (2, 2, 2), (0.1, 0.1, 0.1)], dtype=np.float32)
    ref, ncl, ntri = wf.walk(wf.build(v, f), q, 2.0)
    w, a, b = RawWinding(v, f).fast(q, 2.0)
    assert np.isnan(w[1:4]).all() and np.isnan(ref[1:4]).all() and not ncl[1:4].any() and not ntri[1:4].any()
    ok = [0, 4, 5]
    close(w[ok], ref[ok], (ncl + ntri)[ok], "octahedron")
    assert (a, b) == (int(ncl.sum()), int(ntri.sum())) and w[0].view(np.uint64) == w[5].view(np.uint64)
    scene = WindingScene(cu(v), cu(f), accel="bvh")
    assert scene.compute_occupancy(cu(q)).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    assert torch.signbit(scene.compute_signed_distance(cu(q)[[0, 4]].contiguous())).tolist() == [True, False]
    empty = scene.winding_number(torch.zeros(0, 3, device="cuda"), count_visits=True)
    assert empty.shape == (0,) and empty.dtype == torch.float64 and scene.last_visits == (0, 0)


def test_refusals():
    from surfd_amd import _native as N
    from surfd_amd.winding import WindingScene
    v, f = rr.cube()
    p = cu(uniform_queries(4))
    w = torch.zeros(4, device="cuda", dtype=torch.float64)
    a, b = C.c_int64(), C.c_int64()
    cold = RawWinding(v, f, build=False)
    assert cold.fast_rc(p, 4, 2.0, 0, w) == ERR_STATE and b"surfd_winding_build_bvh" in N.lib().surfd_last_error()
    assert N.lib().surfd_winding_visits(cold.h, C.byref(a), C.byref(b), N.stream()) == ERR_STATE
    assert N.lib().surfd_winding_bvh_info(cold.h, None, None, None, None, 0) == ERR_STATE
    assert N.lib().surfd_winding_bvh_read(cold.h, None, None, None, N.stream()) == ERR_STATE
    raw = RawWinding(v, f)
    for bad in (0.999, 0.0, -2.0, float("nan"), float("-inf")):
        assert raw.fast_rc(p, 4, bad, 0, w) == ERR_ARG and b"beta" in N.lib().surfd_last_error()
    assert raw.fast_rc(p, 4, 2.0, 1, w) == ERR_ARG                       # SURFD_WINDING_ONE_SPLIT belongs to the exact path
    assert raw.fast_rc(p, 4, 2.0, 4, w) == ERR_ARG
    assert raw.fast_rc(p, -1, 2.0, 0, w) == ERR_ARG
    assert raw.fast_rc(p, 2 ** 31, 2.0, 0, w) == ERR_ARG
    assert raw.fast_rc(None, 4, 2.0, 0, w) == ERR_ARG
    assert raw.fast_rc(p, 4, 2.0, 0, None) == ERR_ARG
    assert raw.fast_rc(None, 0, 2.0, 0, None) == 0                       # Q = 0 is a no-op
    torch.cuda.synchronize()
    assert not w.any()
    scene = WindingScene(cu(v), cu(f), accel="bvh")
    with pytest.raises(ValueError, match="beta"):
        scene.winding_number(p, beta=0.5)
    with pytest.raises(ValueError, match="accel"):
        scene.winding_number(p, accel="tiles")
    with pytest.raises(ValueError, match="one_split"):
        scene.winding_number(p, one_split=True)
    with pytest.raises(ValueError, match="count_visits"):
        scene.winding_number(p, accel="exact", count_visits=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene.winding_number(torch.zeros(3, 3))


def test_a_vertex_beyond_2_to_20_is_never_approximated_across():
    v, f = rr.icosphere(2)
    v = v.copy()
    v[0] = (2.0 ** 21, 3.0, -5.0)
    t = wf.build(v, f)
    assert np.isinf(t["records"][..., 6]).any()
    q = np.concatenate([uniform_queries(200, 12), uniform_queries(57, 13) * np.float32(4e6)])
    raw = RawWinding(v, f)
    assert np.array_equal(read_records(raw, t), t["records"])
    for beta in (1.0, 2.0):
        ref, ncl, ntri = wf.walk(t, q, beta)
        w, a, b = raw.fast(q, beta)
        close(w, ref, ncl + ntri, f"far vertex beta-{beta}")
        assert (a, b) == (int(ncl.sum()), int(ntri.sum()))
        far = sum(int((t["leaves"][i] >= 0).sum()) for i in range(t["lay"]["nleaf"]) if np.isinf(t["records"][i // 4, i % 4, 6]))
        assert far > 0 and (ntri >= far).all()                           # those leaves are entered by every query


def read_records(raw, t):
    """surfd_winding_bvh_info / _bvh_read through the raw ABI, to host memory"""
    N = raw.N
    levels, leaves, nodes = C.c_int(), C.c_int(), C.c_int()
    sizes = (C.c_int32 * 16)()
    N.check(N.lib().surfd_winding_bvh_info(raw.h, C.byref(levels), C.byref(leaves), C.byref(nodes), sizes, 16))
    assert [int(sizes[k]) for k in range(levels.value)] == t["lay"]["size"] and leaves.value == t["lay"]["nleaf"]
    rec = np.full((nodes.value, 4, 7), 9.0)
    N.check(N.lib().surfd_winding_bvh_read(raw.h, None, None, rec.ctypes.data, N.stream()))
    return rec


# ---- 6. occupancy and voxel grids against the exact path's -------------------------------------------------------------------------
def test_occupancy_and_voxel_grid_equal_the_exact_path_on_the_holed_sphere():
    from surfd_amd import meshprep, voxelize
    from surfd_amd.winding import WindingScene
    v, f, holes = holed()
    vd, fd = cu(v), cu(f)
    q, kept, inside = wr.holed_sphere_queries(holes)
    qd = cu(q[kept])
    exact, fast = WindingScene(vd, fd), WindingScene(vd, fd, accel="bvh")
    assert np.array_equal(exact.compute_occupancy(qd).cpu().numpy() > 0, inside[kept])
    occ, w = fast.compute_occupancy(qd, return_winding=True)
    assert torch.equal(occ, exact.compute_occupancy(qd)) and torch.equal(w, fast.winding_number(qd))
    assert torch.equal(exact.compute_occupancy(qd, accel="bvh"), occ)
    assert not torch.equal(w, exact.winding_number(qd))                  # an approximation, and said so
    assert float((w - exact.winding_number(qd)).abs().max()) <= 0.05
    assert torch.equal(fast.compute_signed_distance(qd), exact.compute_signed_distance(qd))
    assert torch.equal(meshprep.is_inside(fast, None, qd, method="winding"), occ > 0)
    grid = voxelize.voxelize_winding(vd, fd, 16, accel="bvh")
    assert torch.equal(grid.packed, voxelize.voxelize_winding(vd, fd, 16).packed) and grid.count() > 0
    assert torch.equal(voxelize.voxelize_winding(vd, fd, 16, accel="bvh", beta=3.0).packed, grid.packed)


# ---- 7. the drivers ----------------------------------------------------------------------------------------------------------------
def test_evaluate_driver_winding_accel(tmp_path):
    from examples import evaluate as E
    gen, ref = tmp_path / "gen", tmp_path / "ref"
    gen.mkdir(), ref.mkdir()
    hv, hf, _ = holed()
    cv, cf = rr.icosphere(3)
    mesh_udf_ref.write_obj(gen / "ball.obj", hv, hf)
    mesh_udf_ref.write_obj(ref / "ball.obj", cv, cf)
    base = ["--generated", str(gen), "--reference", str(ref), "--paired", "--num_points", "256", "--normalize", "none",
            "--output", str(tmp_path / "m.json"), "--voxel_iou", "16", "--voxel_mode", "winding"]
    exact = E.run(E.parse(base))
    assert "winding_accel" not in exact["options"]
    fast = E.run(E.parse(base + ["--winding_accel", "bvh", "--winding_beta", "3"]))
    assert fast["options"]["winding_accel"] == "bvh" and fast["options"]["winding_beta"] == 3.0
    assert fast["items"]["ball"]["voxel_iou"] == exact["items"]["ball"]["voxel_iou"] > 0.9


def test_preprocess_udfs_winding_accel(tmp_path):
    from examples import preprocess_udfs as P
    v, f, holes = holed()
    mesh_udf_ref.write_obj(tmp_path / "ball.obj", v, f)
    base = [str(tmp_path / "ball.obj"), "--num_surface_points", "3000", "--num_queries_per_std", "1500", "1000", "250", "2000", "--seed", "5",
            "--signed", "--sign", "winding", "--num_queries_on_surface", "200"]
    items = {}
    for tag, extra in (("exact", []), ("named", ["--winding_accel", "exact"]), ("bvh", ["--winding_accel", "bvh"]),
                       ("inf", ["--winding_accel", "bvh", "--winding_beta", "inf"])):
        P.run(P.parse(base + ["--output_dir", str(tmp_path / tag)] + extra))
        items[tag] = dict(np.load(tmp_path / tag / "ball.npz"))
    for k in items["exact"]:                                             # naming the default changes nothing
        assert np.array_equal(items["exact"][k], items["named"][k]), k
    z, e = items["bvh"], items["exact"]
    assert sorted(z) == sorted(e)
    for k in ("coords", "pcd", "vertices", "triangles"):                 # the same random numbers either way
        assert np.array_equal(z[k], e[k]), k
    assert np.array_equal(np.abs(z["labels"]), np.abs(e["labels"])) and z["labels"].dtype == e["labels"].dtype
    assert not z["labels"][:200].any() and not z["gradients"][:200].any() and z["gradients"].shape == e["gradients"].shape
    q = z["coords"][200:].astype(np.float64)
    radius = np.linalg.norm(q, axis=1)
    kept = np.abs(radius - 0.75) > 0.05
    for h in holes:
        kept &= np.linalg.norm(q - h, axis=1) > 0.35
    assert kept.sum() > 500
    assert np.array_equal(z["labels"][200:][kept] < 0, radius[kept] < 0.75)
    # beta = inf: every triangle exactly, in another order; a sign can differ only where |w| is within F 2^-50 of 1/2
    assert np.array_equal(items["inf"]["labels"][200:][kept], e["labels"][200:][kept])
