"""GPU tests of mesh preprocessing (surfd_amd/meshprep.py, csrc/meshdist.hip) against mathematics in fp64
(tests/mesh_udf_ref.py).  Every test here fails on a tree without surfd_amd/meshprep.py.

The distance tolerance is measured, not chosen.  `python tests/mesh_udf_ref.py` evaluates the kernel's formulas in numpy at fp32
(kernel_formulas_fp32: neither the code under test nor its output) against the fp64 oracle on this file's own meshes and
queries (mesh_udf_ref.test_meshes, 20 000 pipeline-made queries each) and prints the largest |dist32 - dist64| per mesh:
    wavy_sheet 3 042 triangles: 9.944e-08    convex_polyhedron 5 120: 8.971e-08    spliced_sheet 3 212: 3.532e-08
    zero_area 200: 4.990e-08    needles 400 (edges ~0.5, aspect 2^-20 .. 1e-2; 20 200 queries, half of them uniform): 1.380e-07
FP32_RESTATEMENT_ERROR is the largest of them; the kernel may order its additions differently (and its reciprocal is the
hardware's), so 4 x that is allowed.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_udf_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_RESTATEMENT_ERROR = 1.380e-07          # measured: see the docstring
TOL = 4 * FP32_RESTATEMENT_ERROR
STABILITY_REPEATS = 40                      # as tests/test_gpu_dgcnn.py


def cu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


@pytest.fixture(scope="module")
def M():
    from surfd_amd import meshprep
    return meshprep


@pytest.fixture(scope="module")
def cases():
    """name -> (v, t, q, dist64): the meshes of mesh_udf_ref.test_meshes with their queries and the oracle's distances"""
    out = {}
    for name, (v, t, seed) in R.test_meshes().items():
        q = R.test_queries(name, v, t, seed)
        out[name] = (v, t, q, R.closest_fp64(v, t, q)[0])
    return out


def run(M, v, t, q, **kw):
    d, p, j = M.closest_points(cu(v), cu(t), cu(q), **kw)
    torch.cuda.synchronize()
    return d.cpu().numpy(), p.cpu().numpy(), j.cpu().numpy()


def check_against_fp64(v, t, q, d64, d, p, j, tol=TOL):
    """items 6 and 7 of the issue, for 100 % of the queries"""
    assert np.isfinite(d).all() and np.isfinite(p).all()
    assert j.min() >= 0 and j.max() < len(t)
    e_d = np.abs(d.astype(np.float64) - d64).max()
    e_on = R.point_triangle_fp64(v, t, j, p).max()
    e_qp = np.abs(np.linalg.norm(q.astype(np.float64) - p.astype(np.float64), axis=1) - d64).max()
    print(f"max |dist - dist64| = {e_d:.3e}, max dist(point, its triangle) = {e_on:.3e}, max | |q - point| - dist64 | = {e_qp:.3e} (tol {tol:.3e})")
    assert e_d <= tol
    assert e_on <= tol
    assert e_qp <= tol


@pytest.mark.parametrize("name", ["wavy_sheet", "convex_polyhedron"])
def test_distance_point_and_triangle_against_fp64(M, cases, name):
    v, t, q, d64 = cases[name]
    assert len(q) >= 20000 and len(t) >= 3000
    d, p, j = run(M, v, t, q)
    check_against_fp64(v, t, q, d64, d, p, j)


def test_constructed_answers_on_the_convex_polyhedron(M):
    v, t, face = R.convex_polyhedron()
    v64 = v.astype(np.float64)
    g = np.random.default_rng(8)
    n_q = 4000
    pick = g.integers(0, len(t), n_q)
    w = g.dirichlet([3.0, 3.0, 3.0], n_q)                                 # strictly inside
    a, b, c = v64[t[pick, 0]], v64[t[pick, 1]], v64[t[pick, 2]]
    cpt = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    s = 10.0 ** g.uniform(-4, np.log10(0.5), n_q)
    q = (cpt + s[:, None] * n).astype(np.float32)
    # the fp32 query is not exactly c + s n: the constructed answers are taken for the query as stored
    q64 = q.astype(np.float64)
    s_q = ((q64 - cpt) * n).sum(1)
    c_q = q64 - s_q[:, None] * n
    d, p, j = run(M, v, t, q)
    for x, y in zip((d, p, j), run(M, v, t, q, brute_force=True)):        # culled == brute force on the constructed queries too
        assert np.array_equal(x, y)
    assert np.abs(d - s_q).max() <= TOL
    assert np.abs(p - c_q).max() <= TOL
    # "that face": the flat face of the polyhedron; within it the foot of the query may have crossed into a coplanar neighbour
    # of the picked triangle by the rounding of q, so the triangle must hold the foot within the tolerance
    assert (face[j] == face[pick]).all()
    assert R.point_triangle_fp64(v, t, j, c_q).max() <= TOL
    udf, grad = M.compute_udf_and_gradients(cu(v), cu(t), cu(q))
    udf, grad = udf.cpu().numpy(), grad.cpu().numpy().astype(np.float64)
    assert np.abs(udf - s_q).max() <= TOL
    # q - point is off s n by at most TOL in length, so the angle to n is at most asin(TOL / s) (and the norm is 1 to fp32)
    cosang = np.clip((grad * n).sum(1) / np.linalg.norm(grad, axis=1), -1, 1)
    assert (np.arccos(cosang) <= np.arcsin(np.minimum(1.0, TOL / s_q)) + 1e-6).all()
    # queries exactly on mesh vertices
    d, p, j = run(M, v, t, v)
    assert (d == 0.0).all() and np.array_equal(p, v)
    for x, y in zip((d, p, j), run(M, v, t, v, brute_force=True)):        # exact-zero ties between neighbours go by the index
        assert np.array_equal(x, y)
    udf, grad = M.compute_udf_and_gradients(cu(v), cu(t), cu(v))
    assert bool((udf == 0).all()) and bool((grad == 0).all())


def test_degenerate_triangles(M, cases):
    v, t, q, d64 = cases["spliced_sheet"]
    area = R.triangle_areas_fp64(v, t)
    longest = np.maximum.reduce([np.linalg.norm(v[t[:, i]].astype(np.float64) - v[t[:, k]], axis=1) for i, k in ((1, 0), (2, 0), (2, 1))])
    flat = 2 * area <= 1e-5 * longest ** 2                                # no area, or collinear up to the rounding of the vertices
    assert (area == 0).sum() >= 40 and flat.sum() >= 70                   # the spliced zero-area triangles are really there
    d, p, j = run(M, v, t, q)
    check_against_fp64(v, t, q, d64, d, p, j)
    # long needles over the whole range of aspects from 1e-2 down to 2^-20, half of the queries far away
    v, t, q, d64 = cases["needles"]
    edges = np.linalg.norm(v[t[:, 1]].astype(np.float64) - v[t[:, 0]], axis=1)
    aspect = 2 * R.triangle_areas_fp64(v, t) / np.maximum.reduce([np.linalg.norm(v[t[:, i]].astype(np.float64) - v[t[:, k]], axis=1) for i, k in ((1, 0), (2, 0), (2, 1))]) ** 2
    assert aspect.min() < 2e-6 and aspect.max() > 5e-3 and np.median(edges) > 0
    d, p, j = run(M, v, t, q)
    check_against_fp64(v, t, q, d64, d, p, j)
    v, t, q, d64 = cases["zero_area"]
    d, p, j = run(M, v, t, q)
    check_against_fp64(v, t, q, d64, d, p, j)                             # distances to its segments and points
    d, p, _ = run(M, v, t, v)                                             # on the degenerate triangles' own vertices
    assert np.isfinite(d).all() and d.max() <= TOL


def big_case():
    v, t = R.wavy_sheet(240)                                              # 114 242 triangles
    q = R.pipeline_queries(v, t, 105, per_sigma=36000, uniform=12000, cloud=20000)   # 120 000 queries
    return v, t, q


def test_culled_equals_brute_force_bit_for_bit(M, cases):
    for name, (v, t, q, _) in cases.items():
        a = run(M, v, t, q)
        b = run(M, v, t, q, brute_force=True)
        for x, y, what in zip(a, b, ("dist", "point", "tri")):
            assert np.array_equal(x, y), (name, what)
    v, t, q = big_case()
    assert len(t) >= 10 ** 5 and len(q) >= 10 ** 5
    md = M.MeshDistance(cu(v), cu(t))
    qd = cu(q)
    a = md.closest(qd, count_skipped=True)
    skipped, total = md.last_skipped_tiles, md.last_total_tiles
    b = md.closest(qd, brute_force=True)
    for x, y, what in zip(a, b, ("dist", "point", "tri")):
        assert torch.equal(x, y), what
    print(f"culling skipped {skipped} of {total} (wave, tile) visits = {skipped / total:.4f}")
    assert 0 < skipped <= total
    # a sample of the big case against fp64 (the whole of it is 1.4e10 pairs in numpy)
    sel = np.random.default_rng(1).choice(len(q), 300, replace=False)
    d64 = R.closest_fp64(v, t, q[sel], chunk=16)[0]
    assert np.abs(a[0].cpu().numpy()[sel] - d64).max() <= TOL


def test_outputs_do_not_depend_on_the_other_queries(M, cases):
    v, t, q, _ = cases["spliced_sheet"]
    md = M.MeshDistance(cu(v), cu(t))
    qd = cu(q)
    full = md.closest(qd)
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(len(q), generator=g).cuda()
    got = md.closest(qd[perm])
    for x, y in zip(full, got):
        assert torch.equal(x[perm], y)
    sub = perm[:777]
    got = md.closest(qd[sub].contiguous())
    for x, y in zip(full, got):
        assert torch.equal(x[sub], y)
    got = md.closest(qd[:1])
    for x, y in zip(full, got):
        assert torch.equal(x[:1], y)
    d0, p0, j0 = md.closest(qd[:0])
    assert d0.shape == (0,) and p0.shape == (0, 3) and j0.shape == (0,)


def test_distance_does_not_depend_on_the_triangle_order(M, cases):
    for name in ("wavy_sheet", "spliced_sheet"):
        v, t, q, _ = cases[name]
        d = run(M, v, t, q)[0]
        perm = np.random.default_rng(2).permutation(len(t))
        d2, p2, j2 = run(M, v, t[perm], q)
        assert np.array_equal(d, d2), name
        assert R.point_triangle_fp64(v, t[perm], j2, p2).max() <= TOL


def test_repeated_calls_are_bit_identical(M, cases):
    v, t, q, _ = cases["convex_polyhedron"]
    md = M.MeshDistance(cu(v), cu(t))
    qd = cu(q)
    first = md.closest(qd)
    for _ in range(STABILITY_REPEATS):
        again = md.closest(qd)
        for x, y in zip(first, again):
            assert torch.equal(x, y)
    other = M.MeshDistance(cu(v), cu(t)).closest(qd)
    for x, y in zip(first, other):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["cube", "sheet"])
def test_workspace_regrowth_changes_nothing(M, name):
    """One handle: 64 queries, then 5000, then the first 64 again.  The handle's arena (csrc/meshscene.h) holds S * Q partial
    results, so the second call has to free and allocate it and the third runs in an arena larger than it needs.  Every call
    equals the same call on a fresh handle.  cube: 12 triangles, one chunk, S = 1; sheet: 450 triangles, two chunks, S = 2."""
    import raycast_ref as rr
    v, t = rr.cube() if name == "cube" else rr.wavy_sheet(16)
    assert len(t) == (12 if name == "cube" else 450)
    vd, td = cu(v), cu(t)
    q = cu(np.random.default_rng(11).uniform(-1, 1, (5000, 3)).astype(np.float32))
    small = q[:64].contiguous()
    md = M.MeshDistance(vd, td)
    for queries in (small, q, small):
        got = md.closest(queries)
        fresh = M.MeshDistance(vd, td).closest(queries)
        for x, y in zip(got, fresh):
            assert torch.equal(x, y)


def test_bad_indices_are_a_return_code(M):
    import ctypes as C
    from surfd_amd import _native as N
    v = torch.zeros(4, 3).cuda()
    t = torch.tensor([[0, 1, 2], [1, 2, 9]], dtype=torch.int32).cuda()
    h = C.c_void_p()
    assert N.lib().surfd_mesh_create(N.ptr(v), 4, N.ptr(t), 2, N.stream(), C.byref(h)) == -1
    assert b"outside" in N.lib().surfd_last_error() and not h.value
    t[1, 2] = -1
    assert N.lib().surfd_mesh_create(N.ptr(v), 4, N.ptr(t), 2, N.stream(), C.byref(h)) == -1
    t[1, 2] = 3
    N.check(N.lib().surfd_mesh_create(N.ptr(v), 4, N.ptr(t), 2, N.stream(), C.byref(h)))
    assert N.lib().surfd_mesh_num_triangles(h) == 2
    assert N.lib().surfd_mesh_closest(h, N.ptr(v), -1, 0, None, None, None, None, N.stream()) == -1        # negative Q
    assert N.lib().surfd_mesh_closest(h, None, 0, 0, None, None, None, None, N.stream()) == 0              # Q = 0: a no-op
    assert N.lib().surfd_mesh_closest(h, N.ptr(v), 4, 0, None, None, None, None, N.stream()) == 0          # all outputs null
    torch.cuda.synchronize()
    N.lib().surfd_mesh_destroy(h)
    with pytest.raises(ValueError, match="outside"):
        M.MeshDistance(v, torch.tensor([[0, 1, 7]]).cuda())


def test_sampler(M):
    v, t = R.wavy_sheet()
    vd, td = cu(v), cu(t)
    g = torch.Generator(device="cuda").manual_seed(11)
    pts = M.sample_points_uniformly(vd, td, 50000, generator=g)
    assert pts.shape == (50000, 3) and pts.dtype == torch.float32
    again = M.sample_points_uniformly(vd, td, 50000, generator=torch.Generator(device="cuda").manual_seed(11))
    assert torch.equal(pts, again)
    # every sampled point lies on the mesh
    assert float(M.point_to_mesh_distance(pts, vd, td).max()) <= TOL
    # area weights: chi-square of the per-triangle counts of 1e6 samples.  64 triangles -> 63 degrees of freedom; the 99.9 %
    # quantile of chi2(63) is 103.4 (seed fixed, so the test is deterministic; a wrong weighting gives thousands)
    v, t = R.area_ladder()
    area = R.triangle_areas_fp64(v, t)
    assert area.max() / area.min() >= 99
    md = M.MeshDistance(cu(v), cu(t))
    n = 10 ** 6
    pts = M.sample_points_uniformly(cu(v), cu(t), n, generator=torch.Generator(device="cuda").manual_seed(12))
    d, _, j = md.closest(pts)
    assert float(d.max()) <= TOL
    counts = np.bincount(j.cpu().numpy(), minlength=len(t)).astype(np.float64)
    expect = n * area / area.sum()
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print(f"chi2 = {chi2:.1f} (63 degrees of freedom)")
    assert chi2 < 103.4


def test_mesh_distance(M):
    v, t = R.wavy_sheet()
    vd, td = cu(v), cu(t)
    same = M.mesh_distance(vd, td, vd, td, n=50000, generator=torch.Generator(device="cuda").manual_seed(1))
    assert same["d12"] <= TOL and same["d21"] <= TOL and same["sum"] == same["d12"] + same["d21"]
    shift = np.array([0.0, 0.0, 0.05], np.float32)
    v2 = (v + shift).astype(np.float32)
    n = 4000
    got = M.mesh_distance(vd, td, cu(v2), td, n=n, generator=torch.Generator(device="cuda").manual_seed(2))
    # the oracle on the same samples: the same generator calls in the same order reproduce them, so the two means agree within
    # the distance tolerance (tighter than the sampling error of either mean, which is about 0.05 / sqrt(n))
    g = torch.Generator(device="cuda").manual_seed(2)
    p1 = M.sample_points_uniformly(vd, td, n, generator=g).cpu().numpy()
    p2 = M.sample_points_uniformly(cu(v2), td, n, generator=g).cpu().numpy()
    ref12 = R.closest_fp64(v2, t, p1)[0]
    ref21 = R.closest_fp64(v, t, p2)[0]
    print(f"d12 {got['d12']:.9f} vs fp64 {ref12.mean():.9f}; d21 {got['d21']:.9f} vs fp64 {ref21.mean():.9f}")
    assert abs(got["d12"] - ref12.mean()) <= TOL and abs(got["d21"] - ref21.mean()) <= TOL
    assert abs(got["sum"] - (ref12.mean() + ref21.mean())) <= 2 * TOL
    d12 = M.point_to_mesh_distance(cu(p1), cu(v2), td).cpu().numpy()
    assert np.abs(d12 - ref12).max() <= TOL
    assert 0 < got["d12"] <= 0.05 + TOL and 0 < got["d21"] <= 0.05 + TOL


def test_end_to_end_drivers(M, tmp_path):
    meshes = tmp_path / "meshes"
    meshes.mkdir()
    v, t = R.wavy_sheet(24)
    R.write_obj(meshes / "sheet.obj", v, t)
    pv, pt, _ = R.convex_polyhedron(levels=2)
    R.write_obj(meshes / "poly.obj", pv, pt)
    out = tmp_path / "udfs"
    env = dict(os.environ, PYTHONPATH=ROOT)
    counts = [3000, 2000, 500, 500]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "preprocess_udfs.py"), str(meshes), "--output_dir", str(out),
                        "--num_surface_points", "12000", "--num_queries_per_std", *map(str, counts), "--seed", "5"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for name, nv, nt in (("sheet", len(v), len(t)), ("poly", len(pv), len(pt))):
        z = np.load(out / f"{name}.npz")
        assert sorted(z.files) == ["coords", "gradients", "labels", "pcd", "triangles", "vertices"]
        assert z["vertices"].shape == (nv, 3) and z["vertices"].dtype == np.float32
        assert z["triangles"].shape == (nt, 3) and z["triangles"].dtype == np.int64
        assert z["pcd"].shape == (12000, 3) and z["pcd"].dtype == np.float32
        assert z["coords"].shape == (sum(counts), 3) and z["coords"].dtype == np.float32
        assert z["labels"].shape == (sum(counts),) and z["labels"].dtype == np.float32
        assert z["gradients"].shape == (sum(counts), 3) and z["gradients"].dtype == np.float32
        assert z["labels"].min() >= 0 and z["labels"].max() <= np.float32(0.1)
        assert np.abs(z["coords"]).max() <= 1.0
        gn = np.linalg.norm(z["gradients"].astype(np.float64), axis=1)
        assert ((gn == 0) | (np.abs(gn - 1) <= 1e-6)).all()
        # the labels are the clipped fp64 distances of the written queries to the written mesh
        sel = np.random.default_rng(0).choice(sum(counts), 500, replace=False)
        d64 = np.minimum(R.closest_fp64(z["vertices"], z["triangles"], z["coords"][sel])[0], 0.1)
        assert np.abs(z["labels"][sel] - d64).max() <= TOL
    rec = tmp_path / "rec"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "reconstruct.py"), "--synthetic", "--metrics", "--resolution", "64",
                        "--output_dir", str(rec), str(out)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    m = json.load(open(rec / "metrics.json"))
    assert sorted(m) == ["poly", "sheet"]
    for item in m.values():
        assert np.isfinite(item["udf_mean_abs_error"]) and item["udf_mean_abs_error"] >= 0
        if item["faces"]:
            assert all(np.isfinite(item[k]) and item[k] >= 0 for k in ("reconstruction_to_original", "original_to_reconstruction", "mesh_distance"))
