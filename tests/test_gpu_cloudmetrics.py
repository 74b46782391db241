"""GPU tests of the point-cloud metrics (surfd_amd/cloudmetrics.py, csrc/cloudnn.hip; run with -m gpu on an MI355X) against the
yardsticks of tests/cloud_ref.py.  Every test here fails on a tree without surfd_amd/cloudmetrics.py.

Bounds (u = 2^-24; derived, not tuned):
  * nearest_neighbors: d2 bit-equal and idx equal to the fp32 restatement for 100 % of the points (min only selects).
  * a directed mean: within 1 fp32 ulp of float32(fp64 sum of the restatement's d2 / Na) (the fp64 summation order is free, so
    the last rounding may land on either neighbour, nothing more) and within a relative 7 u of the fp64 mathematics: on the path
    of the dx^2 term lie the subtraction (counted twice by the square), the multiplication and two additions, <= 5 u on d2, all
    terms being non-negative; the minimum of values each within 5 u of the truth is within 5 u of the true minimum; the fp64
    sum adds nothing visible; the final rounding <= 1 u; 1 u is spare for second-order terms.  `python tests/cloud_ref.py`
    measures the fp32 restatement against fp64 on its own 58 cloud pairs: largest relative error of a mean 0.933 u.
  * a Chamfer distance (two directed means added in fp32): 8 u.
  * a directed mean against the kernel's own summation order (cloud_ref.mean_kernel_order, the order csrc/cloudnn.hip's header
    states): 0 ulp, for 100 % of the entries.  No tolerance: the header fixes every fp64 addition, fp64 addition is commutative,
    and the d2 that are summed are bit-equal to the restatement's (min only selects).  The 1-ulp and 7 u checks above stay.

Launch plans and tile edges (items 11 to 18; which path a shape takes is asked of surfd_cloud_nn_matrix_plan, never restated):
  * every template instance P = 1, 2, 4, 8 and 1, 2, 3 register tiles of the query cloud, at both sides of every Na boundary,
    against candidate clouds of 1, 3, 4, 5 points (a tile shorter than the unroll, equal to it, one past it) and at both sides
    of one and two candidate tiles (2 047 ... 4 097), random clouds and lattice clouds full of ties and duplicates;
  * every launch plan: one candidate cloud per workgroup, several (span > 1), a ragged last range, span > 1 with the query
    registers loaded once and with them reloaded per candidate cloud, span > 1 over two candidate tiles; candidate clouds of
    one range differ in seed and in scale, so a sum, a count or a minimum carried over from the previous cloud shows;
  * cn_nn_kernel with winners in the second and third candidate tile, ties across tiles and with a tile's padding copies,
    Nb = 2, 3, 5, and the grid's y limit B = 65 535;
  * the threshold compare with d2 == tau2 on many points (strict); d2 = +inf from finite inputs and subnormal d2;
  * optional outputs, and sentinels around every output: nothing outside [B, Na] or [M, R] is written;
  * the association of the four wave sums on a cloud built so that it decides the fp32 result (cloud_ref.wave_order_case).
"""
import ctypes
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = R.U
STABILITY_REPEATS = 40                      # as tests/test_gpu_dgcnn.py
TAU = 0.05
TAU2 = float(np.float32(TAU * TAU))
SENT_F, SENT_I = -7.0, -7                   # what an output buffer holds before a raw call: no d2, mean or count is negative
PAD = 64                                    # sentinel elements on either side of an output
ERR_UNSUPPORTED = -4


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.fixture(scope="module")
def CM():
    from surfd_amd import cloudmetrics
    return cloudmetrics


@pytest.fixture(scope="module")
def small_sets():
    """name -> (A [5, Na, 3], B [7, Nb, 3]) for item 6 / 7: 2 048-point clouds, and sizes that cross every tile edge"""
    out = {"n2048": (np.concatenate((R.family("shell", 3), R.family("torus", 2))), np.concatenate((R.family("shell", 3, first=5), R.family("torus", 4, first=5))))}
    out["odd"] = (np.concatenate((R.family("shell", 3, 777), R.family("torus", 2, 777))),
                  np.concatenate((R.family("shell", 3, 2049, first=5), R.family("torus", 4, 2049, first=5))))
    return out


@pytest.fixture(scope="module")
def metric_data():
    """(clouds [24, 2048, 3], splits, the fp64 matrix of directed means [24, 24])"""
    allc, splits = R.metric_sets()
    return allc, splits, R.matrix_f64(allc, allc)


# ---- 5. nearest neighbours ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "lattice"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Na,Nb", [(1, 1), (63, 777), (777, 63), (2048, 2048), (10000, 2048)])
def test_nearest_neighbors_equal_the_restatement(CM, kind, B, Na, Nb):
    make = R.random_cloud if kind == "random" else R.lattice_cloud
    a, b = make(B, Na, seed=Na + B), make(B, Nb, seed=7 * Nb + B + 1)
    d2, idx = CM.nearest_neighbors(cu(a), cu(b))
    assert d2.dtype == torch.float32 and idx.dtype == torch.int64 and d2.shape == idx.shape == (B, Na)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    for i in range(B):
        rd, ri = R.nn_f32(a[i], b[i])
        assert np.array_equal(idx[i], ri), f"{int((idx[i] != ri).sum())} of {Na} indices differ"
        assert np.array_equal(d2[i].view(np.int32), rd.view(np.int32)), f"{int((d2[i] != rd).sum())} of {Na} d2 differ"
    if kind == "lattice" and Nb >= 10:
        assert any(len(np.unique(b[i], axis=0)) < Nb for i in range(B))      # the candidates do hold duplicates


@pytest.mark.parametrize("kind", ["random", "lattice"])
def test_nearest_neighbors_of_a_cloud_in_itself(CM, kind):
    x = (R.random_cloud if kind == "random" else R.lattice_cloud)(2, 3000, seed=11)
    d2, idx = CM.nearest_neighbors(cu(x), cu(x))
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    assert (d2 == 0).all()
    n = np.arange(3000)[None]
    assert (idx <= n).all()                                              # the point itself or a lower-indexed duplicate
    assert np.array_equal(np.take_along_axis(x, idx[..., None], 1), x)
    if kind == "lattice":
        assert (idx < n).any()


# ---- 6. the directed means ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n2048", "odd"])
@pytest.mark.parametrize("swap", [False, True])
def test_directed_means_against_restatement_and_fp64(CM, small_sets, name, swap):
    A, B = small_sets[name][::-1] if swap else small_sets[name]
    mean, below = CM.directed_means(cu(A), cu(B), tau2=TAU2)
    assert mean.shape == below.shape == (len(A), len(B)) and mean.dtype == torch.float32 and below.dtype == torch.int32
    mean, below = mean.cpu().numpy(), below.cpu().numpy()
    m32, c32 = R.matrix_f32(A, B, TAU2)
    m64 = R.matrix_f64(A, B)
    ulps = R.ulp_distance(mean, m32)
    rel = np.abs(mean.astype(np.float64) - m64) / m64
    print(f"{name} swap={swap}: max ulp distance to the fp32 restatement {ulps.max()}; max relative error vs fp64 {rel.max() / U:.3f} u "
          f"(bound 7 u); restatement vs fp64 {(np.abs(m32.astype(np.float64) - m64) / m64).max() / U:.3f} u")
    assert ulps.max() <= 1
    assert rel.max() <= R.MEAN_BOUND
    assert np.array_equal(below, c32)
    assert 0 < c32.min() and c32.max() < A.shape[1]                     # the threshold does cut through the clouds


# ---- 7. invariances, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n2048", "odd"])
def test_entries_do_not_depend_on_the_call(CM, small_sets, name):
    A, B = (cu(x) for x in small_sets[name])
    mean, below = CM.directed_means(A, B, tau2=TAU2)
    for i, j in ((0, 0), (4, 6), (2, 3)):
        m1, c1 = CM.directed_means(A[i:i + 1], B[j:j + 1], tau2=TAU2)
        assert torch.equal(m1[0, 0], mean[i, j]) and torch.equal(c1[0, 0], below[i, j])
    for chunk in (1, 2, 3):
        mc, cc = CM.directed_means(A, B, tau2=TAU2, chunk=chunk)
        assert torch.equal(mc, mean) and torch.equal(cc, below)
    full = CM.chamfer_matrix(A, B)
    assert torch.equal(full, mean + CM.directed_means(B, A)[0].t())
    assert torch.equal(CM.chamfer_matrix(A, B, chunk=2), full)
    # a set against itself: the shortcut (one direction, transposed) equals the two launches on a copy
    assert torch.equal(CM.chamfer_matrix(A, A), CM.chamfer_matrix(A, A.clone()))
    # any order of the candidate cloud's points
    g = torch.Generator().manual_seed(5)
    perm = torch.randperm(B.shape[1], generator=g).cuda()
    mp, cp = CM.directed_means(A, B[:, perm].contiguous(), tau2=TAU2)
    assert torch.equal(mp, mean) and torch.equal(cp, below)


def test_repeated_calls_give_one_output(CM, small_sets):
    A, B = (cu(x) for x in small_sets["n2048"])
    outs = set()
    for _ in range(STABILITY_REPEATS):
        mean, below = CM.directed_means(A, B, tau2=TAU2)
        d2, idx = CM.nearest_neighbors(A, B[:5])
        outs.add((mean.cpu().numpy().tobytes(), below.cpu().numpy().tobytes(), d2.cpu().numpy().tobytes(), idx.cpu().numpy().tobytes()))
    assert len(outs) == 1


# ---- 8. set metrics end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["same", "disjoint", "copy"])
def test_set_metrics_against_fp64(CM, metric_data, split):
    allc, splits, m64 = metric_data
    gi, ri = splits[split]
    D64 = m64 + m64.T
    D_gr, D_gg, D_rr = R.split_matrices(D64, gi, ri)
    gaps = R.assert_decided(D_gr, D_gg, D_rr)                           # a condition on the inputs: 100 % of the rows
    want_mc, want_nna = R.mmd_cov_f64(D_gr), R.one_nna_f64(D_gg, D_rr, D_gr)
    got = CM.compute_all_metrics(cu(allc[gi]), cu(allc[ri]), return_matrices=True)
    rel = np.abs(got["D_gr"].cpu().numpy().astype(np.float64) - D_gr) / np.maximum(D_gr, 1e-300)
    print(f"{split}: smallest arg-min gaps {gaps}; D_gr max relative error {rel.max() / U:.3f} u (bound 8 u); "
          f"mmd {got['mmd_cd']:.9g} vs {want_mc['mmd']:.9g}, cov {got['cov_cd']} vs {want_mc['cov']}, 1-nna {got['1nna_cd']} vs {want_nna['acc']}")
    assert rel.max() <= 8 * U
    assert all(isinstance(got[k], float) for k in ("mmd_cd", "cov_cd", "1nna_cd"))
    assert abs(got["mmd_cd"] - want_mc["mmd"]) <= 8 * U * want_mc["mmd"]
    assert abs(got["mmd_smp_cd"] - want_mc["mmd_smp"]) <= 8 * U * want_mc["mmd_smp"]
    assert got["cov_cd"] == want_mc["cov"]
    assert got["1nna_cd"] == want_nna["acc"] and got["1nna_cd_gen"] == want_nna["acc_gen"] and got["1nna_cd_ref"] == want_nna["acc_ref"]
    assert CM.compute_all_metrics(cu(allc[gi]), cu(allc[ri]), chunk=5) == {k: v for k, v in got.items() if not k.startswith("D_")}
    if split == "copy":
        assert got["cov_cd"] == 1.0 and got["mmd_cd"] == 0.0 and got["1nna_cd"] <= 0.5
    if split == "disjoint":
        assert got["1nna_cd"] == 1.0


# ---- 9. paired Chamfer distance and F-score ------------------------------------------------------------------------------------------
def test_chamfer_distance_against_fp64(CM):
    g = np.random.default_rng(4)
    a = np.concatenate((R.family("shell", 2, 2048), R.family("torus", 2, 2048)))
    b = (a[:, ::-1] + g.normal(0, 0.03, a.shape)).astype(np.float32)[:, :1500].copy()    # a noisy, smaller copy of every cloud
    d2ab = np.stack([R.nn_f64(a[i], b[i]) for i in range(4)])
    d2ba = np.stack([R.nn_f64(b[i], a[i]) for i in range(4)])
    for d2 in (d2ab, d2ba):                                             # a condition on the inputs: no d2 within 6 u of tau^2
        assert (np.abs(d2 - TAU2) > 6 * U * TAU2).all()
    want_p, want_r = (d2ab < TAU2).mean(1), (d2ba < TAU2).mean(1)
    assert (0 < want_p).all() and (want_p < 1).all() and (0 < want_r).all() and (want_r < 1).all()
    want_cd = d2ab.mean(1) + d2ba.mean(1)
    got = {k: v.cpu().numpy() for k, v in CM.chamfer_distance(cu(a), cu(b), f_threshold=TAU).items()}
    assert sorted(got) == ["cd", "d_ab", "d_ba", "fscore", "precision", "recall"]
    assert all(v.shape == (4,) and v.dtype == np.float32 for v in got.values())
    print(f"cd max relative error {(np.abs(got['cd'] - want_cd) / want_cd).max() / U:.3f} u (bound 8 u); precision {got['precision']}, recall {got['recall']}")
    assert (np.abs(got["cd"].astype(np.float64) - want_cd) <= 8 * U * want_cd).all()
    assert (np.abs(got["d_ab"].astype(np.float64) - d2ab.mean(1)) <= 7 * U * d2ab.mean(1)).all()
    assert np.array_equal(got["precision"], want_p.astype(np.float32)) and np.array_equal(got["recall"], want_r.astype(np.float32))
    assert np.allclose(got["fscore"], 2 * want_p * want_r / (want_p + want_r), rtol=4 * U, atol=0)
    # nothing within the threshold on either side: F-score 0, not NaN
    far = CM.chamfer_distance(cu(a[:1]), cu(a[:1] + np.float32(5)), f_threshold=TAU)
    assert float(far["precision"]) == 0 and float(far["recall"]) == 0 and float(far["fscore"]) == 0
    same = CM.chamfer_distance(cu(a), cu(a))
    assert float(same["cd"].abs().max()) == 0 and float(same["fscore"].min()) == 1
    with pytest.raises(ValueError, match="NaN or Inf"):
        bad = cu(a).clone()
        bad[1, 5, 2] = float("nan")
        CM.chamfer_distance(bad, cu(b))
    with pytest.raises(ValueError, match="same batch size"):
        CM.nearest_neighbors(cu(a), cu(b[:3]))


# ---- 10. the driver -----------------------------------------------------------------------------------------------------------------
def _write_obj(path, v, t):
    with open(path, "w") as f:
        for p in v:
            f.write(f"v {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n")
        for q in t:
            f.write(f"f {q[0] + 1} {q[1] + 1} {q[2] + 1}\n")


def _box_mesh(sx, sy, sz):
    v = np.array([[x, y, z] for x in (-sx, sx) for y in (-sy, sy) for z in (-sz, sz)], np.float32)
    quads = ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3))
    t = np.array([[q[0], q[1], q[2]] for q in quads] + [[q[0], q[2], q[3]] for q in quads], np.int64)
    return v, t


def _load_like_the_driver(directory, num_points, generator, M):
    out = []
    for f in sorted(os.listdir(directory), key=lambda f: os.path.splitext(f)[0]):
        path = os.path.join(directory, f)
        if f.endswith(".obj"):
            v, t = M.read_mesh(path)
            out.append(M.sample_points_uniformly(v, t, num_points, generator=generator))
        else:
            p = torch.from_numpy(np.load(path)["pcd"])
            out.append(p[torch.randperm(len(p), generator=generator)[:num_points]])
    return torch.stack(out)


def test_evaluate_driver(CM, tmp_path):
    from surfd_amd import meshprep as M
    gen_dir, ref_dir = tmp_path / "gen", tmp_path / "ref"
    gen_dir.mkdir(); ref_dir.mkdir()
    rng = np.random.default_rng(2)
    for k in range(3):                                                  # three OBJ meshes and three .npz clouds per side
        for d, s in ((gen_dir, 1.0), (ref_dir, 1.1)):
            _write_obj(d / f"item{k}.obj", *_box_mesh(0.3 + 0.1 * k, 0.5 * s, 0.2 + 0.05 * k))
            np.savez(d / f"item{k + 3}.npz", pcd=R.torus_cloud(k + (0 if s == 1.0 else 3), 900) + rng.normal(0, 0.01, (900, 3)).astype(np.float32))
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, os.path.join(ROOT, "examples", "evaluate.py"), "--generated", str(gen_dir), "--reference", str(ref_dir),
            "--num_points", "512", "--seed", "3"]

    def direct(normalize):
        g = torch.Generator().manual_seed(3)
        gen = CM.normalize_clouds(_load_like_the_driver(gen_dir, 512, g, M), normalize).contiguous().cuda()
        ref = CM.normalize_clouds(_load_like_the_driver(ref_dir, 512, g, M), normalize).contiguous().cuda()
        return gen, ref

    r = subprocess.run(base + ["--output", str(tmp_path / "set.json")], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.load(open(tmp_path / "set.json"))
    assert out["num_generated"] == 6 and out["num_reference"] == 6
    assert out["options"] == {"num_points": 512, "normalize": "bbox", "seed": 3, "paired": False}
    want = CM.compute_all_metrics(*direct("bbox"))
    assert out["metrics"] == {k: want[k] for k in ("mmd_cd", "cov_cd", "1nna_cd")}
    assert 0 < out["metrics"]["mmd_cd"] < 0.1 and 0 < out["metrics"]["cov_cd"] <= 1 and 0 <= out["metrics"]["1nna_cd"] <= 1

    r = subprocess.run(base + ["--paired", "--normalize", "none", "--f_threshold", "0.05", "--output", str(tmp_path / "pairs.json")],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.load(open(tmp_path / "pairs.json"))
    want = {k: v.cpu().tolist() for k, v in CM.chamfer_distance(*direct("none"), f_threshold=0.05).items()}
    assert list(out["items"]) == [f"item{k}" for k in range(6)]
    for i, (name, item) in enumerate(out["items"].items()):
        assert item == {k: want[k][i] for k in ("cd", "fscore", "precision", "recall")}, name
    for k in ("cd", "fscore", "precision", "recall"):
        assert out["mean"][k] == float(np.mean(want[k], dtype=np.float64))
    assert all(0 < it["fscore"] <= 1 for it in out["items"].values())


# ---- 11. the launch plan, asked of the library ---------------------------------------------------------------------------------------
GRID_NA = (1, 2, 63, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097)
GRID_NB = (1, 3, 4, 5, 2047, 2048, 2049, 4097)
GRID_TAU2 = {"random": 0.25, "lattice": 1 / 16}      # the lattice's d2 are multiples of 1/64: 1/16 is one of them


def plan_of(M, Na, Rr):
    """(P, S, span, query_tiles) of a surfd_cloud_nn_matrix call, from the library"""
    from surfd_amd import _native as N
    out = [ctypes.c_int(-1) for _ in range(4)]
    N.check(N.lib().surfd_cloud_nn_matrix_plan(M, Na, Rr, *[ctypes.byref(v) for v in out]))
    return tuple(v.value for v in out)


def bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float32).view(np.int32)


def test_shape_grid_covers_every_instance():
    plans = [plan_of(2, Na, 3) for Na in GRID_NA]
    assert {p[0] for p in plans} == {1, 2, 4, 8}
    assert {p[3] for p in plans} == {1, 2, 3}
    assert {p[0] for p in plans if p[3] == 1} == {1, 2, 4, 8} and {p[0] for p in plans if p[3] > 1} == {8}
    assert all(p[1:3] == (3, 1) for p in plans)                         # the grid is about P and the tiles: one cloud per workgroup


# ---- 12. the directed means on the shape grid -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "lattice"])
@pytest.mark.parametrize("Nb", GRID_NB)
@pytest.mark.parametrize("Na", GRID_NA)
def test_directed_means_on_the_shape_grid(CM, kind, Na, Nb):
    make = R.random_cloud if kind == "random" else R.lattice_cloud
    A, B = make(2, Na, seed=Na), make(3, Nb, seed=7 * Nb + 1)
    tau2 = GRID_TAU2[kind]
    mean, below = CM.directed_means(cu(A), cu(B), tau2=tau2)
    plain, none = CM.directed_means(cu(A), cu(B))
    assert none is None and torch.equal(plain, mean)                    # the count is optional and changes no mean
    want, count = R.matrix_kernel_order(A, B, tau2)
    m64 = R.matrix_f64(A, B)
    got = mean.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).sum())} of 6 means differ from the kernel's order: {got} {want}"
    assert np.array_equal(below.cpu().numpy(), count)
    pos = m64 > 0
    assert (np.abs(got.astype(np.float64) - m64)[pos] <= R.MEAN_BOUND * m64[pos]).all()
    if kind == "random":
        assert pos.all()
    else:
        assert np.array_equal(got == 0, ~pos)                           # a lattice cloud can lie inside another: exactly 0 there


# ---- 13. every launch plan -----------------------------------------------------------------------------------------------------------
#             M, R, Na, Nb: the (M, R) rows of the table in tests/test_cloudmetrics_cpu.py on clouds of 5 and 7 points, then span > 1
#             with the queries reloaded per candidate cloud, with the queries loaded once at P = 8, and at P = 2 over two candidate tiles
PLAN_CASES = [(5, 7, 5, 7), (2048, 2, 5, 7), (1025, 3, 5, 7), (700, 7, 5, 7), (2049, 5, 5, 7), (3, 2049, 5, 7), (1, 2049, 5, 7),
              (1, 4100, 5, 7), (1025, 3, 2049, 5), (1025, 3, 2048, 5), (2048, 2, 300, 2049)]
PLAN_P_TILES = {(1025, 3, 2049, 5): (8, 2), (1025, 3, 2048, 5): (8, 1), (2048, 2, 300, 2049): (2, 1)}
PLAN_TAU2 = 0.25


@functools.lru_cache(maxsize=None)
def plan_case(M, Rr, Na, Nb):
    """(A [M, Na, 3], B [Rr, Nb, 3], the means in the kernel's order, the strict counts).  Every candidate cloud has a seed and a
    scale in [0.5, 1.5) of its own, so what one cloud leaves behind in a workgroup cannot pass for the next cloud's result.  The
    query clouds are all distinct, except where that would cost the host billions of point pairs: there four distinct clouds
    repeat in turn (a workgroup has one query cloud; its neighbours' clouds still differ from it)."""
    distinct = M if M * Rr * Na * Nb <= 10 ** 8 else 4
    base = R.random_cloud(distinct, Na, seed=31 * M + Rr)
    B = np.stack([R.random_cloud(1, Nb, seed=1000 + j)[0] * np.float32(0.5 + j / Rr) for j in range(Rr)])
    want, count = R.matrix_kernel_order(base, B, PLAN_TAU2)
    pick = np.arange(M) % distinct
    return base[pick], B, want[pick], count[pick]


def test_plan_cases_cover_what_they_are_meant_to():
    ragged = 0
    for M, Rr, Na, Nb in PLAN_CASES:
        P, S, span, tiles = plan_of(M, Na, Rr)
        assert S * span >= Rr > (S - 1) * span
        assert (span > 1) == ((M, Rr) != (5, 7)), (M, Rr, span)
        assert PLAN_P_TILES.get((M, Rr, Na, Nb), (1, 1)) == (P, tiles)
        ragged += Rr % span != 0
    assert ragged >= 3
    assert plan_of(1, 5, 1)[1:3] == (1, 1)                               # what chunk=1 launches


@pytest.mark.parametrize("M,Rr,Na,Nb", PLAN_CASES)
def test_every_launch_plan(CM, M, Rr, Na, Nb):
    A, B, want, count = plan_case(M, Rr, Na, Nb)
    assert (want[:, 1:] != want[:, :-1]).all() and want.min() > 0       # neighbouring candidate clouds do differ
    dA, dB = cu(A), cu(B)
    mean, below = CM.directed_means(dA, dB, tau2=PLAN_TAU2)
    bad = bits(mean) != bits(want)
    assert not bad.any(), f"{int(bad.sum())} of {M * Rr} means differ, first at (i, j) = {tuple(np.argwhere(bad)[0])}"
    assert np.array_equal(below.cpu().numpy(), count)
    assert 0 < count.sum() < M * Rr * Na                                 # the threshold does cut through the clouds
    m1, c1 = CM.directed_means(dA, dB, tau2=PLAN_TAU2, chunk=1)         # one query and one candidate cloud per launch
    assert torch.equal(m1, mean) and torch.equal(c1, below)


# ---- 14. nearest neighbours across candidate tiles -----------------------------------------------------------------------------------
def nn_against_restatement(CM, a, b):
    """a [B, Na, 3], b [B, Nb, 3]: d2 bit-equal and idx equal to the restatement for 100 % of the points; returns the restatement"""
    d2, idx = CM.nearest_neighbors(cu(a), cu(b))
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    ref = [R.nn_f32(a[i], b[i]) for i in range(len(a))]
    rd, ri = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    assert np.array_equal(idx, ri), f"{int((idx != ri).sum())} of {idx.size} indices differ"
    assert np.array_equal(bits(d2), bits(rd)), f"{int((bits(d2) != bits(rd)).sum())} of {d2.size} d2 differ"
    return rd, ri


@pytest.mark.parametrize("kind", ["random", "lattice"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Na,Nb", [(257, 2), (257, 3), (257, 5), (1, 2049), (300, 2049), (300, 4096), (300, 4097), (300, 6145)])
def test_nearest_neighbors_across_candidate_tiles(CM, kind, B, Na, Nb):
    make = R.random_cloud if kind == "random" else R.lattice_cloud
    a, b = make(B, Na, seed=Na + B), make(B, Nb, seed=7 * Nb + B + 1)
    rd, ri = nn_against_restatement(CM, a, b)
    if Na == 300 and Nb >= 4096 and kind == "random":
        assert (ri >= 2048).any() and (ri < 2048).any()                 # winners on both sides of the first tile edge
    if kind == "lattice" and Nb > 2048:
        assert (rd == 0).any()                                          # ties and duplicates: the lattice is far smaller than the cloud


def far_cloud(n, seed):
    """n points of [9, 11]^3: at least 192 away (squared) from every point of [-1, 1]^3, whose own points are at most 12 apart"""
    return R.random_cloud(1, n, seed)[0] + np.float32(10)


NEAR = np.arange(300) * 6 + 3            # where the near points go inside a tile: 3 ... 1797, every residue of the unroll


def near_copies(a, seed):
    g = np.random.default_rng(seed)
    return (a + g.normal(0, 1e-3, a.shape)).astype(np.float32)


@pytest.mark.parametrize("tile", [1, 2])
def test_winners_in_a_later_tile(CM, tile):
    a = R.random_cloud(1, 300, 5)[0]
    b = far_cloud(6145, 6)
    if tile == 1:
        b[2048 + NEAR] = near_copies(a, 7)
    else:
        b[6144] = 0                      # the third tile's only point, followed in LDS by three padding copies of itself
    rd, ri = R.nn_f32(a, b)
    assert np.array_equal(ri, 2048 + NEAR) if tile == 1 else (ri == 6144).all()
    nn_against_restatement(CM, a[None], b[None])


def test_ties_across_tiles_go_to_the_lower_index(CM):
    a = R.random_cloud(1, 300, 5)[0]
    b = far_cloud(6145, 6)
    b[NEAR] = near_copies(a, 7)
    b[2048 + NEAR] = b[NEAR]
    b[4096 + NEAR] = b[NEAR]
    rd, ri = R.nn_f32(a, b)
    assert np.array_equal(ri, NEAR)                                     # the restatement takes the first of the three equal minima
    for off in (2048, 4096):
        assert np.array_equal(R.nn_f32(a, b[off:])[0].view(np.int32), rd.view(np.int32))      # the later copies do tie, bit for bit
    nn_against_restatement(CM, a[None], b[None])
    # the last point of a tile against its padding copies: three real points and one copy, then one real point and three copies
    for Nb in (4099, 6145):
        b = far_cloud(Nb, 8)
        b[Nb - 1] = 0
        rd, ri = R.nn_f32(a, b)
        assert (ri == Nb - 1).all()
        nn_against_restatement(CM, a[None], b[None])


def test_nearest_neighbors_at_the_batch_limit(CM):
    from surfd_amd import _native as N
    B = 65535                                                           # the y limit of a grid
    a, b = R.random_cloud(B, 2, 21), R.random_cloud(B, 2, 22)
    b[::3, 1] = b[::3, 0]                                               # every third item: two equal candidates, index 0 wins
    d = a[:, :, None, :] - b[:, None, :, :]                             # the restatement of cloud_ref.nn_f32, vectorised over B
    dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert dd.dtype == np.float32 and dd.shape == (B, 2, 2)
    ri = dd.argmin(-1)
    rd = np.take_along_axis(dd, ri[..., None], -1)[..., 0]
    assert (ri[::3] == 0).all() and (ri == 1).any()
    da, db = cu(a), cu(b)
    d2, idx = CM.nearest_neighbors(da, db)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(bits(d2), bits(rd))
    # one more is refused before anything is launched
    d2 = torch.full((64,), SENT_F, device="cuda")
    idx = torch.full((64,), SENT_I, device="cuda", dtype=torch.int32)
    assert N.lib().surfd_cloud_nn(N.ptr(da), N.ptr(db), 65536, 2, 2, N.ptr(d2), N.ptr(idx), N.stream()) == ERR_UNSUPPORTED
    assert b"beyond the supported size" in N.lib().surfd_last_error()
    torch.cuda.synchronize()
    assert (d2 == SENT_F).all() and (idx == SENT_I).all()


# ---- 15. the threshold at its edge ----------------------------------------------------------------------------------------------------
ON_THE_EDGE = {1 / 64: 178, 1 / 32: 127, 3 / 64: 52, 1 / 16: 70}        # points of the query cloud with d2 == tau2, from the restatement


@pytest.mark.parametrize("tau2", sorted(ON_THE_EDGE))
def test_threshold_at_its_edge(CM, tau2):
    a, b = R.lattice_cloud(1, 777, 3), R.lattice_cloud(1, 300, 4)
    t = np.float32(tau2)
    assert float(t) == tau2
    dab, dba = R.nn_f32(a[0], b[0])[0], R.nn_f32(b[0], a[0])[0]
    on, lo, hi = int((dab == t).sum()), int((dab < t).sum()), int((dab > t).sum())
    assert on == ON_THE_EDGE[tau2] and lo >= 78 and hi >= 272           # a condition on the inputs: <= would count `on` more
    assert CM._tau2(math.sqrt(tau2)) == tau2
    mean, below = CM.directed_means(cu(a), cu(b), tau2=tau2)
    assert int(below) == lo
    assert bits(mean)[0, 0] == bits(R.mean_kernel_order(dab))[0]
    back = CM.directed_means(cu(b), cu(a), tau2=tau2)[1]
    assert int(back) == int((dba < t).sum())
    got = CM.chamfer_distance(cu(a), cu(b), f_threshold=math.sqrt(tau2))
    assert float(got["precision"]) == float(np.float32(lo / 777))
    assert float(got["recall"]) == float(np.float32(int((dba < t).sum()) / 300))


# ---- 16. extreme magnitudes, both kernels, bit for bit ------------------------------------------------------------------------------------
def both_kernels_bitwise(CM, a, b, tau2):
    """a [1, Na, 3], b [1, Nb, 3]: d2, idx, the directed mean and the strict count against the restatement; no fp64 bound applies"""
    with np.errstate(over="ignore"):
        rd, ri = R.nn_f32(a[0], b[0])
    d2, idx = CM.nearest_neighbors(cu(a), cu(b))
    assert np.array_equal(idx.cpu().numpy()[0], ri), f"{int((idx.cpu().numpy()[0] != ri).sum())} indices differ"
    assert np.array_equal(bits(d2)[0], bits(rd))
    mean, below = CM.directed_means(cu(a), cu(b), tau2=tau2)
    assert bits(mean)[0, 0] == bits(R.mean_kernel_order(rd))[0]
    assert int(below) == int((rd < np.float32(tau2)).sum())
    return rd, ri, float(mean), int(below)


def test_d2_that_overflows(CM):
    a = R.random_cloud(1, 300, 1) * np.float32(2.0 ** 66)
    b = np.ascontiguousarray(-a[:, ::-1])
    assert np.isfinite(a).all() and np.isfinite(b).all()
    for p, q in ((a, b), (b, a)):
        with np.errstate(over="ignore"):
            rd = R.nn_f32(p[0], q[0])[0]
        tau2 = float(np.sort(rd[np.isfinite(rd)])[100])                 # a d2 of the cloud itself: finite, and on the edge
        rd, ri, mean, below = both_kernels_bitwise(CM, p, q, tau2)
        assert int(np.isinf(rd).sum()) == 39 and (rd[np.isinf(rd)] > 0).all()
        assert (ri[np.isinf(rd)] == 0).all()                            # +inf against every candidate: nothing is < +inf, index 0 stays
        assert mean == float("inf") and 0 < below < 261
    # a whole cloud beyond reach: every d2 is +inf, every idx 0
    rd, ri, mean, below = both_kernels_bitwise(CM, a, np.full((1, 1, 3), 2.0 ** 70, np.float32), float(np.float32(3e38)))
    assert np.isinf(rd).all() and (ri == 0).all() and below == 0


def test_d2_that_is_subnormal(CM):
    a = R.lattice_cloud(1, 300, 2) * np.float32(2.0 ** -68)
    b = R.lattice_cloud(1, 200, 3) * np.float32(2.0 ** -68)
    tiny = np.finfo(np.float32).tiny
    unit = 2.0 ** -142                                                  # (2^-68 / 8)^2: every d2 is a small multiple of it
    rd, ri, mean, below = both_kernels_bitwise(CM, a, b, 4 * unit)
    sub = (rd > 0) & (rd < tiny)
    assert int(sub.sum()) == 230 and int((rd == 0).sum()) == 70 and not (rd >= tiny).any()
    assert (rd / np.float32(unit) == np.round(rd / np.float32(unit))).all()
    assert 0 < mean < tiny and 70 < below < 300 and (ri[sub] > 0).any()  # flushed to zero: mean 0, below 300, every idx 0
    assert (rd == np.float32(4 * unit)).any()


# ---- 17. optional outputs and the bounds of the writes, through the C ABI -----------------------------------------------------------------

def raw_nn(a, b, want_d2=True, want_idx=True):
    """surfd_cloud_nn into the middle of sentinel-filled buffers -> (d2 [B, Na], idx [B, Na]); the sentinels around them, and a
    whole output that was not asked for, must be untouched"""
    from surfd_amd import _native as N
    B, Na, Nb = a.shape[0], a.shape[1], b.shape[1]
    da, db = cu(a), cu(b)
    d2 = torch.full((PAD + B * Na + PAD,), SENT_F, device="cuda")
    idx = torch.full((PAD + B * Na + PAD,), SENT_I, device="cuda", dtype=torch.int32)
    N.check(N.lib().surfd_cloud_nn(N.ptr(da), N.ptr(db), B, Na, Nb, N.ptr(d2[PAD:]) if want_d2 else None,
                                   N.ptr(idx[PAD:]) if want_idx else None, N.stream()))
    torch.cuda.synchronize()
    for buf, sent, wanted in ((d2, SENT_F, want_d2), (idx, SENT_I, want_idx)):
        assert (buf[:PAD] == sent).all() and (buf[PAD + B * Na:] == sent).all(), "written outside [B, Na]"
        inside = buf[PAD:PAD + B * Na]
        assert (inside != sent).all() if wanted else (inside == sent).all()
    return d2[PAD:PAD + B * Na].reshape(B, Na).cpu().numpy(), idx[PAD:PAD + B * Na].reshape(B, Na).cpu().numpy()


@pytest.mark.parametrize("Na", [257, 1])
def test_cloud_nn_writes_what_it_is_asked_for_and_nothing_else(Na):
    from surfd_amd import _native as N
    a, b = R.random_cloud(3, Na, 41), R.random_cloud(3, 2049, 42)
    d2, idx = raw_nn(a, b)
    for i in range(3):
        rd, ri = R.nn_f32(a[i], b[i])
        assert np.array_equal(bits(d2[i]), bits(rd)) and np.array_equal(idx[i], ri)
    only_d2, _ = raw_nn(a, b, want_idx=False)
    _, only_idx = raw_nn(a, b, want_d2=False)
    assert np.array_equal(bits(only_d2), bits(d2)) and np.array_equal(only_idx, idx)
    raw_nn(a, b, want_d2=False, want_idx=False)                          # neither: a no-op
    # one item of the batch into the middle row of three: the rows of its neighbours stay
    da, db = cu(a), cu(b)
    rows = torch.full((3, Na), SENT_F, device="cuda")
    irows = torch.full((3, Na), SENT_I, device="cuda", dtype=torch.int32)
    N.check(N.lib().surfd_cloud_nn(N.ptr(da[1]), N.ptr(db[1]), 1, Na, 2049, N.ptr(rows[1]), N.ptr(irows[1]), N.stream()))
    torch.cuda.synchronize()
    assert (rows[[0, 2]] == SENT_F).all() and (irows[[0, 2]] == SENT_I).all()
    assert np.array_equal(bits(rows[1]), bits(d2[1])) and np.array_equal(irows[1].cpu().numpy(), idx[1])


@pytest.mark.parametrize("M,Rr", [(700, 7), (1, 2049)])
def test_cloud_nn_matrix_writes_its_entries_and_nothing_else(M, Rr):
    from surfd_amd import _native as N
    A, B, want, count = plan_case(M, Rr, 5, 7)
    assert plan_of(M, 5, Rr)[2] > 1 and Rr % plan_of(M, 5, Rr)[2] != 0    # a ragged last range: its workgroup stops at R
    dA, dB = cu(A), cu(B)
    for with_below in (True, False):
        mean = torch.full((PAD + M * Rr + PAD,), SENT_F, device="cuda")
        below = torch.full((PAD + M * Rr + PAD,), SENT_I, device="cuda", dtype=torch.int32)
        N.check(N.lib().surfd_cloud_nn_matrix(N.ptr(dA), M, 5, N.ptr(dB), Rr, 7, PLAN_TAU2, N.ptr(mean[PAD:]),
                                              N.ptr(below[PAD:]) if with_below else None, N.stream()))
        torch.cuda.synchronize()
        for buf, sent in ((mean, SENT_F), (below, SENT_I)):
            assert (buf[:PAD] == sent).all() and (buf[PAD + M * Rr:] == sent).all(), "written outside [M, R]"
        assert np.array_equal(bits(mean[PAD:PAD + M * Rr]).reshape(M, Rr), bits(want))
        if with_below:
            assert np.array_equal(below[PAD:PAD + M * Rr].reshape(M, Rr).cpu().numpy(), count)
        else:
            assert (below == SENT_I).all()


# ---- 18. the stated order where it decides the bits; stability -------------------------------------------------------------------------
def test_wave_sums_are_added_in_the_stated_order(CM):
    a, b, want, exact = R.wave_order_case()
    assert want != exact
    mean, _ = CM.directed_means(cu(a[None]), cu(b[None]))
    assert float(mean) == float(want), f"{float(mean)!r}: the exact sum and any order that adds w2 + w3 first give {float(exact)!r}"
    d2, _ = CM.nearest_neighbors(cu(a[None]), cu(b[None]))
    assert np.array_equal(bits(d2)[0], bits(R.nn_f32(a, b)[0]))


@pytest.mark.parametrize("M,Rr,Na,Nb", [c for c in PLAN_CASES if c[:2] != (5, 7)])
def test_repeated_calls_of_a_plan_with_several_clouds_per_workgroup(CM, M, Rr, Na, Nb):
    A, B, want, count = plan_case(M, Rr, Na, Nb)
    dA, dB = cu(A), cu(B)
    outs = set()
    for _ in range(STABILITY_REPEATS):
        mean, below = CM.directed_means(dA, dB, tau2=PLAN_TAU2)
        outs.add((mean.cpu().numpy().tobytes(), below.cpu().numpy().tobytes()))
    assert outs == {(want.tobytes(), count.astype(np.int32).tobytes())}


def test_repeated_calls_across_three_candidate_tiles(CM):
    a, b = cu(R.random_cloud(3, 300, 303)), cu(R.lattice_cloud(3, 6145, 7 * 6145 + 4))
    outs = set()
    for _ in range(STABILITY_REPEATS):
        d2, idx = CM.nearest_neighbors(a, b)
        outs.add((d2.cpu().numpy().tobytes(), idx.cpu().numpy().tobytes()))
    assert len(outs) == 1
