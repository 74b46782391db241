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
"""
import json
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
