"""GPU tests of the point-cloud normals (surfd_amd/cloudnormals.py, csrc/cloudnormals.hip) against tests/normals_ref.py, the numpy
restatement of the kernel's contract (fp32 pair arithmetic, (d2, index) selection, fp64 moments in rank order, six Jacobi
sweeps in fp64 from + - * / sqrt alone).  Every step is either a selection or one IEEE rounding, so the requirement everywhere
is equality: ``normals`` and ``eigenvalues`` bit-equal and ``knn_idx`` equal for 100 % of the points, no tolerance, no excluded
case, exact ties and duplicated points included.

  1  equality with the restatement: K in {3, 8, 16, 32, 33, 64} x the sizes of SIZES x {random, torus, lattice}, and a cloud
     with 5 copies of every point, and planar clouds
  2  batch independence: a cloud alone, first and last in batches of 1, 3 and 520
  3  ragged batches whose padding is NaN and 1e30 and is never read
  4  bit stability over 10 repeats
  5  the refusals that need a device
  6  the viewpoint flip
  7  the glue: cloudmetrics.normal_consistency on hand-checkable inputs and against numpy, examples/reconstruct.py's
     normal_consistency_16, examples/evaluate.py --paired --normal_consistency, and the default run against the parent
     commit's JSON (tests/golden/)
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
import normals_ref as NR  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g20_evaluate_paired_default.json")
KS = (3, 8, 16, 32, 33, 64)                 # 32 | 33: 256 | 128 lanes per workgroup
FAMILIES = ("random", "torus", "lattice")
STABILITY_REPEATS = 10
# the issue's list (K and K + 1 are added per K), then one size on each side of every boundary of csrc/cloudnormals.hip
SIZES = (63, 64, 65, 255, 256, 257, 777, 2048, 5000,
         127, 128, 129,                     # one | two workgroups of 128 lanes (K > 32); 255, 256, 257 are that of 256 lanes
         512,                               # the whole 8^3 lattice
         1023, 1024, 1025)                  # one | two LDS tiles of candidates


def cu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


@pytest.fixture(scope="module")
def CNM():
    from surfd_amd import cloudnormals
    return cloudnormals


_CASES = {}


def case(family, n):
    """(cloud, its min(64, n) nearest keys per point): computed once per (family, size), shared by every K"""
    if (family, n) not in _CASES:
        x = NR.case_cloud(family, n)
        _CASES[family, n] = (x, NR.knn_keys(x, min(64, n)))
    return _CASES[family, n]


def run(CNM, x, K, **kw):
    """x [B, N, 3] numpy -> (normals, eigenvalues, idx) as numpy"""
    nrm, ev, idx = CNM.estimate_normals(cu(x), K, return_neighbors=True, **kw)
    torch.cuda.synchronize()
    assert nrm.dtype == torch.float32 and ev.dtype == torch.float32 and idx.dtype == torch.int64
    assert nrm.shape == ev.shape == x.shape and idx.shape == x.shape[:2] + (K,)
    return nrm.cpu().numpy(), ev.cpu().numpy(), idx.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def assert_same(got, want, what=""):
    (gn, ge, gi), (wn, we, wi) = got, want
    same_n, same_e, same_i = (bits(gn) == bits(wn)).all(-1), (bits(ge) == bits(we)).all(-1), (gi == wi).all(-1)
    print(f"{what}: normals bit-equal {same_n.mean():.6f}, eigenvalues bit-equal {same_e.mean():.6f}, idx equal {same_i.mean():.6f} "
          f"of {same_n.size} points")
    assert same_i.all(), (what, np.argwhere(~same_i)[:4])
    assert same_e.all(), (what, np.argwhere(~same_e)[:4])
    assert same_n.all(), (what, np.argwhere(~same_n)[:4])


# ---- 1. equality with the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("K", KS)
def test_equals_the_restatement(CNM, family, K):
    for n in sorted(set((K, K + 1) + tuple(s for s in SIZES if s >= K))):
        x, keys = case(family, n)
        want = NR.normals_f64ops(x, K, keys=keys)
        got = run(CNM, x[None], K)
        assert_same(tuple(g[0] for g in got), want, f"{family} N = {n} K = {K}")
        # the [N, 3] form and the call without neighbours are the same computation
        if n == 257:
            nrm, ev = CNM.estimate_normals(cu(x), K)
            assert nrm.shape == (n, 3) and torch.equal(nrm.cpu(), torch.from_numpy(got[0][0])) and torch.equal(ev.cpu(), torch.from_numpy(got[1][0]))


def test_lattice_ties_are_exercised():
    """the whole 8^3 lattice at K = 8: for all but its 8 corners (98.4 %) the 8-th and the 9-th candidate lie at the same
    distance, so the neighbourhood is decided by the index; the subsets of a lattice the other sizes use keep many such ties"""
    assert NR.boundary_ties(case("lattice", 512)[0], 8) >= 0.98
    assert NR.boundary_ties(case("lattice", 2048)[0], 8) >= 0.25


@pytest.mark.parametrize("K", (3, 8, 33, 64))
def test_five_copies_of_every_point(CNM, K):
    """every neighbourhood starts with five candidates at d2 = 0, ordered by index; at K = 3 every covariance is exactly zero"""
    x = NR.copies_cloud(200, 5, seed=3)
    want = NR.normals_f64ops(x, K)
    if K == 3:
        assert (want[1] == 0).all() and (want[0] == np.array([1, 0, 0], np.float32)).all()
    assert_same(tuple(g[0] for g in run(CNM, x[None], K)), want, f"5 copies, K = {K}")


def test_planar_clouds(CNM):
    """a flat 12 x 12 grid in a coordinate plane: every moment across the plane is exactly 0, so the covariance is zero in one
    row and column, two of the three rotations of a sweep are skipped (a_pq == 0), lambda_0 is exactly 0 and the normal exactly
    the plane's axis with the sign rule's +; one grid per axis, and one shifted off the origin"""
    g = np.arange(12, dtype=np.float32) / 8
    u, v = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    for axis in range(3):
        for offset in (0.0, 0.375):
            x = np.full((144, 3), offset, np.float32)
            x[:, (axis + 1) % 3], x[:, (axis + 2) % 3] = u, v
            want = NR.normals_f64ops(x, 9)
            assert (want[0] == np.eye(3, dtype=np.float32)[axis]).all() and (want[1][:, 0] == 0).all() and (want[1][:, 1] > 0).all()
            assert_same(tuple(t[0] for t in run(CNM, x[None], 9)), want, f"plane across axis {axis} at {offset}")


# ---- 2. batch independence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (16, 33))
def test_batch_independence(CNM, K):
    n = 300
    c = NR.case_cloud("torus", n)
    want = NR.normals_f64ops(c, K)
    alone = tuple(g[0] for g in run(CNM, c[None], K))
    assert_same(alone, want, "alone")
    for B in (3, 520):
        x = R.random_cloud(B, n, 40 + B)
        for pos in (0, B - 1):
            y = x.copy()
            y[pos] = c
            got = run(CNM, y, K)
            assert_same(tuple(g[pos] for g in got), alone, f"position {pos} of {B}")


# ---- 3. ragged ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,lengths", [(16, (777, 16, 300, 257)), (64, (777, 64, 129, 128)), (8, (8, 1025, 1024, 9))])
def test_ragged_batches_never_read_their_padding(CNM, K, lengths):
    N = max(lengths)
    x = np.stack([NR.make_cloud(f, N, 60 + b) for b, f in enumerate(("random", "torus", "lattice", "random"))])
    for b, n in enumerate(lengths):
        x[b, n:] = np.nan if b % 2 else 1e30                  # would enter every neighbourhood / poison every moment if read
    want = NR.normals_batch(x, K, lengths=lengths)
    got = run(CNM, x, K, lengths=torch.tensor(lengths))
    assert_same(got, want, f"ragged K = {K}")
    for b, n in enumerate(lengths):
        assert (got[0][b, n:] == 0).all() and (got[1][b, n:] == 0).all() and (got[2][b, n:] == -1).all()
        assert (got[2][b, :n] >= 0).all() and (got[2][b, :n] < n).all()
        alone = run(CNM, x[b:b + 1, :n], K)
        assert_same(tuple(g[0] for g in alone), tuple(g[b, :n] for g in got), f"cloud {b} alone")
    again = run(CNM, x, K, lengths=torch.tensor(lengths, dtype=torch.int32).cuda())
    assert_same(again, got, "int32 cuda lengths")


# ---- 4. bit stability ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K", [(3, 2048, 16), (2, 777, 64), (520, 300, 8)])
def test_bit_stability(CNM, B, N, K):
    """(520, 300, 8): 1 040 workgroups, several on every CU at once"""
    x = np.concatenate([R.random_cloud(B - B // 2, N, 13), R.lattice_cloud(B // 2, N, 14)])
    xd = cu(x)
    first = None
    for r in range(STABILITY_REPEATS):
        out = CNM.estimate_normals(xd, K, return_neighbors=True)
        if first is None:
            first = tuple(t.clone() for t in out)
        else:
            assert torch.equal(out[0].view(torch.int32), first[0].view(torch.int32)), f"repeat {r}"
            assert torch.equal(out[1].view(torch.int32), first[1].view(torch.int32)) and torch.equal(out[2], first[2]), f"repeat {r}"
    rows = [0, 259, 519] if B == 520 else list(range(B))
    got = tuple(t[rows].cpu().numpy() for t in first)
    assert_same(got, NR.normals_batch(x[rows], K), f"first of {STABILITY_REPEATS} repeats, rows {rows}")


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_gpu(CNM):
    x = cu(R.random_cloud(2, 64, 1))
    for bad in (2, 65, 0, -3):
        with pytest.raises(ValueError, match=r"k must lie in 3 \.\. 64"):
            CNM.estimate_normals(x, bad)
    with pytest.raises(ValueError, match="exceeds the 16 points"):
        CNM.estimate_normals(x[:, :16].contiguous(), 17)
    with pytest.raises(ValueError, match="lengths must lie in"):
        CNM.estimate_normals(x, 8, lengths=torch.tensor([64, 65]))
    with pytest.raises(ValueError, match="lengths must lie in"):
        CNM.estimate_normals(x, 8, lengths=torch.tensor([7, 64]).cuda())
    bad = x.clone()
    bad[1, 40, 2] = float("nan")
    with pytest.raises(ValueError, match="NaN or Inf"):
        CNM.estimate_normals(bad, 8)
    bad[1, 40, 2] = float("inf")
    with pytest.raises(ValueError, match="NaN or Inf"):
        CNM.estimate_normals(bad, 8)
    CNM.estimate_normals(bad, 8, lengths=torch.tensor([64, 40]))         # the Inf is padding now
    with pytest.raises(ValueError, match="viewpoint contains NaN or Inf"):
        CNM.estimate_normals(x, 8, viewpoint=torch.tensor([0.0, float("nan"), 0.0]))
    nrm, ev, idx = CNM.estimate_normals(x[:0], 8, return_neighbors=True)   # B = 0
    assert nrm.shape == (0, 64, 3) and ev.shape == (0, 64, 3) and idx.shape == (0, 64, 8)
    from surfd_amd import cloudmetrics as CM
    with pytest.raises(ValueError, match="na must have the shape of its cloud"):
        CM.normal_consistency(x, x[:, :10], x, x)
    with pytest.raises(ValueError, match="nb must be a floating-point tensor"):
        CM.normal_consistency(x, x, x, x.long())
    with pytest.raises(ValueError, match="na is on cpu"):
        CM.normal_consistency(x, x.cpu(), x, x)


# ---- 6. viewpoint -------------------------------------------------------------------------------------------------------------------
def test_viewpoint_flip(CNM):
    """a sphere seen from its centre: every normal points inward by the stated dot, ((n_x v_x + n_y v_y) + n_z v_z) >= 0 with
    v = viewpoint - p in fp32, and is the unflipped normal or its negation; seen from far outside along +x, the near half
    points outward"""
    x = np.stack([NR.sphere_cloud(1000, 1), NR.sphere_cloud(1000, 2)])
    plain, ev0, _ = run(CNM, x, 16)
    centre = torch.zeros(3)
    nrm, ev, _ = run(CNM, x, 16, viewpoint=centre)
    v = np.float32(0) - x

    def dots(n, v):
        return (n[..., 0] * v[..., 0] + n[..., 1] * v[..., 1]) + n[..., 2] * v[..., 2]
    assert dots(nrm, v).dtype == np.float32 and (dots(nrm, v) >= 0).all()
    assert (dots(nrm.astype(np.float64), x.astype(np.float64)) < -0.9).all()          # inward for real, not by a rounding
    flipped = dots(plain, v) < 0
    assert 0.2 < flipped.mean() < 0.8
    assert (bits(nrm) == bits(np.where(flipped[..., None], -plain, plain))).all() and (bits(ev) == bits(ev0)).all()
    # one viewpoint per cloud, on the GPU, and a ragged batch: the padding rows stay zero
    vp = torch.tensor([[0.0, 0, 0], [100.0, 0, 0]])
    lengths = torch.tensor([1000, 600])
    y = x.copy()
    y[1, 600:] = np.nan
    nrm2, _, _ = run(CNM, y, 16, viewpoint=vp.cuda(), lengths=lengths)
    assert (bits(nrm2[0]) == bits(nrm[0])).all()
    v1 = vp[1].numpy() - y[1, :600]
    assert (dots(nrm2[1, :600], v1) >= 0).all() and (nrm2[1, 600:] == 0).all()
    assert (nrm2[1, :600, 0] > 0).mean() > 0.9                                     # towards +x nearly everywhere


# ---- 7. the glue ----------------------------------------------------------------------------------------------------------------------
def test_normal_consistency_on_hand_inputs():
    from surfd_amd import cloudmetrics as CM
    a = cu(R.random_cloud(2, 500, 21))
    n = torch.nn.functional.normalize(torch.randn(2, 500, 3, generator=torch.Generator().manual_seed(1)), dim=-1).cuda()
    # two copies of a cloud with its normals: exactly 1, oriented or not, whatever the normals' lengths
    for normals in (n, 3 * n, n.double()):
        for oriented in (False, True):
            out = CM.normal_consistency(a, normals, a.clone(), normals.clone(), oriented=oriented)
            assert all(out[k].dtype == torch.float64 and out[k].shape == (2,) for k in ("nc_ab", "nc_ba", "nc"))
            assert all(out[k].tolist() == [1.0, 1.0] for k in ("nc_ab", "nc_ba", "nc")), out
    # a cloud against itself with the normals rotated by 60 degrees about an axis perpendicular to them: 0.5
    z = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(2, 500, 3).cuda()
    r60 = torch.tensor([np.sqrt(3) / 2, 0.0, 0.5], dtype=torch.float64).expand(2, 500, 3).cuda()
    r120 = torch.tensor([np.sqrt(3) / 2, 0.0, -0.5], dtype=torch.float64).expand(2, 500, 3).cuda()
    out = CM.normal_consistency(a, z, a, r60)
    assert all(abs(v - 0.5) <= 1e-15 for k in ("nc_ab", "nc_ba", "nc") for v in out[k].tolist()), out
    assert all(abs(v - 0.5) <= 1e-15 for v in CM.normal_consistency(a, z, a, r120)["nc"].tolist())
    assert all(abs(v + 0.5) <= 1e-15 for v in CM.normal_consistency(a, z, a, r120, oriented=True)["nc"].tolist())
    # a zero vector scores 0: half of b's normals zeroed
    half = n.clone()
    half[:, ::2] = 0
    out = CM.normal_consistency(a, n, a, half)
    assert out["nc_ab"].tolist() == [0.5, 0.5] and out["nc_ba"].tolist() == [0.5, 0.5]


def test_normal_consistency_through_the_gpu(CNM):
    """sphere against the same sphere: 1 exactly.  Sphere against a noisy sphere: within 1e-12 of the value numpy computes from
    the restatement's normals and cloud_ref's nearest neighbours (the normals and the neighbours are the same bits; what is left
    is the order of two fp64 sums of 2 048 terms of magnitude <= 1, bounded by 2 048 2^-53 = 2.3e-13)."""
    from surfd_amd import cloudmetrics as CM
    K = 16
    a = NR.sphere_cloud(2048, 5)
    g = np.random.default_rng(6)
    b = (NR.sphere_cloud(2048, 7).astype(np.float64) * (1 + 0.02 * g.standard_normal((2048, 1)))).astype(np.float32)
    ad, bd = cu(a[None]), cu(b[None])
    na, nb = CNM.estimate_normals(ad, K)[0], CNM.estimate_normals(bd, K)[0]
    same = CM.normal_consistency(ad, na, ad.clone(), na.clone())
    assert same["nc"].tolist() == [1.0] and same["nc_ab"].tolist() == [1.0] and same["nc_ba"].tolist() == [1.0]
    ra, rb = NR.normals_f64ops(a, K)[0], NR.normals_f64ops(b, K)[0]
    assert (bits(na[0].cpu().numpy()) == bits(ra)).all() and (bits(nb[0].cpu().numpy()) == bits(rb)).all()
    for oriented in (False, True):
        got = CM.normal_consistency(ad, na, bd, nb, oriented=oriented)
        want = NR.normal_consistency_f64(a, ra, b, rb, oriented=oriented)
        print(f"oriented {oriented}: nc_ab {float(got['nc_ab']):.15f} / {want[0]:.15f}, nc_ba {float(got['nc_ba']):.15f} / {want[1]:.15f}")
        for k, w in zip(("nc_ab", "nc_ba", "nc"), want):
            assert abs(float(got[k]) - w) <= 1e-12, (k, float(got[k]), w)
    assert 0.9 < float(CM.normal_consistency(ad, na, bd, nb)["nc"]) < 1


def test_reconstruct_metrics_normal_consistency_16(tmp_path):
    """examples/reconstruct.py's item_metrics on a box against itself: both sides draw 16 384 different surface points with face
    normals.  A point's nearest neighbour lies on another face (score 0: the faces are perpendicular) only within about the
    sample spacing of an edge, sqrt(area / 16 384) = 0.012 here, along 8.8 of edge length on an area of 2.32: about 5 % of the
    points at most.  Asserted: above 0.9, at most 1."""
    import voxel_ref as X
    from examples.reconstruct import item_metrics
    h = np.array([0.3, 0.5, 0.4])
    v, t = X.box_mesh(-h, h)
    path = str(tmp_path / "box.npz")
    np.savez(path, vertices=np.asarray(v, np.float32), triangles=np.asarray(t, np.int64))
    m = item_metrics(path, np.asarray(v, np.float32), np.asarray(t, np.int64), None, 0)
    print(m)
    assert 0.9 < m["normal_consistency_16"] <= 1
    assert m["voxel_iou_surface_64"] == 1.0 and m["mesh_distance"] < 1e-6
    assert m == item_metrics(path, np.asarray(v, np.float32), np.asarray(t, np.int64), None, 0)     # a function of the seed


def test_evaluate_driver_normal_consistency(tmp_path):
    from test_gpu_cloudsample import EVAL_ARGS, make_eval_inputs     # the inputs and the command the golden JSON was written with
    gen_dir, ref_dir = make_eval_inputs(str(tmp_path))
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, os.path.join(ROOT, "examples", "evaluate.py"), "--generated", gen_dir, "--reference", ref_dir] + EVAL_ARGS

    def call(extra, name):
        r = subprocess.run(base + extra + ["--output", str(tmp_path / name)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.load(open(tmp_path / name)), open(tmp_path / name, "rb").read()

    nc, _ = call(["--normal_consistency", "--normals_k", "12"], "nc.json")
    assert nc["options"]["normal_consistency"] is True and nc["options"]["normals_k"] == 12
    assert list(nc["items"]) == ["item0", "item1", "item2"]
    values = [it["normal_consistency"] for it in nc["items"].values()]
    # item0 / item1: a box against the same box stretched along y, face against face after the normalisation; item2: two tori about
    # DIFFERENT axes (cloud_ref.torus_cloud rolls the coordinates by seed % 3), whose normals have little to do with each other
    assert all(0 <= v <= 1 for v in values) and min(values[:2]) > values[2], values
    assert nc["mean"]["normal_consistency"] == float(np.mean(values, dtype=np.float64))
    default, raw = call([], "default.json")
    # without the flag: the parent commit's output, and everything but the new keys is that output with the flag too
    golden = json.load(open(GOLDEN))
    assert default == golden and raw == json.dumps(golden, indent=1).encode()
    assert "normal_consistency" not in default["options"] and "normal_consistency" not in default["mean"]
    for it in nc["items"].values():
        it.pop("normal_consistency")
    nc["mean"].pop("normal_consistency")
    nc["options"].pop("normal_consistency"), nc["options"].pop("normals_k")
    assert nc == golden
    r = subprocess.run(base[:-len(EVAL_ARGS)] + ["--normal_consistency", "--output", str(tmp_path / "x.json")], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode != 0 and "--paired" in r.stderr
