"""GPU tests of the farthest point sampling (surfd_amd/cloudsample.py, csrc/cloudfps.hip) against tests/fps_ref.py, the numpy
fp32 restatement of the loop.  The minimum and the maximum of the loop only select, so the requirement everywhere is equality:
``idx`` equal and ``cover2`` bit-equal for 100 % of the entries, no tolerance, no excluded case, exact ties and duplicated
points (lattice_cloud) included.

  1  equality with the restatement on random and lattice clouds, B in {1, 3}, the sizes of the issue and one size on each side
     of every boundary the implementation has (SIZES below names them), and a 100 000-point torus cloud -> 2 048
  2  per-cloud start indices; a row of a batch equals the call on that cloud alone
  3  ragged clouds with padding that would win every arg-max if it were read
  4  cover2 against an independent kernel (cloudmetrics.nearest_neighbors), and monotone
  5  bit stability over 40 repeats, including a batch that puts several workgroups on a CU
  6  meshprep.sample_points_evenly: on the surface, and a smaller covering radius than the uniform sample of the same seed
  7  examples/evaluate.py --paired --sampling even, and the default run against the parent commit's JSON (tests/golden/)
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
import fps_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STABILITY_REPEATS = 40                      # as tests/test_gpu_dgcnn.py
ON_SURFACE_TOL = 4 * 1.380e-07              # the bound of tests/test_gpu_meshprep.py::test_sampler (its TOL)
GOLDEN = os.path.join(ROOT, "tests", "golden", "g20_evaluate_paired_default.json")

# (N, K): the issue's list, then one size on each side of every boundary of csrc/cloudfps.hip
SIZES = [(1, 1), (2, 2), (63, 63),
         (64, 64), (65, 65),                # resident <1, 64> | <1, 256> (one wave | four waves)
         (777, 777),
         (1024, 100), (1025, 100),          # resident <4, 256> | <8, 256> (P 4 | 8)
         (2048, 512),
         (8192, 256), (8193, 256),          # resident <8, 1024> | streamed tier
         (20000, 128),
         (256, 64), (257, 64),              # resident <1, 256> | <2, 256> (P 1 | 2)
         (512, 64), (513, 64),              # resident <2, 256> | <4, 256> (P 2 | 4)
         (2049, 64),                        # resident <8, 256> | <16, 256> (P 8 | 16; 2 048 is above)
         (4096, 64), (4097, 64),            # resident <16, 256> | <8, 1024> (workgroup size 256 | 1 024)
         (32768, 48), (32769, 48)]          # streamed: every running minimum in LDS | the last ones in the workspace


def cu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


@pytest.fixture(scope="module")
def CS():
    from surfd_amd import cloudsample
    return cloudsample


def run(CS, x, K, **kw):
    idx, cover2 = CS.farthest_point_sampling(cu(x), K, **kw)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int64 and cover2.dtype == torch.float32 and idx.shape == cover2.shape == (len(x), K)
    return idx.cpu().numpy(), cover2.cpu().numpy()


def assert_same(got, want, what=""):
    (gi, gc), (wi, wc) = got, want
    same_i, same_c = gi == wi, gc.view(np.int32) == np.ascontiguousarray(wc, np.float32).view(np.int32)
    print(f"{what}: idx equal {same_i.mean():.6f}, cover2 bit-equal {same_c.mean():.6f} of {gi.size} entries")
    assert same_i.all(), (what, np.argwhere(~same_i)[:4])
    assert same_c.all(), (what, np.argwhere(~same_c)[:4])


# ---- 1. equality with the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["random", "lattice"])
@pytest.mark.parametrize("N,K", SIZES)
def test_equals_the_restatement(CS, family, N, K):
    make = {"random": R.random_cloud, "lattice": R.lattice_cloud}[family]
    for B in (1, 3):
        x = make(B, N, 100 + N + B)
        if family == "lattice" and N >= 64:
            assert len(np.unique(x[0], axis=0)) < N                      # duplicated points are in
        assert_same(run(CS, x, K), F.fps_batch(x, K), f"{family} B = {B} N = {N} K = {K}")


@pytest.fixture(scope="module")
def torus_100k():
    x = R.family("torus", 1, 100000)
    return x, F.fps_batch(x, 2048)


def test_torus_100000_to_2048(CS, torus_100k):
    x, want = torus_100k
    assert_same(run(CS, x, 2048), want, "torus 100 000 -> 2 048")


def test_lattice_ties_are_exercised():
    """the lattice clouds decide arg-maxima by the index: exact ties of the two best minima in the yardstick's own run"""
    for N, K in ((64, 64), (2048, 512)):
        gaps = F.decisions(R.lattice_cloud(1, N, 100 + N + 1)[0], K, np.float32)
        assert (gaps == 0).sum() >= K // 4, (N, int((gaps == 0).sum()))


# ---- 2. start index and batch independence -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(777, 64), (2048, 64), (9000, 32)])
def test_start_indices_and_batch_independence(CS, N, K):
    B = 5
    x = np.concatenate([R.random_cloud(3, N, 5), R.lattice_cloud(2, N, 6)])
    start = np.array([0, N - 1, N // 2, 17, N - 2][:B], np.int64)
    got = run(CS, x, K, start_index=torch.from_numpy(start))
    assert_same(got, F.fps_batch(x, K, start=start), f"starts {start.tolist()}")
    assert (got[0][:, 0] == start).all()
    for b in range(B):
        alone = run(CS, x[b:b + 1], K, start_index=int(start[b]))
        assert_same(alone, (got[0][b:b + 1], got[1][b:b + 1]), f"row {b} alone")
    # an int32 tensor on the GPU, and the int form
    again = run(CS, x, K, start_index=torch.from_numpy(start).int().cuda())
    assert_same(again, got, "int32 cuda starts")
    assert_same(run(CS, x, K, start_index=3), F.fps_batch(x, K, start=[3] * B), "start_index = 3")


# ---- 3. ragged --------------------------------------------------------------------------------------------------------------------
def test_ragged_clouds_never_read_their_padding(CS):
    N, K = 2048, 100
    lengths = np.array([N, 1, 777, 64], np.int64)
    x = np.concatenate([R.random_cloud(2, N, 8), R.lattice_cloud(2, N, 9)])
    for b, n in enumerate(lengths):
        x[b, n:] = 1e30                                                   # would win every arg-max if read
    want = F.fps_batch(x, K, lengths=lengths)
    assert (want[0][1, 1:] == -1).all() and (want[1][1] == 0).all() and (want[0][3, 64:] == -1).all() and (want[0][2] >= 0).all()
    got = run(CS, x, K, lengths=torch.from_numpy(lengths))
    assert_same(got, want, "ragged")
    assert float(got[1].max()) < 100
    assert_same(run(CS, x, K, lengths=torch.from_numpy(lengths).int().cuda(), start_index=torch.tensor([5, 0, 776, 63])),
                F.fps_batch(x, K, lengths=lengths, start=[5, 0, 776, 63]), "ragged with starts")
    # padding may hold anything, NaN included: it is neither checked nor read
    y = x.copy()
    y[2, 777:] = np.nan
    assert_same(run(CS, y, K, lengths=torch.from_numpy(lengths)), want, "NaN padding")
    # the streamed tier
    N, K = 9000, 40
    lengths = np.array([9000, 8500, 3], np.int64)
    x = R.random_cloud(3, N, 10)
    for b, n in enumerate(lengths):
        x[b, n:] = 1e30
    assert_same(run(CS, x, K, lengths=torch.from_numpy(lengths)), F.fps_batch(x, K, lengths=lengths), "ragged, streamed")
    # pytorch3d's call shape: points gathered, rows beyond a cloud's length zero-filled
    pts, idx = CS.sample_farthest_points(cu(x), K, lengths=torch.from_numpy(lengths))
    assert pts.shape == (3, K, 3) and torch.equal(idx.cpu(), torch.from_numpy(F.fps_batch(x, K, lengths=lengths)[0]))
    assert torch.equal(pts[2, 3:].cpu(), torch.zeros(K - 3, 3)) and torch.equal(pts[0].cpu(), torch.from_numpy(x[0])[idx[0].cpu()])
    g = torch.Generator().manual_seed(4)
    pts, idx = CS.sample_farthest_points(cu(x), K, lengths=torch.from_numpy(lengths), random_start_point=True, generator=g)
    draw = torch.randint(0, 2 ** 31 - 1, (3,), generator=torch.Generator().manual_seed(4)).numpy() % lengths
    assert idx[:, 0].cpu().tolist() == draw.tolist()
    assert torch.equal(idx.cpu(), torch.from_numpy(F.fps_batch(x, K, lengths=lengths, start=draw)[0]))


def test_refusals_on_the_gpu(CS):
    x = cu(R.random_cloud(2, 64, 1))
    with pytest.raises(ValueError, match="K must be at least 1"):
        CS.farthest_point_sampling(x, 0)
    with pytest.raises(ValueError, match="lengths must lie in"):
        CS.farthest_point_sampling(x, 4, lengths=torch.tensor([64, 65]))
    with pytest.raises(ValueError, match="lengths must lie in"):
        CS.farthest_point_sampling(x, 4, lengths=torch.tensor([0, 3]).cuda())
    with pytest.raises(ValueError, match="start_index must lie in"):
        CS.farthest_point_sampling(x, 4, start_index=64)
    with pytest.raises(ValueError, match="start_index must lie in"):
        CS.farthest_point_sampling(x, 4, lengths=torch.tensor([64, 10]), start_index=torch.tensor([63, 10]))
    bad = x.clone()
    bad[1, 5, 2] = float("nan")
    with pytest.raises(ValueError, match="NaN or Inf"):
        CS.farthest_point_sampling(bad, 4)
    CS.farthest_point_sampling(bad, 4, lengths=torch.tensor([64, 5]))    # the NaN is padding now
    idx, cover2 = CS.farthest_point_sampling(x[:0], 4)                   # B = 0
    assert idx.shape == (0, 4) and cover2.shape == (0, 4)


# ---- 4. an independent kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K", [(3, 2048, 512), (2, 20000, 128), (2, 1000, 1000)])
def test_cover2_against_nearest_neighbors(CS, B, N, K):
    from surfd_amd import cloudmetrics as CM
    x = cu(np.concatenate([R.random_cloud(B - 1, N, 11), R.lattice_cloud(1, N, 12)]))
    idx, cover2 = CS.farthest_point_sampling(x, K)
    picked = torch.gather(x, 1, idx[:, :, None].expand(-1, -1, 3)).contiguous()
    d2, _ = CM.nearest_neighbors(x, picked)
    assert torch.equal(cover2[:, K - 1].view(torch.int32), d2.max(1).values.view(torch.int32))
    assert bool((cover2[:, 1:] <= cover2[:, :-1]).all())
    if K == N:
        assert bool((cover2[:, -1] == 0).all())


# ---- 5. bit stability ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K", [(3, 2048, 512), (2, 20000, 128), (520, 1000, 64)])
def test_bit_stability(CS, B, N, K):
    """(520, 1000, 64): 256-lane workgroups, several on every CU at once"""
    x = np.concatenate([R.random_cloud(B - B // 2, N, 13), R.lattice_cloud(B // 2, N, 14)])
    xd = cu(x)
    first = None
    for r in range(STABILITY_REPEATS):
        idx, cover2 = CS.farthest_point_sampling(xd, K)
        if first is None:
            first = (idx.clone(), cover2.clone())
        else:
            assert torch.equal(idx, first[0]) and torch.equal(cover2.view(torch.int32), first[1].view(torch.int32)), f"repeat {r}"
    rows = [0, 259, 519] if B == 520 else list(range(B))
    got = (first[0][rows].cpu().numpy(), first[1][rows].cpu().numpy())
    assert_same(got, F.fps_batch(x[rows], K), f"first of {STABILITY_REPEATS} repeats, rows {rows}")


# ---- 6. even surface clouds -----------------------------------------------------------------------------------------------------------
def torus_mesh(nu=96, nv=48, R0=0.6, r0=0.25):
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    p = np.stack(((R0 + r0 * np.cos(v)) * np.cos(u), (R0 + r0 * np.cos(v)) * np.sin(u), r0 * np.sin(v)), -1).reshape(-1, 3)
    n = np.arange(nu * nv).reshape(nu, nv)
    a, b, c, d = n, np.roll(n, -1, 0), np.roll(np.roll(n, -1, 0), -1, 1), np.roll(n, -1, 1)
    t = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return p.astype(np.float32), t.astype(np.int64)


@pytest.mark.parametrize("shape", ["torus", "sphere"])
def test_sample_points_evenly(shape):
    """Measured with this test's own inputs on the MI355X (covering radius^2 against 100 000 uniform surface points, K = 1 024,
    init_factor 5, seeds 0, 1, 2), uniform / even: torus 2.36, 2.77, 3.24 (1.49e-2 / 6.32e-3, 2.04e-2 / 7.38e-3, 1.92e-2 /
    5.94e-3); sphere 1.97, 2.61, 3.16 (2.21e-2 / 1.12e-2, 2.19e-2 / 8.42e-3, 2.40e-2 / 7.60e-3).  The assertion stays the issue's:
    strictly smaller.  The test prints the figures."""
    import voxel_ref as X
    from surfd_amd import cloudmetrics as CM, meshprep as M
    v, t = torus_mesh() if shape == "torus" else X.icosphere(subdivisions=3)
    vd, td = cu(v), cu(t, torch.int64)
    K = 1024
    dense = M.sample_points_uniformly(vd, td, 100000, generator=torch.Generator(device="cuda").manual_seed(99))
    for seed in (0, 1, 2):
        even = M.sample_points_evenly(vd, td, K, generator=torch.Generator(device="cuda").manual_seed(seed))
        assert even.shape == (K, 3) and even.dtype == torch.float32 and even.is_cuda
        again = M.sample_points_evenly(vd, td, K, generator=torch.Generator(device="cuda").manual_seed(seed))
        assert torch.equal(even, again)
        assert float(M.point_to_mesh_distance(even, vd, td).max()) <= ON_SURFACE_TOL
        uniform = M.sample_points_uniformly(vd, td, K, generator=torch.Generator(device="cuda").manual_seed(seed))
        c_even = float(CM.nearest_neighbors(dense[None], even[None].contiguous())[0].max())
        c_uniform = float(CM.nearest_neighbors(dense[None], uniform[None].contiguous())[0].max())
        print(f"{shape} seed {seed}: covering radius^2 uniform {c_uniform:.4e}, even {c_even:.4e}, uniform / even = {c_uniform / c_even:.2f}")
        assert c_even < c_uniform
    # a CPU mesh and a CPU generator: the same candidates as sample_points_uniformly draws, the result back on the CPU
    vc, tc = torch.from_numpy(v), torch.from_numpy(t)
    even = M.sample_points_evenly(vc, tc, 64, init_factor=3, generator=torch.Generator().manual_seed(5))
    cand = M.sample_points_uniformly(vc, tc, 192, generator=torch.Generator().manual_seed(5))
    assert even.device.type == "cpu" and torch.equal(even, cand[torch.from_numpy(F.fps_f32(cand.numpy(), 64)[0])])


# ---- 7. the driver -----------------------------------------------------------------------------------------------------------------
def make_eval_inputs(root):
    """two directories of three items each: item0 / item1 as .obj boxes, item2 as an .npz cloud of 3 000 points"""
    import mesh_udf_ref as MR
    import voxel_ref as X
    gen_dir, ref_dir = os.path.join(root, "gen"), os.path.join(root, "ref")
    os.makedirs(gen_dir), os.makedirs(ref_dir)
    for k in range(2):
        for d, s in ((gen_dir, 1.0), (ref_dir, 1.1)):
            h = np.array([0.3 + 0.1 * k, 0.5 * s, 0.2 + 0.05 * k])
            MR.write_obj(os.path.join(d, f"item{k}.obj"), *X.box_mesh(-h, h))
    np.savez(os.path.join(gen_dir, "item2.npz"), pcd=R.torus_cloud(1, 3000))
    np.savez(os.path.join(ref_dir, "item2.npz"), pcd=R.torus_cloud(2, 3000))
    return gen_dir, ref_dir


EVAL_ARGS = ["--paired", "--num_points", "512", "--seed", "3", "--f_threshold", "0.05"]


def test_evaluate_driver_even_sampling(tmp_path):
    gen_dir, ref_dir = make_eval_inputs(str(tmp_path))
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, os.path.join(ROOT, "examples", "evaluate.py"), "--generated", gen_dir, "--reference", ref_dir] + EVAL_ARGS

    def call(extra, name):
        r = subprocess.run(base + extra + ["--output", str(tmp_path / name)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.load(open(tmp_path / name))

    even = call(["--sampling", "even", "--init_factor", "4"], "even.json")
    assert even["options"]["sampling"] == "even" and even["options"]["init_factor"] == 4
    assert list(even["items"]) == ["item0", "item1", "item2"] and all(0 < it["fscore"] <= 1 and it["cd"] > 0 for it in even["items"].values())
    assert even == call(["--sampling", "even", "--init_factor", "4"], "even2.json")              # reproducible for a fixed seed
    default = call([], "default.json")
    assert "sampling" not in default["options"] and default["items"] != even["items"]
    # the default run is what the parent commit wrote for the same command and inputs
    assert default == json.load(open(GOLDEN))
    assert default == call(["--sampling", "uniform"], "uniform.json")
