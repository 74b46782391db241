"""GPU tests of the point-cloud encoder (surfd_amd/dgcnn.py, csrc/dgcnn.hip; run with -m gpu on an MI355X): kNN against
exact brute force, the EdgeConv features and the latents against the reference's own Dgcnn (tests/golden/g18_dgcnn.npz,
tools/make_golden.py g18), bitwise determinism / batch independence / permutation invariance, and the reconstruction driver.

The second half pins the kernels at the shapes the fixture does not hold, against tests/dgcnn_ref.py (proven on the fixture
by tests/test_dgcnn_cpu.py): the kNN bit for bit on continuous clouds, the network by value on inputs without rounding, the
network against fp64 with general weights, and one handle across calls of different sizes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dgcnn_ref as R
from surfd_amd import synth
from surfd_amd.dgcnn import Dgcnn, knn_points

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


def _encoder(L):
    m = Dgcnn(L)
    m.load_state_dict(synth.synth_dgcnn_state_dict(L, seed=0), strict=True)
    return m.cuda().eval()


def _brute_knn(x, K):
    """stable (distance, index) order of the fp64 squared distances: (dists fp64, idx int64)"""
    x = x.double()
    ds, ids = [], []
    for q0 in range(0, x.shape[1], 1024):
        d = ((x[:, q0:q0 + 1024, None, :] - x[:, None, :, :]) ** 2).sum(-1)
        s, i = torch.sort(d, dim=-1, stable=True)
        ds.append(s[..., :K]); ids.append(i[..., :K])
    return torch.cat(ds, 1), torch.cat(ids, 1)


def _lattice_cloud(B, N, seed):
    """points on the 1/8 lattice of [-2, 2]^3 (every fp32 squared distance exact; ties everywhere) plus duplicated points"""
    g = torch.Generator().manual_seed(seed)
    side = max(3, int(round((N / 4) ** (1 / 3))))                  # a lattice small enough to hold duplicates
    p = torch.randint(-side, side + 1, (B, N, 3), generator=g).float() / 8
    dup = torch.randint(0, N, (B, N // 10), generator=g)
    p[torch.arange(B)[:, None], torch.randint(0, N, (B, N // 10), generator=g)] = p[torch.arange(B)[:, None], dup]
    return p


def _surface_cloud(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, N, 3, generator=g)
    v = v / v.norm(dim=-1, keepdim=True) * torch.tensor([0.6, 0.4, 0.5])
    return (v + torch.randn(B, N, 3, generator=g) * 0.01).float()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [20, 777, 10000])
def test_knn_exact_on_lattice(B, N):
    x = _lattice_cloud(B, N, seed=N + B)
    d, i = knn_points(x.cuda(), 20)
    rd, ri = _brute_knn(x.cuda(), 20)
    assert i.dtype == torch.int64 and d.dtype == torch.float32
    assert torch.equal(i, ri), f"{int((i != ri).sum())} indices differ"
    assert torch.equal(d.double(), rd)


@pytest.mark.parametrize("K", [1, 8, 13, 16, 24, 32])
def test_knn_other_k_exact_on_lattice(K):
    x = _lattice_cloud(2, 3000, seed=K)
    d, i = knn_points(x.cuda(), K)
    rd, ri = _brute_knn(x.cuda(), K)
    assert torch.equal(i, ri) and torch.equal(d.double(), rd)


def test_knn_fixture_clouds(golden):
    z = golden("g18_dgcnn")
    for name in ("a", "b"):
        _, i = knn_points(T(z[f"{name}__pts"])[None].cuda(), 20)
        assert np.array_equal(i[0].cpu().numpy(), z[f"{name}__knn_idx"].astype(np.int64)), name


@pytest.mark.parametrize("seed", [0, 1])
def test_knn_continuous_against_brute_force(seed):
    x = _surface_cloud(2, 10000, seed).cuda()
    d, i = knn_points(x, 20)
    rd, ri = _brute_knn(x, 21)
    kth, rkth = d[..., -1].double(), rd[..., 19]
    rel = float(((kth - rkth).abs() / rkth.clamp_min(1e-30)).max())
    assert rel <= 1e-6, rel
    # index sets agree except at near-ties of the boundary: a point in one set and not in the other is within fp32 rounding of
    # the K-th distance
    same = (i.sort(-1).values == ri[..., :20].sort(-1).values).all(-1)
    bad = (~same).nonzero()
    for b, n in bad.tolist():
        diff = set(i[b, n].tolist()) ^ set(ri[b, n, :20].tolist())
        dd = ((x[b, list(diff)].double() - x[b, n].double()) ** 2).sum(-1)
        assert float((dd - rkth[b, n]).abs().max()) <= 2e-6 * float(rkth[b, n]), (b, n)
    assert len(bad) <= 20, len(bad)


def test_edgeconv_features_against_reference(golden):
    z = golden("g18_dgcnn")
    m = _encoder(32)
    for name in ("a", "b", "c"):
        x = T(z[f"{name}__pts"])[None].cuda()
        _, x1234 = m.forward_features(x)
        got = x1234[0, T(z[f"{name}__rows"]).long().cuda()].cpu()
        ref = T(z[f"{name}__x1234"])
        for blk, (c0, c1) in enumerate(((0, 64), (64, 128), (128, 256), (256, 512)), 1):
            g, r = got[:, c0:c1], ref[:, c0:c1]
            err = float((g - r).abs().max())
            assert err <= 1e-5 * float(r.abs().max()) + 1e-6, f"cloud {name} x{blk}: max err {err:.3e} (scale {float(r.abs().max()):.3f})"


@pytest.mark.parametrize("L", [32, 64])
def test_latents_against_reference(golden, L):
    z = golden("g18_dgcnn")
    m = _encoder(L)
    for name in ("a", "b", "c"):
        x = T(z[f"{name}__pts"])[None].cuda()
        lat = m(x)[0].double().cpu()
        r64 = T(z[f"{name}__latent_L{L}_f64"])
        r32 = T(z[f"{name}__latent_L{L}_f32"]).double()
        e_gpu = float((lat - r64).abs().max())
        e_ref = float((r32 - r64).abs().max())
        bound = 2 * e_ref + 1e-5 * float(r64.abs().max())
        assert e_gpu <= bound, f"cloud {name} L={L}: GPU vs fp64 {e_gpu:.3e}, reference fp32 vs fp64 {e_ref:.3e}, bound {bound:.3e}"
        print(f"cloud {name} L={L}: GPU vs fp64 {e_gpu:.3e}, reference fp32 vs fp64 {e_ref:.3e}")


def test_latent_index_column():
    m = _encoder(32)
    x = _surface_cloud(3, 500, 5).cuda()
    li = torch.tensor([4.0, 7.0, 9.0], device="cuda")
    out = m(x, latent_index=li)
    assert out.shape == (3, 33)
    assert torch.equal(out[:, :32], m(x)) and torch.equal(out[:, 32], li)


def test_bitwise_determinism_batch_independence_and_permutation():
    m = _encoder(64)
    for seed in range(11, 21):                 # a cloud without a distance tie at the k-th neighbour (for the permutation)
        x = _surface_cloud(8, 10000, seed).cuda()
        d, _ = knn_points(x, 21)
        if bool((d[..., 19] < d[..., 20]).all()):
            break
    else:
        pytest.fail("no tie-free test cloud among seeds 11..20")
    outs = torch.stack([m(x) for _ in range(40)])
    distinct = torch.unique(outs.view(40, -1).view(torch.int32), dim=0).shape[0]
    assert distinct == 1, f"{distinct} distinct outputs over 40 encodes of B = 8"
    ref = outs[0]
    for b in range(8):
        assert torch.equal(m(x[b:b + 1])[0], ref[b]), f"cloud {b}: alone != in a batch of 8"
    # permutation of the points: no distance tie at the k-th neighbour, so the same neighbour sets
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(10000, generator=g).cuda()
    assert torch.equal(m(x[:, perm]), ref)


def _write_inputs(tmp_path):
    g = torch.Generator().manual_seed(21)
    u, v = torch.rand(6000, generator=g) * 6.2832, torch.rand(6000, generator=g) * 6.2832
    pcd = torch.stack([(0.5 + 0.2 * torch.cos(v)) * torch.cos(u), 0.2 * torch.sin(v), (0.5 + 0.2 * torch.cos(v)) * torch.sin(u)], 1)
    np.savez(tmp_path / "shape_a.npz", pcd=pcd.numpy().astype(np.float32), udfs=np.zeros(3, np.float32))
    np.save(tmp_path / "shape_b.npy", (pcd * 0.8).numpy().astype(np.float32))
    return [str(tmp_path / "shape_a.npz"), str(tmp_path / "shape_b.npy")]


def _driver(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "reconstruct.py")] + args, capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_reconstruct_driver_meshes(tmp_path):
    inputs = _write_inputs(tmp_path)
    out = tmp_path / "out"
    _driver(["--synthetic", "--resolution", "64", "--num_points_pcd", "4000", "--output_dir", str(out)] + inputs)
    for item in ("shape_a", "shape_b"):
        text = (out / f"{item}_meshudf.obj").read_text()
        assert text.count("\nv ") + text.startswith("v ") > 0 and "\nf " in text, item


def test_reconstruct_driver_latents_only(tmp_path):
    inputs = _write_inputs(tmp_path)
    out = tmp_path / "lat"
    _driver(["--synthetic", "--latents_only", "--num_points_pcd", "4000", "--output_dir", str(out)] + inputs)
    z = np.load(out / "latents.npz")
    assert sorted(z.files) == ["shape_a", "shape_b"]
    # the same draws and the same encoder, called directly
    from surfd_amd.dgcnn import random_point_sampling
    ckpt = torch.load(out / "ae_synthetic.pt", map_location="cpu")
    m = Dgcnn(32)
    m.load_state_dict(ckpt["encoder"], strict=True)
    m = m.cuda().eval()
    torch.manual_seed(10)
    a = torch.from_numpy(np.load(inputs[0])["pcd"]).cuda()
    b = torch.from_numpy(np.load(inputs[1])).cuda()
    lat_a = m(random_point_sampling(a, 4000)[None])[0]
    lat_b = m(random_point_sampling(b, 4000)[None])[0]
    assert np.array_equal(z["shape_a"], lat_a.cpu().numpy())
    assert np.array_equal(z["shape_b"], lat_b.cpu().numpy())


# ---- every shape the handle accepts, against tests/dgcnn_ref.py ------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _splits(B, N, k):
    """dg_splits of csrc/dgcnn.hip restated: the number of candidate splits per query block"""
    tiles = -(-N // 256)
    s = min(max(1, -(-1024 // (B * tiles))), 256 // k, tiles)
    span = -(-(-(-N // s)) // 256) * 256
    return -(-N // span)


# (B, N, K, S).  S by hand from dg_splits: min(ceil(1024 / (B ceil(N / 256))), 256 / K, ceil(N / 256)) splits of whole
# 256-point tiles.  N <= 256 is one tile, S = 1.  (1, 257, 17): min(512, 15, 2) = 2, the second split holds one candidate.
# (3, 513, 24): min(114, 10, 3) = 3.  (2, 1100, 21): min(103, 12, 5) = 5 and (1, 1100, 19): min(205, 13, 5) = 5, spans of
# 256, the last split holds 76.  (70, 300, 8): min(ceil(1024 / 140) = 8, 32, 2) = 2.  K = 16 and 24 are where dg_kth
# falls through to its default; 17, 19, 21, 24 run the KT = 24 templates, 16 the KT = 16 one.
KNN_SHAPES = [(1, 16, 16, 1), (2, 24, 24, 1), (1, 257, 17, 2), (3, 513, 24, 3), (2, 1100, 21, 5), (1, 1100, 19, 5), (70, 300, 8, 2)]


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), (37.0, -12.0, 5.0)], ids=["centred", "offset"])
@pytest.mark.parametrize("B,N,K,S", KNN_SHAPES)
def test_knn_bit_exact_on_continuous_clouds(B, N, K, S, offset):
    """distances bit-equal and indices equal to the separately rounded fp32 statement (a contracted or reordered distance sum
    differs in the last bit of some distance; far from the origin the differences cancel and distances tie)"""
    assert _splits(B, N, K) == S                                             # a changed split rule is to be noticed here
    x = R.surface_cloud(B, N, seed=N + K, offset=offset)
    rd, ri = R.knn_f32(x, K)
    d, i = knn_points(x.cuda(), K)
    assert d.shape == (B, N, K) and i.dtype == torch.int64
    nbad = int((_bits(d) != _bits(rd)).sum())
    assert nbad == 0, f"{nbad} of {d.numel()} distances differ in their bits"
    assert torch.equal(i.cpu(), ri), f"{int((i.cpu() != ri).sum())} indices differ"


def test_knn_identical_points():
    x = torch.tensor([0.3, -0.7, 1.1]).expand(2, 64, 3).contiguous().cuda()
    for K in (1, 16, 17, 20, 24, 32):
        d, i = knn_points(x, K)
        assert torch.equal(i.cpu(), torch.arange(K).expand(2, 64, K)), K
        assert bool((_bits(d) == 0).all()), K                                # +0, not -0


def _module(sd, L, k):
    m = Dgcnn(L, k=k)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


@pytest.mark.parametrize("k,N,B,L", R.NETWORK_SHAPES)
def test_network_exact_cases(k, N, B, L):
    """Inputs without rounding (tests/dgcnn_ref.py exact_case): whatever the order of the sums, every element of x1..x4 and of
    the latent has to equal the fp64 restatement by value.  N == k, one-row and one-candidate tails, k = 1 and 32, the
    KT = 16 / 24 lists in the forward pass, more than one column block of conv_5 and L = 1."""
    x, idx, sd, info = R.exact_case(k, N, B, L)
    # the preconditions, on the CPU before anything touches the GPU
    lat64, x64 = R.dgcnn_forward(sd, x, idx, torch.float64, fold_dtype=torch.float32)
    lat32, x32 = R.dgcnn_forward(sd, x, idx, torch.float32)
    assert torch.equal(x32.double(), x64) and torch.equal(lat32.double(), lat64)
    for i in range(1, 6):
        s, _ = R.fold_bn(sd, i, torch.float32)
        assert torch.equal(s, sd[f"bn_{i}.weight"])
        assert (i == 5 and L == 1) or (bool((s > 0).any()) and bool((s < 0).any()))
    assert info["min_act"] > 0 and float(x64.min()) > 0 and float(lat64.min()) > 0
    assert 8 * info["bound"] < 2 ** 24
    # the GPU
    m = _module(sd, L, k)
    xg = x.cuda()
    _, gi = m.knn(xg)
    assert torch.equal(gi.cpu(), idx)                                        # a lattice: the kNN is exact, ties by index
    rlat, rx = R.dgcnn_forward(sd, x, gi, torch.float64, fold_dtype=torch.float32)
    lat, x1234 = m.forward_features(xg)
    for blk, (c0, c1) in enumerate(R.X_SLICES, 1):
        got, ref = x1234[..., c0:c1].double().cpu().numpy(), rx[..., c0:c1].numpy()
        assert np.array_equal(got, ref), f"x{blk}: {int((got != ref).sum())} of {ref.size} elements differ"
    got, ref = lat.double().cpu().numpy(), rlat.numpy()
    assert np.array_equal(got, ref), f"latent: {int((got != ref).sum())} of {ref.size} elements differ"
    assert np.array_equal(m(xg).double().cpu().numpy(), ref)                 # and without the feature copy


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("k,N,B,L", R.NETWORK_SHAPES)
def test_network_against_fp64(k, N, B, L, seed):
    """General weights (both scale signs, a zero scale, the leaky branch) on jittered surface clouds: per block of x1..x4 and
    for the latent, err(GPU, fp64) <= 2 err(fp32 restatement, fp64) + 1e-5 max|fp64|, the reference evaluated with the GPU's
    own neighbours."""
    sd = synth.synth_dgcnn_state_dict(L, seed)
    m = _module(sd, L, k)
    x = R.surface_cloud(B, N, seed=31 * N + k + seed)
    _, gi = m.knn(x.cuda())
    r64, rx64 = R.dgcnn_forward(sd, x, gi, torch.float64)
    r32, rx32 = R.dgcnn_forward(sd, x, gi, torch.float32)
    lat, x1234 = m.forward_features(x.cuda())
    lat, x1234 = lat.double().cpu(), x1234.double().cpu()
    parts = [(f"x{b}", x1234[..., c0:c1], rx32[..., c0:c1].double(), rx64[..., c0:c1]) for b, (c0, c1) in enumerate(R.X_SLICES, 1)]
    parts.append(("latent", lat, r32.double(), r64))
    fails = []
    for name, g, f32, f64 in parts:
        e_gpu, e_ref = float((g - f64).abs().max()), float((f32 - f64).abs().max())
        bound = 2 * e_ref + 1e-5 * float(f64.abs().max())
        print(f"k={k} N={N} B={B} L={L} seed={seed} {name}: GPU vs fp64 {e_gpu:.3e}, fp32 restatement vs fp64 {e_ref:.3e}, "
              f"bound {bound:.3e}, ratio {e_gpu / bound:.3f}")
        if not e_gpu <= bound:
            fails.append((name, e_gpu, e_ref, bound))
    assert not fails, fails


def test_one_handle_across_sizes():
    """the arena grows and is reused, and the partial kNN lists overwrite old features: every call equals a fresh module's"""
    sd = synth.synth_dgcnn_state_dict(64, seed=0)
    m = _module(sd, 64, 20)
    shapes = [(2, 1000), (1, 20), (3, 257), (2, 1000)]
    other_n = [777, 40, 1500, 300]                                           # kNN calls through the same handle, in between
    clouds = {s: R.surface_cloud(s[0], s[1], seed=s[0] * s[1]).cuda() for s in shapes}
    outs = []
    for (B, N), n2 in zip(shapes, other_n):
        x = clouds[B, N]
        lat, x1234 = m.forward_features(x)
        y = R.surface_cloud(2, n2, seed=n2).cuda()
        d, i = m.knn(y)
        lat2 = m(x)
        fresh = _module(sd, 64, 20)
        flat, fx = fresh.forward_features(x)
        assert torch.equal(_bits(lat), _bits(flat)) and torch.equal(_bits(x1234), _bits(fx)), (B, N)
        assert torch.equal(_bits(lat2), _bits(flat)), (B, N)
        fd, fi = _module(sd, 64, 20).knn(y)
        assert torch.equal(_bits(d), _bits(fd)) and torch.equal(i, fi), (B, N, n2)
        outs.append((lat, x1234))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[3][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[3][1]))


def test_rebinds_after_weight_updates():
    """The handle's copy follows the module: a parameter written in place, a BUFFER written in place (the key has to see
    buffers) and a load_state_dict each give what a fresh module loaded with the changed state_dict gives, bit for bit."""
    def fresh(sd):
        return _module({k: v.detach().cpu().clone() for k, v in sd.items()}, 32, 20)

    x = R.surface_cloud(2, 64, seed=5).cuda()
    m = _module(synth.synth_dgcnn_state_dict(32, seed=0), 32, 20)
    y0 = m(x)
    with torch.no_grad():
        m.conv_1.weight.mul_(1.5)
    y1 = m(x)
    assert not torch.equal(y1, y0)
    assert torch.equal(y1, fresh(m.state_dict())(x))
    with torch.no_grad():
        m.bn_3.running_var.add_(0.5)
    y2 = m(x)
    assert not torch.equal(y2, y1)
    assert torch.equal(y2, fresh(m.state_dict())(x))
    m.load_state_dict(synth.synth_dgcnn_state_dict(32, seed=1), strict=True)
    y3 = m(x)
    assert not torch.equal(y3, y2)
    assert torch.equal(y3, fresh(synth.synth_dgcnn_state_dict(32, seed=1))(x))
