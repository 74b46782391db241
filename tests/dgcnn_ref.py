"""TEST INFRASTRUCTURE — plain-torch restatement of the point-cloud encoder (reference AutoEncoder/models/dgcnn.py:9-115, eval
mode, max aggregation) as functions of a state dict, in the PER-EDGE form the original uses: gather the neighbours,
concatenate (x_j - x_i, x_i), Linear, folded eval-mode BatchNorm, leaky-ReLU, max over k; four blocks, conv_5 + BN + leaky-ReLU
+ max over the points.  It is not the P / Q factorisation of csrc/dgcnn.hip and shares no code with the product path.  The
dtype is a parameter (fp32: what a plain evaluation gives; fp64: the judge) and so are the neighbour indices, so that the kNN
and the features are tested apart.  tests/test_dgcnn_cpu.py proves it on the reference-made fixture g18_dgcnn.

knn_f32 restates the self-kNN in fp32 with un-fused torch CPU element-wise ops, which is the bit-exact statement of what
dg_knn_kernel documents (diff = query - candidate; dx*dx, + dy*dy, + dz*dz, one rounding each; (distance, index) order).

exact_case builds points and a state dict for which every fp32 operation of the network is exact, so that the answer does not
depend on the order of any sum and the GPU has to equal the fp64 restatement by value.  No GPU, never imported by the product."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch
from torch import Tensor

F32, F64 = torch.float32, torch.float64
CH = (64, 64, 128, 256)                                    # output channels of blocks 1-4
X_SLICES = ((0, 64), (64, 128), (128, 256), (256, 512))    # where x1..x4 lie in their concatenation
SLOPE = 0.2
EPS = 1e-5
# (k, N, B, L) of the network cases: N == k; N < 64 (one row tile, mostly padding); N = 65 (one valid row in the second tile);
# N = 129 and 257 (one candidate past a kNN tile at 257); k = 1 and 32 (the partial kNN lists inside the x1..x4 region at
# their smallest and largest); k = 16, 17, 24 (the KT = 16 / 24 lists in the forward pass); L = 1, 33, 65, 100, 130 (conv_5
# with a ragged and with more than one 64-column block); B > 1 with ragged N (per-cloud tiles of the conv_5 partials)
NETWORK_SHAPES = [(20, 20, 1, 32), (20, 21, 2, 64), (1, 5, 1, 1), (8, 63, 3, 65), (16, 65, 2, 100), (17, 129, 1, 130),
                  (24, 257, 2, 33), (32, 32, 1, 64), (32, 1000, 2, 32)]


# ------------------------------------------------------------------------------------ kNN, fp32, bit-exact
def knn_f32(x: Tensor, K: int) -> Tuple[Tensor, Tensor]:
    """x [B, N, 3] fp32 -> (squared distances [B, N, K] fp32, idx [B, N, K] int64) of the self-kNN: each product and each sum
    is its own fp32 torch op (nothing can be contracted), then a stable sort on the distance, i.e. (distance, index) order."""
    x = x.detach().cpu()
    assert x.dtype == F32 and x.dim() == 3 and x.shape[-1] == 3
    ds, ids = [], []
    for q0 in range(0, x.shape[1], 512):
        q = x[:, q0:q0 + 512]
        dx = q[:, :, None, 0] - x[:, None, :, 0]
        dy = q[:, :, None, 1] - x[:, None, :, 1]
        dz = q[:, :, None, 2] - x[:, None, :, 2]
        d = dx * dx
        d = d + dy * dy
        d = d + dz * dz
        s, i = torch.sort(d, dim=-1, stable=True)
        ds.append(s[..., :K].clone()); ids.append(i[..., :K].clone())
    return torch.cat(ds, 1), torch.cat(ids, 1)


# ------------------------------------------------------------------------------------ the network
def fold_bn(sd: Dict[str, Tensor], i: int, dtype) -> Tuple[Tensor, Tensor]:
    """eval-mode BatchNorm bn_i as y = s v + t, folded in ``dtype`` in PyTorch's order: invstd = 1 / sqrt(var + eps),
    s = invstd * weight, t = bias - mean * s"""
    w, b, m, v = (sd[f"bn_{i}.{n}"].detach().cpu().to(dtype) for n in ("weight", "bias", "running_mean", "running_var"))
    s = (1 / torch.sqrt(v + EPS)) * w
    return s, b - m * s


def edge_linear(f: Tensor, idx: Tensor, W: Tensor, n0: int = 0) -> Tensor:
    """f [B, N, D], idx [B, n, k] (the neighbours of points n0 .. n0 + n - 1), W [O, 2 D] -> W [f_j - f_i ; f_i] for every
    edge: [B, n, k, O]"""
    B, _, D = f.shape
    nb = f[torch.arange(B)[:, None, None], idx]                               # [B, n, k, D]
    ctr = f[:, n0:n0 + idx.shape[1], None, :].expand(B, idx.shape[1], idx.shape[2], D)
    return torch.cat((nb - ctr, ctr), dim=3) @ W.t()


def bn_lrelu(v: Tensor, s: Tensor, t: Tensor) -> Tensor:
    y = v * s + t
    return torch.where(y > 0, y, y * SLOPE)


def edge_block(f: Tensor, idx: Tensor, W: Tensor, s: Tensor, t: Tensor, chunk: int = 256) -> Tensor:
    """one EdgeConv block, [B, N, D] -> [B, N, O]; the points go through in chunks (the edge tensor is k times the input)"""
    out = [bn_lrelu(edge_linear(f, idx[:, n0:n0 + chunk], W, n0), s, t).max(dim=2).values for n0 in range(0, f.shape[1], chunk)]
    return torch.cat(out, 1)


def dgcnn_forward(sd: Dict[str, Tensor], x: Tensor, idx: Tensor, dtype=F64, fold_dtype=None) -> Tuple[Tensor, Tensor]:
    """x [B, N, 3], idx [B, N, k] -> (latent [B, L], x1234 [B, N, 512]) in ``dtype``.  ``fold_dtype`` (default: dtype) is the
    precision in which the BatchNorms are folded: the exact cases fold in fp32, where their scale is exactly bn.weight."""
    fold_dtype = dtype if fold_dtype is None else fold_dtype
    idx = idx.detach().cpu().long()
    f = x.detach().cpu().to(dtype)
    feats = []
    for i in range(1, 5):
        s, t = (a.to(dtype) for a in fold_bn(sd, i, fold_dtype))
        f = edge_block(f, idx, sd[f"conv_{i}.weight"].detach().cpu().to(dtype), s, t)
        feats.append(f)
    x1234 = torch.cat(feats, dim=-1)
    s, t = (a.to(dtype) for a in fold_bn(sd, 5, fold_dtype))
    y = bn_lrelu(x1234 @ sd["conv_5.weight"].detach().cpu().to(dtype).t(), s, t)
    return y.max(dim=1).values, x1234


# ------------------------------------------------------------------------------------ clouds
def lattice_cloud(B: int, N: int, seed: int) -> Tensor:
    """[B, N, 3] fp32 on the 1/8 lattice, a lattice small enough that ties and duplicated points are everywhere; every
    cloud of the batch has its own points"""
    g = torch.Generator().manual_seed(seed)
    side = max(3, int(round((N / 4) ** (1 / 3))))
    return torch.randint(-side, side + 1, (B, N, 3), generator=g).float() / 8


def surface_cloud(B: int, N: int, seed: int, offset=(0.0, 0.0, 0.0)) -> Tensor:
    """[B, N, 3] fp32: jittered points of an ellipsoid; a large ``offset`` makes the coordinate differences cancel"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, N, 3, generator=g)
    v = v / v.norm(dim=-1, keepdim=True) * torch.tensor([0.6, 0.4, 0.5])
    return (v + torch.randn(B, N, 3, generator=g) * 0.01 + torch.tensor(offset)).float()


# ------------------------------------------------------------------------------------ exact cases
def exact_running_var() -> float:
    """an fp32 running_var with fl32(var + fl32(1e-5)) == 1.0f: sqrt and the division are then exact and the folded scale of
    the BatchNorm is bn.weight itself"""
    eps = np.float32(EPS)
    near = np.float32(1) - eps
    for v in (near, np.nextafter(near, np.float32(0)), np.nextafter(near, np.float32(2))):
        if np.float32(v + eps) == np.float32(1):
            return float(v)
    raise AssertionError("no fp32 value v near 1 - 1e-5 with fl32(v + 1e-5f) == 1")


def _ternary_rows(g, O: int, I: int) -> Tensor:
    """[O, I] weights in {-1, 0, 1} with one to four non-zeros per row"""
    W = torch.zeros(O, I)
    for o in range(O):
        nnz = min(I, 1 + int(torch.randint(0, 4, (1,), generator=g)))
        cols = torch.randperm(I, generator=g)[:nnz]
        W[o, cols] = torch.where(torch.rand(nnz, generator=g) < 0.5, -1.0, 1.0)
    return W


def exact_case(k: int, N: int, B: int, L: int, seed: int = 0):
    """(x [B, N, 3] fp32, idx [B, N, k] int64, state dict, info) of a network whose every fp32 operation is exact.

    Points on the 1/8 lattice; conv weights in {-1, 0, 1}, at most four non-zeros per row; running_var = exact_running_var(),
    so that the folded scale is bn.weight in {-2, 1, -1, 2} (by channel mod 4: both signs in every group of four channels);
    running_mean a multiple of 1/8 in [-1/2, 1/2]; bias an integer per channel that puts the smallest pre-activation of the
    channel into [1, 2) (found in fp64 with the neighbours knn_f32 gives, block by block).  So every value anywhere is a
    multiple of 1/8, leaky-ReLU is the identity, and no channel has s = t = 0.  ``info['bound']`` is, over all five blocks, the
    largest value that any partial sum of the per-edge form or of the kernel's P / Q form can reach in any order
    (max |x| |W1|^T + max |x| |W2 - W1|^T, times |s| = 2, plus |t|): below 2^24 / 8 every such sum is exact in fp32.
    ``info['min_act']`` is the smallest activation (> 0 is the claim)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * k + N)
    x = lattice_cloud(B, N, seed=int(torch.randint(0, 2 ** 31, (1,), generator=g)))
    _, idx = knn_f32(x, k)
    var = exact_running_var()
    sd: Dict[str, Tensor] = {}
    cin = (6, 128, 128, 256, 512)
    bound, min_act = 0.0, float("inf")
    f = x.double()
    feats = []
    for i, C in enumerate(CH + (L,), 1):
        W = _ternary_rows(g, C, cin[i - 1])
        s = torch.tensor([-2.0, 1.0, -1.0, 2.0])[torch.arange(C) % 4]
        mean = torch.randint(-4, 5, (C,), generator=g).float() / 8
        if i < 5:
            D = cin[i - 1] // 2
            pre = edge_linear(f, idx, W.double()) * s.double() - (mean * s).double()   # what the bias is added to
            lo = pre.amin(dim=(0, 1, 2))
            W1, W2 = W[:, :D].double(), W[:, D:].double()
            mag = float((f.abs() @ W1.abs().t()).max() + (f.abs() @ (W2 - W1).abs().t()).max())
        else:
            pre = (f @ W.double().t()) * s.double() - (mean * s).double()
            lo = pre.amin(dim=(0, 1))
            mag = float((f.abs() @ W.double().abs().t()).max())
        bias = (1 - torch.floor(lo)).float()                                  # lo + bias in [1, 2)
        t = bias - mean * s
        bound = max(bound, 2 * mag + float(t.abs().max()))
        sd[f"conv_{i}.weight"] = W
        sd[f"bn_{i}.weight"], sd[f"bn_{i}.bias"], sd[f"bn_{i}.running_mean"] = s, bias, mean
        sd[f"bn_{i}.running_var"] = torch.full((C,), var)
        sd[f"bn_{i}.num_batches_tracked"] = torch.tensor(100, dtype=torch.long)
        act = pre + bias.double()
        min_act = min(min_act, float(act.min()))
        if i < 5:
            f = act.max(dim=2).values
            feats.append(f)
            if i == 4:
                f = torch.cat(feats, dim=-1)
    return x, idx, sd, {"bound": bound, "min_act": min_act}
