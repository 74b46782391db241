"""Point-cloud metrics on the MI355X path: how good a reconstruction is (Chamfer distance, F-score of a pair of clouds) and
how good a SET of generated shapes is against a held-out set (minimum matching distance, coverage and 1-nearest-neighbour
accuracy over Chamfer distances: the protocol of Achlioptas et al. 2018 as used in PointFlow).  The reference ships no
evaluation code, so nothing here has a counterpart there; the pair arithmetic is pytorch3d's ``knn_points(p1, p2, K=1)``.

  nearest_neighbors    per-point nearest neighbour of paired clouds                (csrc/cloudnn.hip, cn_nn_kernel)
  chamfer_distance     d_ab, d_ba, cd, precision, recall, fscore of paired clouds  (the same kernel, both directions)
  normal_consistency   nc_ab, nc_ba, nc: agreement of the normals of paired clouds (nearest_neighbors + torch, fp64)
  chamfer_matrix       [M, R] Chamfer distances between every cloud of two sets    (csrc/cloudnn.hip, cn_matrix_kernel)
  mmd_cov, one_nna     the set metrics on distance matrices (pure torch, any device, fp32 or fp64)
  compute_all_metrics  two sets of clouds -> {"mmd_cd", "cov_cd", "1nna_cd"}
  normalize_clouds     per-cloud normalisation (pure torch)

A Chamfer distance here is the SUM of the two directed means of SQUARED nearest-neighbour distances.  The nearest-neighbour
search runs in csrc/cloudnn.hip and nowhere else: device tensors in, device tensors out, CPU tensors are refused (no CPU
fallback).  Every tie (equal distances) goes to the lower index, in the kernels and in the set metrics.

Out of scope: the earth mover's distance (an approximate auction solver is a project of its own) and ragged sets (all clouds
of one set have the same number of points).  Clouds that cover their surface evenly (less sampling noise in every metric
here) come from cloudsample.farthest_point_sampling / meshprep.sample_points_evenly.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _native as N


# ---- checks -------------------------------------------------------------------------------------------------------------------
def _check_form(name: str, x: Tensor) -> None:
    if not isinstance(x, Tensor) or x.dim() != 3 or x.shape[2] != 3:
        raise ValueError(f"{name} must be a [B, N, 3] tensor, got {tuple(x.shape) if isinstance(x, Tensor) else type(x).__name__}")
    if x.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {x.dtype}")
    if x.shape[1] < 1:
        raise ValueError(f"{name} must hold at least one point per cloud, got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous (call .contiguous())")


def _check_pair(a: Tensor, b: Tensor, paired: bool) -> None:
    """shapes / dtype / contiguity of both first, the CPU-tensor refusal after them, the finiteness test (a host sync) last"""
    _check_form("a", a)
    _check_form("b", b)
    if paired and a.shape[0] != b.shape[0]:
        raise ValueError(f"paired clouds need the same batch size, got {a.shape[0]} and {b.shape[0]}")
    for name, x in (("a", a), ("b", b)):
        if not x.is_cuda:
            raise ValueError(f"{name} is on {x.device}: the nearest-neighbour search runs only on the GPU through libsurfd_hip.so "
                             "(no CPU fallback), move it with .cuda()")
    if a.device != b.device:
        raise ValueError(f"a is on {a.device}, b is on {b.device}")
    for name, x in (("a", a), ("b", b)):
        if x.numel() and not bool(torch.isfinite(x).all()):
            raise ValueError(f"{name} contains NaN or Inf")


def _tau2(f_threshold: float) -> float:
    """tau^2 as the kernels and the yardstick compare against it: float32(tau * tau), the product taken in double"""
    if not f_threshold > 0:
        raise ValueError(f"f_threshold must be positive, got {f_threshold}")
    return float(torch.tensor(float(f_threshold) * float(f_threshold), dtype=torch.float64).float())


# ---- nearest neighbours of paired clouds ---------------------------------------------------------------------------------------
def nearest_neighbors(a: Tensor, b: Tensor) -> Tuple[Tensor, Tensor]:
    """a [B, Na, 3], b [B, Nb, 3] -> (d2 [B, Na] float32, idx [B, Na] int64): for every point of a_i the squared distance to, and
    the index of, its nearest point of b_i.  d2 = (dx dx + dy dy) + dz dz in fp32, ties go to the lower index."""
    _check_pair(a, b, paired=True)
    B, Na, Nb = a.shape[0], a.shape[1], b.shape[1]
    d2 = torch.empty(B, Na, device=a.device, dtype=torch.float32)
    idx = torch.empty(B, Na, device=a.device, dtype=torch.int32)
    if B:
        with torch.cuda.device(a.device):
            N.check(N.lib().surfd_cloud_nn(N.ptr(a), N.ptr(b), B, Na, Nb, N.ptr(d2), N.ptr(idx), N.stream()))
    return d2, idx.long()


def chamfer_distance(a: Tensor, b: Tensor, f_threshold: float = 0.01) -> Dict[str, Tensor]:
    """Paired clouds a [B, Na, 3] (the prediction), b [B, Nb, 3] (the ground truth) -> [B] float32 tensors:
    ``d_ab`` / ``d_ba`` the mean squared nearest-neighbour distance a -> b / b -> a (fp64 mean of the fp32 d2, rounded once),
    ``cd`` = d_ab + d_ba, ``precision`` / ``recall`` the share of a's / b's points whose nearest neighbour is closer than
    ``f_threshold`` (d2 < float32(tau^2), compared in fp32), ``fscore`` = 2 P R / (P + R), 0 where P + R = 0."""
    tau2 = _tau2(f_threshold)
    _check_pair(a, b, paired=True)
    B, Na, Nb = a.shape[0], a.shape[1], b.shape[1]
    d2ab = torch.empty(B, Na, device=a.device, dtype=torch.float32)
    d2ba = torch.empty(B, Nb, device=a.device, dtype=torch.float32)
    if B:
        with torch.cuda.device(a.device):
            N.check(N.lib().surfd_cloud_nn(N.ptr(a), N.ptr(b), B, Na, Nb, N.ptr(d2ab), None, N.stream()))
            N.check(N.lib().surfd_cloud_nn(N.ptr(b), N.ptr(a), B, Nb, Na, N.ptr(d2ba), None, N.stream()))
    d_ab = (d2ab.double().sum(1) / Na).float()
    d_ba = (d2ba.double().sum(1) / Nb).float()
    precision = ((d2ab < tau2).sum(1).double() / Na).float()
    recall = ((d2ba < tau2).sum(1).double() / Nb).float()
    pr = precision + recall
    fscore = torch.where(pr > 0, 2 * precision * recall / pr.clamp_min(1e-30), torch.zeros_like(pr))
    return {"d_ab": d_ab, "d_ba": d_ba, "cd": d_ab + d_ba, "precision": precision, "recall": recall, "fscore": fscore}


def _normals64(name: str, n: Tensor, like: Tensor) -> Tensor:
    if not isinstance(n, Tensor) or n.shape != like.shape:
        raise ValueError(f"{name} must have the shape of its cloud, {tuple(like.shape)}, got "
                         f"{tuple(n.shape) if isinstance(n, Tensor) else type(n).__name__}")
    if not n.is_floating_point():
        raise ValueError(f"{name} must be a floating-point tensor, got {n.dtype}")
    if n.device != like.device:
        raise ValueError(f"{name} is on {n.device}, its cloud on {like.device}")
    return n.double()


def _dot3(p: Tensor, q: Tensor) -> Tensor:
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def _cosines(n: Tensor, m: Tensor, idx: Tensor) -> Tensor:
    """n [B, Na, 3], m [B, Nb, 3] float64, idx [B, Na] into m -> [B, Na]: <n, m'> / sqrt(<n, n> <m', m'>), m' = m[idx]: both
    vectors normalised in fp64, with one division, so that a vector against itself scores exactly 1 (sqrt(s s) = s in binary
    floating point); 0 where either vector is zero"""
    mm = torch.gather(m, 1, idx[:, :, None].expand(-1, -1, 3))
    scale = (_dot3(n, n) * _dot3(mm, mm)).sqrt()
    ok = scale > 0
    return torch.where(ok, _dot3(n, mm) / torch.where(ok, scale, torch.ones_like(scale)), torch.zeros_like(scale))


def normal_consistency(a: Tensor, na: Tensor, b: Tensor, nb: Tensor, oriented: bool = False) -> Dict[str, Tensor]:
    """Paired clouds a [B, Na, 3], b [B, Nb, 3] with normals na [B, Na, 3], nb [B, Nb, 3] (cloudnormals.estimate_normals,
    meshprep.sample_points_with_normals) -> [B] float64 tensors: ``nc_ab`` the mean over the points of a of |<n, n'>| between
    the point's normal and the normal of its nearest neighbour in b (``nearest_neighbors``: ties to the lower index),
    ``nc_ba`` the same from b to a, ``nc`` their average.  ``oriented``: the signed dot product instead of its magnitude, for
    normals that carry an orientation.  Both normals are normalised in fp64; a zero vector scores 0.  1 = the normals agree
    everywhere (the normal consistency MeshUDF reports)."""
    _check_pair(a, b, paired=True)
    na64, nb64 = _normals64("na", na, a), _normals64("nb", nb, b)
    _, iab = nearest_neighbors(a, b)
    _, iba = nearest_neighbors(b, a)
    dab, dba = _cosines(na64, nb64, iab), _cosines(nb64, na64, iba)
    if not oriented:
        dab, dba = dab.abs(), dba.abs()
    nc_ab, nc_ba = dab.mean(1), dba.mean(1)
    return {"nc_ab": nc_ab, "nc_ba": nc_ba, "nc": (nc_ab + nc_ba) / 2}


# ---- Chamfer matrix of two sets -------------------------------------------------------------------------------------------------
def directed_means(A: Tensor, B: Tensor, tau2: Optional[float] = None, chunk: Optional[int] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """A [M, Na, 3], B [R, Nb, 3] -> (mean [M, R] float32, below [M, R] int32 or None): mean[i, j] = the mean over the points of
    A_i of the squared distance to their nearest point of B_j; with ``tau2`` also how many of those are < tau2.  ``chunk`` bounds
    the clouds of either set per launch; every entry has the same bits whatever it is."""
    _check_pair(A, B, paired=False)
    M, Na, R, Nb = A.shape[0], A.shape[1], B.shape[0], B.shape[1]
    if chunk is not None and chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    mean = torch.empty(M, R, device=A.device, dtype=torch.float32)
    below = torch.empty(M, R, device=A.device, dtype=torch.int32) if tau2 is not None else None
    cm, cr = min(M, chunk or M), min(R, chunk or R)
    L = N.lib()
    with torch.cuda.device(A.device):
        for i0 in range(0, M, max(cm, 1)):
            for j0 in range(0, R, max(cr, 1)):
                a, b = A[i0:i0 + cm], B[j0:j0 + cr]
                whole = a.shape[0] == M and b.shape[0] == R
                m = mean if whole else torch.empty(a.shape[0], b.shape[0], device=A.device, dtype=torch.float32)
                c = None if below is None else (below if whole else torch.empty(a.shape[0], b.shape[0], device=A.device, dtype=torch.int32))
                N.check(L.surfd_cloud_nn_matrix(N.ptr(a), a.shape[0], Na, N.ptr(b), b.shape[0], Nb, float(tau2 or 0.0), N.ptr(m), N.ptr(c),
                                                N.stream()))
                if not whole:
                    mean[i0:i0 + cm, j0:j0 + cr] = m
                    if below is not None:
                        below[i0:i0 + cm, j0:j0 + cr] = c
    return mean, below


def chamfer_matrix(A: Tensor, B: Tensor, chunk: Optional[int] = None) -> Tensor:
    """A [M, Na, 3], B [R, Nb, 3] -> [M, R] float32 Chamfer distances: mean_ab + mean_ba.T (one fp32 addition per entry).  Two
    launches per chunk pair, one per direction; when B is A (the same tensor) the second direction is the transpose of the first
    and is not computed again.  ``chunk`` bounds the clouds per launch only."""
    ab, _ = directed_means(A, B, chunk=chunk)
    same = A is B or (A.data_ptr() == B.data_ptr() and A.shape == B.shape)
    ba = ab if same else directed_means(B, A, chunk=chunk)[0]
    return ab + ba.t()


# ---- set metrics on distance matrices (pure torch) --------------------------------------------------------------------------------
def _check_matrix(name: str, D: Tensor, shape=None) -> None:
    if not isinstance(D, Tensor) or D.dim() != 2 or D.shape[0] < 1 or D.shape[1] < 1:
        raise ValueError(f"{name} must be a non-empty 2-D tensor")
    if D.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name} must be float32 or float64, got {D.dtype}")
    if shape is not None and tuple(D.shape) != tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(D.shape)}")
    if bool(torch.isnan(D).any()):
        raise ValueError(f"{name} contains NaN")


def _argmin_low(D: Tensor, dim: int) -> Tuple[Tensor, Tensor]:
    """(min, argmin) along ``dim`` with every tie broken towards the lower index, spelled out so that it does not rest on what
    a device's argmin does with ties"""
    v = D.min(dim, keepdim=True).values
    n = D.shape[dim]
    ar = torch.arange(n, device=D.device).reshape([n if d == dim else 1 for d in range(D.dim())])
    idx = torch.where(D == v, ar, torch.full_like(ar, n)).min(dim).values
    return v.squeeze(dim), idx


def mmd_cov(D: Tensor) -> Dict[str, float]:
    """D [G, R]: distances between G generated and R reference samples ->
    ``mmd``: mean over the reference samples j of min_i D[i, j] (how close the nearest generated sample is);
    ``cov``: the share of reference samples that are the nearest reference sample (lower index on ties) of some generated one;
    ``mmd_smp``: mean over the generated samples i of min_j D[i, j]."""
    _check_matrix("D", D)
    min_gen, _ = _argmin_low(D, 0)
    min_ref, nearest_ref = _argmin_low(D, 1)
    return {"mmd": float(min_gen.double().mean()), "cov": float(torch.unique(nearest_ref).numel()) / D.shape[1],
            "mmd_smp": float(min_ref.double().mean())}


def one_nna(D_gg: Tensor, D_rr: Tensor, D_gr: Tensor) -> Dict[str, float]:
    """1-nearest-neighbour accuracy.  D_gg [G, G], D_rr [R, R], D_gr [G, R] form the matrix of the union ordered [generated;
    reference]; every sample is classified by the label of its nearest OTHER sample (diagonal excluded, lower index on ties).
    ``acc``: share of samples classified as what they are (0.5 = the two sets cannot be told apart, 1.0 = disjoint),
    ``acc_gen`` / ``acc_ref``: the same over the generated / the reference samples alone."""
    _check_matrix("D_gr", D_gr)
    G, R = D_gr.shape
    _check_matrix("D_gg", D_gg, (G, G))
    _check_matrix("D_rr", D_rr, (R, R))
    if not (D_gg.dtype == D_rr.dtype == D_gr.dtype and D_gg.device == D_rr.device == D_gr.device):
        raise ValueError("D_gg, D_rr and D_gr must share dtype and device")
    if G + R < 2:
        raise ValueError("1-NNA needs at least two samples")
    U = torch.cat((torch.cat((D_gg, D_gr), 1), torch.cat((D_gr.t(), D_rr), 1)), 0).clone()
    U.fill_diagonal_(float("inf"))
    _, nn = _argmin_low(U, 1)
    pred_ref = nn >= G
    is_ref = torch.arange(G + R, device=U.device) >= G
    ok = pred_ref == is_ref
    # shares as one correctly rounded division of two integers (a mean of 0 / 1 values need not round the same way)
    return {"acc": int(ok.sum()) / (G + R), "acc_gen": int(ok[:G].sum()) / G, "acc_ref": int(ok[G:].sum()) / R}


def compute_all_metrics(gen: Tensor, ref: Tensor, chunk: Optional[int] = None, return_matrices: bool = False) -> dict:
    """gen [G, N, 3], ref [R, N, 3] -> {"mmd_cd", "cov_cd", "1nna_cd"} (python floats; + "mmd_smp_cd", "1nna_cd_gen",
    "1nna_cd_ref"), and with ``return_matrices`` the three Chamfer matrices "D_gr" [G, R], "D_gg" [G, G], "D_rr" [R, R]."""
    _check_pair(gen, ref, paired=False)
    D_gr = chamfer_matrix(gen, ref, chunk=chunk)
    D_gg = chamfer_matrix(gen, gen, chunk=chunk)
    D_rr = chamfer_matrix(ref, ref, chunk=chunk)
    mc, nna = mmd_cov(D_gr), one_nna(D_gg, D_rr, D_gr)
    out = {"mmd_cd": mc["mmd"], "cov_cd": mc["cov"], "1nna_cd": nna["acc"], "mmd_smp_cd": mc["mmd_smp"], "1nna_cd_gen": nna["acc_gen"],
           "1nna_cd_ref": nna["acc_ref"]}
    if return_matrices:
        out.update({"D_gr": D_gr, "D_gg": D_gg, "D_rr": D_rr})
    return out


# ---- normalisation (pure torch) --------------------------------------------------------------------------------------------------
def normalize_clouds(x: Tensor, mode: str = "bbox") -> Tensor:
    """x [B, N, 3] (or [N, 3]) -> the same shape, every cloud on its own: ``"none"`` unchanged; ``"unit_sphere"`` centroid to the
    origin, then scaled so that the farthest point has radius 1; ``"bbox"`` bounding-box centre to the origin, then scaled so that
    the longest side is 2 (the cloud fills [-1, 1] along it).  A cloud without extent is only centred."""
    if x.dim() not in (2, 3) or x.shape[-1] != 3 or x.shape[-2] < 1:
        raise ValueError(f"x must be [B, N, 3] or [N, 3] with N >= 1, got {tuple(x.shape)}")
    if not x.is_floating_point():
        raise ValueError(f"x must be a floating-point tensor, got {x.dtype}")
    if mode == "none":
        return x
    if mode == "unit_sphere":
        c = x - x.mean(-2, keepdim=True)
        r = c.norm(dim=-1).amax(-1)[..., None, None]
    elif mode == "bbox":
        lo, hi = x.amin(-2, keepdim=True), x.amax(-2, keepdim=True)
        c = x - (lo + hi) / 2
        r = ((hi - lo).amax(-1, keepdim=True)) / 2
    else:
        raise ValueError(f"unknown mode '{mode}' (none, unit_sphere, bbox)")
    return c / torch.where(r > 0, r, torch.ones_like(r))
