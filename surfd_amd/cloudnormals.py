"""Normals of point clouds on the MI355X path: for every point the K nearest points of its own cloud (itself included), the
covariance of that neighbourhood and its eigen-decomposition.  The reference ships no evaluation code; the calls stand for
open3d's ``estimate_normals`` / pytorch3d's ``estimate_pointcloud_normals``.

  estimate_normals      [B, N, 3] -> (normals [B, N, 3], eigenvalues [B, N, 3][, idx [B, N, K] int64])   (csrc/cloudnormals.hip)
  surface_variation     eigenvalues -> lambda_0 / (lambda_0 + lambda_1 + lambda_2)  (Pauly et al. 2002; pure torch, any device)
  cloudmetrics.normal_consistency       how well the normals of two clouds agree at nearest neighbours
  meshprep.sample_points_with_normals   surface points of a mesh with their face normals

The contract, per point i of a cloud with n valid points (csrc/cloudnormals.hip states it in full, tests/normals_ref.py restates
it in numpy): d2 = (dx dx + dy dy) + dz dz in fp32 with d = x_j - x_i, one rounding per operation; the neighbourhood is the K
smallest j < n under (d2, j), the point itself being a candidate like any other and ties going to the lower index; first and
second moments of the differences in fp64, in rank order; six cyclic Jacobi sweeps in fp64; eigenvalues ascending, rounded once
to fp32 and not clamped (lambda_0 may be a tiny negative number); the normal is the eigenvector of lambda_0 rounded once to
fp32, not renormalised, with its component of largest magnitude positive (the lowest axis on a tie).  Every output is bit for
bit a function of the point and its cloud: batch, position in the batch and launch geometry do not enter.  Rows at or beyond
``lengths[b]`` come back as zeros (-1 in idx) and their input is never read.

The search and the eigen-solver run in csrc/cloudnormals.hip and nowhere else: device tensors in, device tensors out, CPU
tensors are refused (no CPU fallback).  Out of scope: grid or tree culling (brute force, O(n^2) per cloud), radius or hybrid
neighbourhoods, a globally consistent orientation (``viewpoint`` turns every normal on its own), normals inside the encoder.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from . import _native as N
from .cloudmetrics import _check_form
from .cloudsample import _int_vector

K_MIN, K_MAX = 3, 64
MAX_POINTS = 1 << 20


def _check_ranges(k: int, B: int, n_max: int, lengths: Optional[Tensor]) -> None:
    """the ranges of k and lengths (tensors of any device; a host sync when lengths lives on the GPU)"""
    if not K_MIN <= k <= K_MAX:
        raise ValueError(f"k must lie in {K_MIN} .. {K_MAX}, got {k}")
    if n_max > MAX_POINTS:
        raise ValueError(f"x holds {n_max} points per cloud, more than the supported {MAX_POINTS}")
    if k > n_max:
        raise ValueError(f"k = {k} exceeds the {n_max} points of a cloud")
    if lengths is not None and B and not bool(((lengths >= k) & (lengths <= n_max)).all()):
        raise ValueError(f"lengths must lie in k .. N = {k} .. {n_max}, got {int(lengths.min())} .. {int(lengths.max())}")


def _check_viewpoint(viewpoint, B: int) -> None:
    if not isinstance(viewpoint, Tensor) or viewpoint.shape not in ((3,), (B, 3)):
        raise ValueError(f"viewpoint must be a [3] or [B, 3] = [{B}, 3] tensor, got "
                         f"{tuple(viewpoint.shape) if isinstance(viewpoint, Tensor) else type(viewpoint).__name__}")
    if viewpoint.dtype != torch.float32:
        raise ValueError(f"viewpoint must be float32, got {viewpoint.dtype}")


def _check(x: Tensor, k: int, lengths: Optional[Tensor], viewpoint) -> Optional[Tensor]:
    """shape / dtype / contiguity first, the CPU-tensor refusal after them, then the ranges of k and lengths, the finiteness test
    of the valid part (a host sync) last.  -> lengths as an int32 tensor on x's device, or None"""
    _check_form("x", x)
    B, n_max = x.shape[0], x.shape[1]
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"k must be an int, got {type(k).__name__}")
    if lengths is not None:
        _int_vector("lengths", lengths, B)
    if viewpoint is not None:
        _check_viewpoint(viewpoint, B)
    if not x.is_cuda:
        raise ValueError(f"x is on {x.device}: the normal estimation runs only on the GPU through libsurfd_hip.so "
                         "(no CPU fallback), move it with .cuda()")
    _check_ranges(k, B, n_max, lengths)
    if lengths is not None:
        lengths = lengths.to(device=x.device, dtype=torch.int32).contiguous()
    if x.numel():
        finite = torch.isfinite(x).all(-1)
        if lengths is not None:                                # padding beyond lengths is not checked (and never read)
            finite = finite | (torch.arange(n_max, device=x.device)[None, :] >= lengths[:, None])
        if not bool(finite.all()):
            raise ValueError("x contains NaN or Inf")
    if viewpoint is not None and not bool(torch.isfinite(viewpoint).all()):
        raise ValueError("viewpoint contains NaN or Inf")
    return lengths


def estimate_normals(x: Tensor, k: int = 16, lengths: Optional[Tensor] = None, viewpoint: Optional[Tensor] = None,
                     return_neighbors: bool = False) -> Union[Tuple[Tensor, Tensor], Tuple[Tensor, Tensor, Tensor]]:
    """x [B, N, 3] (or [N, 3]: one cloud, outputs without the batch axis) float32 cuda contiguous -> (normals [B, N, 3] float32,
    eigenvalues [B, N, 3] float32 ascending[, idx [B, N, k] int64 with ``return_neighbors``]).  ``k`` in 3 .. 64: the
    neighbourhood size, the point itself included (idx[..., 0] is the point, or the lowest index among its duplicates).
    ``lengths`` [B] integer: the valid points of every cloud (k .. N; the rest is padding, never read; its rows are zeros and
    -1).  ``viewpoint`` [3] or [B, 3] float32: a normal n at p is negated where ((n_x v_x + n_y v_y) + n_z v_z) < 0 with
    v = viewpoint - p, all in fp32 torch operations, so that it faces the viewpoint; without it the normal's component of
    largest magnitude is positive (surfaces here are unoriented: a canonical representative, no more).

    Host syncs: one for the finiteness test of x (and of viewpoint), one more for the range test of ``lengths`` when it lives
    on the GPU.  The kernel launch itself is stream-ordered."""
    single = isinstance(x, Tensor) and x.dim() == 2
    if single:
        x = x[None]
    lengths32 = _check(x, k, lengths, viewpoint)
    B, n_max = x.shape[0], x.shape[1]
    normals = torch.empty(B, n_max, 3, device=x.device, dtype=torch.float32)
    eigenvalues = torch.empty(B, n_max, 3, device=x.device, dtype=torch.float32)
    idx = torch.empty(B, n_max, k, device=x.device, dtype=torch.int32) if return_neighbors else None
    if B:
        with torch.cuda.device(x.device):
            N.check(N.lib().surfd_cloud_normals(N.ptr(x), B, n_max, N.ptr(lengths32), k, N.ptr(normals), N.ptr(eigenvalues), N.ptr(idx),
                                                N.stream()))
    if viewpoint is not None:
        v = viewpoint.to(x.device).reshape(-1, 1, 3) - x
        if lengths32 is not None:                              # padding may hold anything: its rows stay zero
            v = torch.where((torch.arange(n_max, device=x.device)[None, :] < lengths32[:, None])[:, :, None], v, torch.zeros_like(v))
        dot = (normals[..., 0] * v[..., 0] + normals[..., 1] * v[..., 1]) + normals[..., 2] * v[..., 2]
        normals = torch.where((dot < 0)[..., None], -normals, normals)
    out = (normals, eigenvalues) + ((idx.long(),) if return_neighbors else ())
    return tuple(t[0] for t in out) if single else out


def surface_variation(eigenvalues: Tensor) -> Tensor:
    """eigenvalues [..., 3] ascending (as estimate_normals returns them) -> [...]: max(lambda_0, 0) / (lambda_0 + lambda_1 +
    lambda_2), 0 where the sum is 0 (a neighbourhood of coincident points).  0 on a plane, 1/3 for an isotropic neighbourhood
    (Pauly et al. 2002).  Pure torch, any device, in the dtype of the input."""
    if not isinstance(eigenvalues, Tensor) or eigenvalues.dim() < 1 or eigenvalues.shape[-1] != 3:
        raise ValueError(f"eigenvalues must be a [..., 3] tensor, got "
                         f"{tuple(eigenvalues.shape) if isinstance(eigenvalues, Tensor) else type(eigenvalues).__name__}")
    if not eigenvalues.is_floating_point():
        raise ValueError(f"eigenvalues must be a floating-point tensor, got {eigenvalues.dtype}")
    total = (eigenvalues[..., 0] + eigenvalues[..., 1]) + eigenvalues[..., 2]
    ok = total != 0
    return torch.where(ok, eigenvalues[..., 0].clamp_min(0) / torch.where(ok, total, torch.ones_like(total)), torch.zeros_like(total))
