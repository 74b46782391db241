"""Farthest point sampling on the MI355X path: K points of a cloud that cover it evenly, each the point farthest from every
pick before it.  The reference samples at random (utils/utils.py:44-77, restated as ``dgcnn.random_point_sampling``); this
module stands for pytorch3d's ``sample_farthest_points``.

  farthest_point_sampling   [B, N, 3] -> (idx [B, K] int64, cover2 [B, K] float32)      (csrc/cloudfps.hip)
  sample_farthest_points    pytorch3d's call shape: -> (points [B, K, 3], idx [B, K])
  meshprep.sample_points_evenly   mesh -> K even surface points (uniform candidates, then farthest point sampling)

The loop, per cloud with n valid points: mind = +inf; s = start; for k < K: idx[k] = s; mind[i] = min(mind[i], d2(p_i, p_s)) with
d2 = (dx dx + dy dy) + dz dz in fp32, one rounding per operation; s = argmax mind, the LOWER index on ties; cover2[k] = mind[s],
the squared covering radius of the first k + 1 picks.  The minimum and the maximum only select, so the index sequence is bit
for bit a function of the input (tests/fps_ref.py restates it in numpy).  Beyond n picks: idx = -1, cover2 = 0.  Duplicated
points are legal: once everything is covered the lowest index is picked again.

The search runs in csrc/cloudfps.hip and nowhere else: device tensors in, device tensors out, CPU tensors are refused (no CPU
fallback).  Out of scope: one cloud spread over several workgroups, weighted or feature-space sampling.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from . import _native as N
from .cloudmetrics import _check_form

MAX_POINTS = 1 << 20


def _int_vector(name: str, v, B: int) -> None:
    if not isinstance(v, Tensor) or v.dim() != 1 or v.shape[0] != B:
        raise ValueError(f"{name} must be a [B] = [{B}] tensor, got {tuple(v.shape) if isinstance(v, Tensor) else type(v).__name__}")
    if v.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name} must be int32 or int64, got {v.dtype}")


def _check_ranges(K: int, B: int, n_max: int, lengths: Optional[Tensor], start_index) -> None:
    """the ranges of K, lengths and start_index (tensors of any device; a host sync when they live on the GPU)"""
    if K < 1:
        raise ValueError(f"K must be at least 1, got {K}")
    if n_max > MAX_POINTS:
        raise ValueError(f"x holds {n_max} points per cloud, more than the supported {MAX_POINTS}")
    if lengths is not None and B and not bool(((lengths >= 1) & (lengths <= n_max)).all()):
        raise ValueError(f"lengths must lie in 1 .. N = {n_max}, got {int(lengths.min())} .. {int(lengths.max())}")
    if isinstance(start_index, Tensor):
        limit = lengths.to(start_index.device) if lengths is not None else n_max
        if B and not bool(((start_index >= 0) & (start_index < limit)).all()):
            raise ValueError("start_index must lie in 0 .. n - 1 of every cloud (n = lengths[b], else N)")
    else:
        lowest = int(lengths.min()) if (lengths is not None and B) else n_max
        if not 0 <= start_index < lowest:
            raise ValueError(f"start_index must lie in 0 .. n - 1 of every cloud (n = lengths[b], else N), got {start_index}")


def _check(x: Tensor, K: int, lengths: Optional[Tensor], start_index) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """shape / dtype / contiguity first, the CPU-tensor refusal after them, then the ranges of K, lengths and start_index, the
    finiteness test of the valid part (a host sync) last.  -> (lengths, start) as int32 tensors on x's device, or None"""
    _check_form("x", x)
    B, n_max = x.shape[0], x.shape[1]
    if isinstance(K, bool) or not isinstance(K, int):
        raise ValueError(f"K must be an int, got {type(K).__name__}")
    if lengths is not None:
        _int_vector("lengths", lengths, B)
    if isinstance(start_index, Tensor):
        _int_vector("start_index", start_index, B)
    elif isinstance(start_index, bool) or not isinstance(start_index, int):
        raise ValueError(f"start_index must be an int or a [B] integer tensor, got {type(start_index).__name__}")
    if not x.is_cuda:
        raise ValueError(f"x is on {x.device}: the farthest point sampling runs only on the GPU through libsurfd_hip.so "
                         "(no CPU fallback), move it with .cuda()")
    _check_ranges(K, B, n_max, lengths, start_index)
    if lengths is not None:
        lengths = lengths.to(device=x.device, dtype=torch.int32).contiguous()
    if isinstance(start_index, Tensor):
        start = start_index.to(device=x.device, dtype=torch.int32).contiguous()
    else:
        start = None if start_index == 0 else torch.full((B,), start_index, device=x.device, dtype=torch.int32)
    if x.numel():
        finite = torch.isfinite(x).all(-1)
        if lengths is not None:                                # padding beyond lengths is not checked (and never read)
            finite = finite | (torch.arange(n_max, device=x.device)[None, :] >= lengths[:, None])
        if not bool(finite.all()):
            raise ValueError("x contains NaN or Inf")
    return lengths, start


def farthest_point_sampling(x: Tensor, K: int, lengths: Optional[Tensor] = None,
                            start_index: Union[int, Tensor] = 0) -> Tuple[Tensor, Tensor]:
    """x [B, N, 3] float32 cuda contiguous -> (idx [B, K] int64, cover2 [B, K] float32).  ``lengths`` [B] integer: the valid
    points of every cloud (1 .. N; the rest is padding, never read).  ``start_index`` an int or a [B] integer tensor: the first
    pick (0 .. n - 1).  idx[b, k] is the k-th pick of cloud b (-1 beyond n picks); cover2[b, k] the squared covering radius of
    the first k + 1 picks: every valid point of the cloud lies within it of a pick.  Ties go to the lower index."""
    lengths32, start32 = _check(x, K, lengths, start_index)
    B, n_max = x.shape[0], x.shape[1]
    idx = torch.empty(B, K, device=x.device, dtype=torch.int32)
    cover2 = torch.empty(B, K, device=x.device, dtype=torch.float32)
    if B:
        L = N.lib()
        with torch.cuda.device(x.device):
            nbytes = int(L.surfd_cloud_fps_workspace_bytes(B, n_max))
            work = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32) if nbytes else None
            N.check(L.surfd_cloud_fps(N.ptr(x), B, n_max, N.ptr(lengths32), N.ptr(start32), K, N.ptr(idx), N.ptr(cover2), N.ptr(work),
                                      N.stream()))
    return idx.long(), cover2


def sample_farthest_points(x: Tensor, K: int, lengths: Optional[Tensor] = None, random_start_point: bool = False,
                           generator: Optional[torch.Generator] = None) -> Tuple[Tensor, Tensor]:
    """pytorch3d's call shape: x [B, N, 3] -> (points [B, K, 3], idx [B, K] int64).  Rows with idx == -1 (K above a cloud's
    length) are zero-filled.  ``random_start_point``: the first pick of every cloud is drawn with ``torch.randint`` on
    ``generator`` (of any device; the draw is moved to x's), uniformly over its valid points; otherwise it is point 0."""
    start: Union[int, Tensor] = 0
    if random_start_point:
        _check_form("x", x)
        B, n_max = x.shape[0], x.shape[1]
        if lengths is not None:
            _int_vector("lengths", lengths, B)
        dev = generator.device if generator is not None else x.device
        # one draw per cloud in [0, 2^31), reduced modulo the cloud's length: a [B] call whose count does not depend on the lengths
        draw = torch.randint(0, 2 ** 31 - 1, (B,), generator=generator, device=dev).to(x.device)
        n = lengths.to(x.device).long().clamp(1, n_max) if lengths is not None else torch.full((B,), n_max, device=x.device)
        start = draw % n
    idx, _ = farthest_point_sampling(x, K, lengths=lengths, start_index=start)
    points = torch.gather(x, 1, idx.clamp_min(0)[:, :, None].expand(-1, -1, 3))
    return torch.where((idx >= 0)[:, :, None], points, torch.zeros_like(points)), idx
