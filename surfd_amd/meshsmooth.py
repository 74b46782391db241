"""The vertex-moving steps between the mesh stages on the MI355X path: a mesh that was made and filtered on the device is smoothed
and gets its vertex normals there.

  MeshSmoother                    the neighbourhoods of one connectivity, kept for repeated calls
  MeshSmoother.laplacian          MeshLab's apply_coord_laplacian_smoothing               <- meshproc.laplacian_smooth
  MeshSmoother.smooth_borders     the border smoothing loop of get_mesh_from_udf          <- meshproc.smooth_borders
  MeshSmoother.taubin             Taubin's lambda | mu smoothing, which does not shrink   (no host counterpart)
  MeshSmoother.vertex_normals     corner-angle or area weighted vertex normals            <- meshproc.vertex_normals_by_angle
  laplacian_smooth, smooth_borders, vertex_normals_by_angle, taubin_smooth                the one-shot forms

The work runs in csrc/meshsmooth.hip and nowhere else: device tensors in, device tensors out, CPU tensors are refused (no CPU
fallback).  Positions are float32 or float64 [V, 3]; the arithmetic is fp64 and so are the results, as meshproc's are.  Every
result is a function of the inputs alone: no atomics, a fixed order of summation per vertex (csrc/meshsmooth.hip's header
states it, tests/meshsmooth_ref.py restates it sequentially), so repeated calls agree bit for bit, and so do the device and
the restatement (up to acos in the angle-weighted normals).

Definitions.  Half-edge h = 3 f + c runs from t[f, c] to t[f, (c + 1) % 3].  It is a BORDER half-edge iff its unordered vertex
pair occurs exactly once among all 3 F half-edges; faces with repeated indices take part in that count
(meshproc.border_edge_rows), which is not how meshtopo classifies edges.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from . import _native as N
from .meshconn import _MeshConnectivity

DTYPE = {torch.float32: 0, torch.float64: 1}                 # SURFD_MESHSMOOTH_F32 / _F64
SET = {"all": 0, "border": 1}                                # SURFD_MESHSMOOTH_ALL / _BORDER
WEIGHT = {"angle": 0, "area": 1}                             # SURFD_MESHSMOOTH_ANGLE / _AREA


class MeshSmoother(_MeshConnectivity):
    """The neighbourhoods of one mesh connectivity (per vertex: the half-edges that leave it and that arrive at it, its border
    neighbours, its corners), built once by stable radix sorts and kept.  Host syncs: the constructor only (the bad-index flag
    and the two border counts are read back; ``num_vertices=None`` also reads the largest index); every method only enqueues.
    One stream at a time per object: the library keeps its position buffers in the handle."""

    _abi = "surfd_meshsmooth"
    _what = "the mesh smoothing"
    _vertex_dtypes = tuple(DTYPE)

    def __init__(self, triangles: Tensor, num_vertices: Optional[int] = None):
        faces, vertices, self.num_border_halfedges, self.num_border_vertices = self._open(triangles, num_vertices)
        assert faces == self.num_faces and vertices == self.num_vertices

    def laplacian(self, vertices: Tensor, steps: int = 3, cotangent: bool = True, boundary: bool = True) -> Tensor:
        """[V, 3] float64: ``steps`` Jacobi sweeps of meshproc.laplacian_smooth (MeshLab's apply_coord_laplacian_smoothing with its
        defaults): every vertex moves to (p + sum w p_j) / (1 + sum w) over its half-edges, w the cotangent of the angle opposite
        the half-edge (1 without ``cotangent``); with ``boundary`` a vertex on a border half-edge is averaged with itself and its
        neighbours along the border only.  ``steps=0`` returns a copy."""
        v = self._positions(vertices)
        if int(steps) < 0:
            raise ValueError(f"steps must not be negative, got {steps}")
        if self.num_faces == 0:
            return vertices
        out = torch.empty(self.num_vertices, 3, device=self.device, dtype=torch.float64)
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_meshsmooth_laplacian(self._handle, N.ptr(v), DTYPE[v.dtype], int(steps), int(bool(cotangent)), int(bool(boundary)),
                                                       N.ptr(out), N.stream()))
        return out

    def umbrella(self, vertices: Tensor, k0: float, k1: Optional[float] = None, sweeps: int = 1, neighbours: str = "all") -> Tensor:
        """[V, 3] float64: ``sweeps`` Jacobi sweeps p <- p + k (mean of the neighbours - p), k = k0 in the even sweeps and k1
        (default k0) in the odd ones; ``neighbours``: "all" (the other end of every half-edge at the vertex) or "border" (of its
        border half-edges; other vertices stay).  A vertex without neighbours stays."""
        v = self._positions(vertices)
        if neighbours not in SET:
            raise ValueError(f"neighbours must be one of {sorted(SET)}, got {neighbours!r}")
        if int(sweeps) < 0:
            raise ValueError(f"sweeps must not be negative, got {sweeps}")
        if self.num_faces == 0:
            return vertices
        out = torch.empty(self.num_vertices, 3, device=self.device, dtype=torch.float64)
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_meshsmooth_umbrella(self._handle, N.ptr(v), DTYPE[v.dtype], float(k0), float(k0 if k1 is None else k1), int(sweeps),
                                                      SET[neighbours], N.ptr(out), N.stream()))
        return out

    def smooth_borders(self, vertices: Tensor, lam: float = 0.3, iterations: int = 20) -> Tensor:
        """[V, 3] float64, meshproc.smooth_borders bit for bit: every vertex on a border edge moves ``lam`` of the way to the mean
        of its border neighbours, ``iterations`` times; the others stay."""
        return self.umbrella(vertices, lam, lam, iterations, "border")

    def taubin(self, vertices: Tensor, steps: int = 10, lam: float = 0.5, mu: float = -0.53) -> Tensor:
        """[V, 3] float64: ``steps`` times an umbrella sweep with ``lam`` followed by one with ``mu`` over all half-edges (Taubin
        1995): the negative second factor undoes the shrinkage of the first."""
        if int(steps) < 0:
            raise ValueError(f"steps must not be negative, got {steps}")
        return self.umbrella(vertices, lam, mu, 2 * int(steps), "all")

    def vertex_normals(self, vertices: Tensor, weight: str = "angle", return_raw: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
        """unit [V, 3] float64 (and raw [V, 3] with ``return_raw``): "angle" is meshproc.vertex_normals_by_angle (the unit face
        normals weighted by the corner angles), "area" the sum of the faces' cross products; raw is the sum before it is
        normalised, unit is 0 where raw is."""
        v = self._positions(vertices)
        if weight not in WEIGHT:
            raise ValueError(f"weight must be one of {sorted(WEIGHT)}, got {weight!r}")
        unit = torch.empty(self.num_vertices, 3, device=self.device, dtype=torch.float64)
        raw = torch.empty_like(unit) if return_raw else None
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_meshsmooth_vertex_normals(self._handle, N.ptr(v), DTYPE[v.dtype], WEIGHT[weight], N.ptr(unit), N.ptr(raw), N.stream()))
        return (unit, raw) if return_raw else unit


# ---- one-shot forms -----------------------------------------------------------------------------------------------------------
def _smoother(vertices: Tensor, faces: Tensor) -> MeshSmoother:
    MeshSmoother._check(faces, vertices)
    return MeshSmoother(faces, int(vertices.shape[0]))


def laplacian_smooth(vertices: Tensor, faces: Tensor, steps: int = 3, cotangent: bool = True, boundary: bool = True) -> Tensor:
    """the device counterpart of meshproc.laplacian_smooth (MeshSmoother.laplacian)"""
    return _smoother(vertices, faces).laplacian(vertices, steps, cotangent, boundary)


def smooth_borders(vertices: Tensor, faces: Tensor, lam: float = 0.3, iterations: int = 20) -> Tensor:
    """the device counterpart of meshproc.smooth_borders, bit for bit (MeshSmoother.smooth_borders)"""
    return _smoother(vertices, faces).smooth_borders(vertices, lam, iterations)


def taubin_smooth(vertices: Tensor, faces: Tensor, steps: int = 10, lam: float = 0.5, mu: float = -0.53) -> Tensor:
    """Taubin's lambda | mu smoothing (MeshSmoother.taubin)"""
    return _smoother(vertices, faces).taubin(vertices, steps, lam, mu)


def vertex_normals_by_angle(vertices: Tensor, faces: Tensor) -> Tensor:
    """the device counterpart of meshproc.vertex_normals_by_angle (MeshSmoother.vertex_normals)"""
    return _smoother(vertices, faces).vertex_normals(vertices, "angle")
