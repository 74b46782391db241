"""Generalized winding numbers of a triangle mesh on the MI355X path: inside / outside that survives holes.

  WindingScene.winding_number          <- libigl's winding_number(V, F, O) (Jacobson et al. 2013)
  WindingScene.compute_occupancy       the role of open3d's RaycastingScene.compute_occupancy, decided by |w| >= threshold
  WindingScene.compute_signed_distance the role of RaycastingScene.compute_signed_distance, signed by the same rule
  winding_number                       the one-shot form

w(p) is the signed solid angle of the mesh seen from p over 4 pi: 1 inside and 0 outside a closed mesh whose faces are oriented
outwards, and a hole costs only its own solid angle, where the parity of ray crossings (surfd_amd/raycast.py, voxelize_solid)
flips a whole cone or column behind every missing face.  The sum runs in csrc/winding.hip and nowhere else: device tensors in,
device tensors out, CPU tensors are refused (no CPU fallback).  Every triangle contributes to every query, so nothing is sorted
or culled: Q x F terms.

w depends on the ORIENTATION of the faces.  A wholly inverted mesh gives -w, which ``|w| >= threshold`` forgives; a mesh whose
faces are not consistently oriented (tests/raycast_ref.cube_flipped) gives values between about -0.67 and 0.66 that mean nothing,
while its crossing parity is fine.  ``orient=True`` re-orients such a mesh first (surfd_amd/meshtopo.py: every manifold patch gets
a consistent winding, its lowest face keeps its own); ``orient="outward"`` also turns closed patches so that their volume is
positive.  A patch that has no consistent winding (a Moebius band) raises.  The default leaves the triangles as they came.
The fp64 bits of a query's w do not depend on the other queries of the call, on its position, or on the launch geometry.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from . import _native as N
from .meshprep import MeshDistance, _MeshScene, _check_mesh, _check_points

ONE_SPLIT = 1                   # SURFD_WINDING_ONE_SPLIT


def _check_threshold(threshold: float) -> float:
    threshold = float(threshold)
    if not 0.0 < threshold < 1.0:
        raise ValueError(f"threshold must lie in (0, 1), got {threshold}")
    return threshold


class WindingScene(_MeshScene):
    """One mesh, kept for repeated calls.  The triangles reach the library in the caller's order.  Host syncs: the constructor
    checks the vertices and the index range and the library's create reads its flags; the calls themselves do not sync.  One
    stream at a time per object: the library keeps its partial sums in a workspace of the handle."""

    _abi = "surfd_winding"

    def __init__(self, vertices: Tensor, triangles: Tensor, orient: Union[bool, str] = False):
        self._distance: Optional[MeshDistance] = None

        def oriented(v: Tensor, t: Tensor) -> Tensor:
            if orient is False:
                return t
            from .meshtopo import oriented_for_winding
            return oriented_for_winding(v, t, orient)

        self.vertices, self.triangles = self._open(vertices, triangles, morton=False, prepare=oriented)

    def _points(self, points: Tensor) -> Tensor:
        _check_points("points", points, need_cuda=False)
        _check_points("points", points)
        if points.device != self.device:
            raise RuntimeError(f"points are on {points.device}, the mesh is on {self.device}")
        return points.contiguous()

    def winding_number(self, points: Tensor, one_split: bool = False) -> Tensor:
        """points [N, 3] float32 -> [N] float64.  A point that holds a NaN or an Inf gets NaN.  ``one_split`` is a test switch:
        one workgroup walks all triangles for its queries (the same bits, slower when N is small)."""
        p = self._points(points)
        w = torch.empty(p.shape[0], device=self.device, dtype=torch.float64)
        if p.shape[0] == 0:
            return w
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_winding_eval(self._handle, N.ptr(p), p.shape[0], ONE_SPLIT if one_split else 0, N.ptr(w), N.stream()))
        return w

    def compute_occupancy(self, points: Tensor, threshold: float = 0.5,
                          return_winding: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
        """points [N, 3] -> [N] float32, 1 where |w| >= threshold and 0 elsewhere (a NaN point is outside).  The absolute value
        makes a wholly inverted mesh work; inconsistently oriented faces do not (see the module's text).  ``return_winding``
        adds w [N] float64."""
        threshold = _check_threshold(threshold)
        w = self.winding_number(points)
        occ = (w.abs() >= threshold).float()
        return (occ, w) if return_winding else occ

    def mesh_distance(self) -> MeshDistance:
        """the closest-point structure of the same mesh (made on first use)"""
        if self._distance is None:
            self._distance = MeshDistance(self.vertices, self.triangles)
        return self._distance

    def compute_signed_distance(self, points: Tensor, threshold: float = 0.5) -> Tensor:
        """points [N, 3] -> [N] float32: the distance to the mesh (meshprep.MeshDistance), negative where compute_occupancy
        says occupied"""
        occ = self.compute_occupancy(points, threshold)
        dist = self.mesh_distance().closest(points)[0]
        return torch.where(occ > 0, -dist, dist)


def winding_number(vertices: Tensor, triangles: Tensor, points: Tensor, orient: Union[bool, str] = False) -> Tensor:
    """[N] float64: the winding number of the mesh at every point (one WindingScene, one call).  ``orient``: see WindingScene."""
    _check_mesh(vertices, triangles, need_cuda=False)
    _check_points("points", points, need_cuda=False)
    return WindingScene(vertices, triangles, orient=orient).winding_number(points)
