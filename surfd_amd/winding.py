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

``accel="bvh"`` is the opt-in fast path (Barill et al. 2018, dipole only): the box hierarchy of
csrc/meshbvh.hip over the triangles, and every query replaces a part of the mesh whose centre is farther than ``beta`` times its
radius by one dipole term.  It is an APPROXIMATION (about 3e-2 in w at beta = 2, 1e-2 at beta = 3 on the project's test meshes)
whose cost per query is logarithmic in the number of faces.  ``beta=inf`` evaluates every triangle exactly, in the tree's order.
The default, ``accel="exact"``, is the sum described above, bit for bit.

w depends on the ORIENTATION of the faces.  A wholly inverted mesh gives -w, which ``|w| >= threshold`` forgives; a mesh whose
faces are not consistently oriented (tests/raycast_ref.cube_flipped) gives values between about -0.67 and 0.66 that mean nothing,
while its crossing parity is fine.  ``orient=True`` re-orients such a mesh first (surfd_amd/meshtopo.py: every manifold patch gets
a consistent winding, its lowest face keeps its own); ``orient="outward"`` also turns closed patches so that their volume is
positive.  A patch that has no consistent winding (a Moebius band) raises.  The default leaves the triangles as they came.
The fp64 bits of a query's w do not depend on the other queries of the call, on its position, or on the launch geometry.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from . import _native as N
from .meshprep import MeshDistance, _MeshScene, _check_mesh, _check_points

ONE_SPLIT = 1                   # SURFD_WINDING_ONE_SPLIT
COUNT_VISITS = 2                # SURFD_WINDING_COUNT_VISITS
WINDING_ACCELS = ("exact", "bvh")


def _check_winding_accel(accel: str) -> str:
    if accel not in WINDING_ACCELS:
        raise ValueError(f"accel must be 'exact' or 'bvh', got {accel!r}")
    return accel


def _check_beta(beta: float) -> float:
    beta = float(beta)
    if not beta >= 1.0:                                          # a NaN fails too
        raise ValueError(f"beta must be a finite number >= 1 or +inf, got {beta}")
    return beta


def _check_threshold(threshold: float) -> float:
    threshold = float(threshold)
    if not 0.0 < threshold < 1.0:
        raise ValueError(f"threshold must lie in (0, 1), got {threshold}")
    return threshold


class WindingScene(_MeshScene):
    """One mesh, kept for repeated calls.  The triangles reach the library in the caller's order.  Host syncs: the constructor
    checks the vertices and the index range and the library's create reads its flags; the calls themselves do not sync.  One
    stream at a time per object: the library keeps its partial sums in a workspace of the handle.

    ``accel="bvh"`` builds the hierarchy and its moments (one more host sync) and makes the fast path with ``beta`` the default of
    ``winding_number``, ``compute_occupancy`` and ``compute_signed_distance``; a call's ``accel`` / ``beta`` override both, and
    the hierarchy is built on first use."""

    _abi = "surfd_winding"
    last_visits: Optional[Tuple[int, int]] = None       # (cluster terms, triangle terms) of the last call that counted them

    def __init__(self, vertices: Tensor, triangles: Tensor, orient: Union[bool, str] = False, accel: str = "exact", beta: float = 2.0):
        _check_winding_accel(accel)
        self.beta = _check_beta(beta)
        self._distance: Optional[MeshDistance] = None

        def oriented(v: Tensor, t: Tensor) -> Tensor:
            if orient is False:
                return t
            from .meshtopo import oriented_for_winding
            return oriented_for_winding(v, t, orient)

        self.vertices, self.triangles = self._open(vertices, triangles, morton=False, prepare=oriented)
        self.accel = accel
        self._built = False
        if accel == "bvh":
            self._build_bvh()

    def _build_bvh(self) -> None:
        """the hierarchy and its moments, once per object (the library's build is idempotent): one host sync"""
        if not self._built:
            with torch.cuda.device(self.device):
                N.check(N.lib().surfd_winding_build_bvh(self._handle, N.stream()))
            self._built = True

    def read_bvh(self) -> dict:
        """the hierarchy (built on first use) as the library holds it, for tests: what meshprep._BvhScene.read_bvh gives ("perm" is
        None: the handle has the caller's triangle order) and "records": [nodes, 4, 7] float64, (p.xyz, N.xyz, R2) of a node's 4 children,
        (0, 0, 0, 0, 0, 0, -1) for a child that does not exist; on the device"""
        self._build_bvh()
        levels, leaves, nodes = C.c_int(), C.c_int(), C.c_int()
        sizes = (C.c_int32 * 16)()
        N.check(N.lib().surfd_winding_bvh_info(self._handle, C.byref(levels), C.byref(leaves), C.byref(nodes), sizes, 16))
        boxes = torch.empty(nodes.value, 6, 4, device=self.device, dtype=torch.float32)
        tri = torch.empty(leaves.value, 4, device=self.device, dtype=torch.int32)
        rec = torch.empty(nodes.value, 4, 7, device=self.device, dtype=torch.float64)
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_winding_bvh_read(self._handle, N.ptr(boxes), N.ptr(tri), N.ptr(rec), N.stream()))
        return {"level_sizes": [int(sizes[k]) for k in range(levels.value)], "boxes": boxes, "leaves": tri, "perm": self._perm,
                "records": rec}

    def _points(self, points: Tensor) -> Tensor:
        _check_points("points", points, need_cuda=False)
        _check_points("points", points)
        if points.device != self.device:
            raise RuntimeError(f"points are on {points.device}, the mesh is on {self.device}")
        return points.contiguous()

    def winding_number(self, points: Tensor, one_split: bool = False, accel: Optional[str] = None, beta: Optional[float] = None,
                       count_visits: bool = False) -> Tensor:
        """points [N, 3] float32 -> [N] float64.  A point that holds a NaN or an Inf gets NaN.  ``one_split`` is a test switch of
        the exact path: one workgroup walks all triangles for its queries (the same bits, slower when N is small).  ``accel`` and
        ``beta`` default to the object's.  With ``count_visits`` (``accel="bvh"``) the call's cluster terms and triangle terms,
        summed over the points, are left in ``last_visits`` (one host sync)."""
        accel = self.accel if accel is None else _check_winding_accel(accel)
        beta = self.beta if beta is None else _check_beta(beta)
        if accel == "bvh" and one_split:
            raise ValueError("one_split is a switch of the exact path: it needs accel='exact'")
        if accel != "bvh" and count_visits:
            raise ValueError("count_visits counts the hierarchy's terms: it needs accel='bvh'")
        p = self._points(points)
        w = torch.empty(p.shape[0], device=self.device, dtype=torch.float64)
        if accel == "bvh":
            self._build_bvh()
            with torch.cuda.device(self.device):
                N.check(N.lib().surfd_winding_eval_fast(self._handle, N.ptr(p), p.shape[0], beta, COUNT_VISITS if count_visits else 0,
                                                        N.ptr(w), N.stream()))
                if count_visits:
                    self.last_visits = self._read_counters("visits")
            return w
        if p.shape[0] == 0:
            return w
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_winding_eval(self._handle, N.ptr(p), p.shape[0], ONE_SPLIT if one_split else 0, N.ptr(w), N.stream()))
        return w

    def compute_occupancy(self, points: Tensor, threshold: float = 0.5, return_winding: bool = False,
                          accel: Optional[str] = None, beta: Optional[float] = None) -> Union[Tensor, Tuple[Tensor, Tensor]]:
        """points [N, 3] -> [N] float32, 1 where |w| >= threshold and 0 elsewhere (a NaN point is outside).  The absolute value
        makes a wholly inverted mesh work; inconsistently oriented faces do not (see the module's text).  ``return_winding``
        adds w [N] float64.  ``accel`` / ``beta``: see winding_number."""
        threshold = _check_threshold(threshold)
        w = self.winding_number(points, accel=accel, beta=beta)
        occ = (w.abs() >= threshold).float()
        return (occ, w) if return_winding else occ

    def mesh_distance(self) -> MeshDistance:
        """the closest-point structure of the same mesh (made on first use)"""
        if self._distance is None:
            self._distance = MeshDistance(self.vertices, self.triangles)
        return self._distance

    def compute_signed_distance(self, points: Tensor, threshold: float = 0.5, accel: Optional[str] = None,
                                beta: Optional[float] = None) -> Tensor:
        """points [N, 3] -> [N] float32: the distance to the mesh (meshprep.MeshDistance), negative where compute_occupancy
        says occupied"""
        occ = self.compute_occupancy(points, threshold, accel=accel, beta=beta)
        dist = self.mesh_distance().closest(points)[0]
        return torch.where(occ > 0, -dist, dist)


def winding_number(vertices: Tensor, triangles: Tensor, points: Tensor, orient: Union[bool, str] = False, accel: str = "exact",
                   beta: float = 2.0) -> Tensor:
    """[N] float64: the winding number of the mesh at every point (one WindingScene, one call).  ``orient``, ``accel``, ``beta``:
    see WindingScene."""
    _check_winding_accel(accel)
    _check_beta(beta)
    _check_mesh(vertices, triangles, need_cuda=False)
    _check_points("points", points, need_cuda=False)
    return WindingScene(vertices, triangles, orient=orient, accel=accel, beta=beta).winding_number(points)
