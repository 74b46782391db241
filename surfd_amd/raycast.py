"""Ray casting on a triangle mesh on the MI355X path: first hits, crossing counts, and what follows from them (occlusion,
inside / outside, signed distance, visibility between points).  The counterpart of the ray half of open3d's
``o3d.t.geometry.RaycastingScene``, whose ``compute_signed_distance`` the reference calls at AutoEncoder/utils.py:251:

  RaycastingScene.cast_rays               <- RaycastingScene.cast_rays          (t_hit, primitive_ids, primitive_uvs, primitive_normals)
  RaycastingScene.count_intersections     <- RaycastingScene.count_intersections
  RaycastingScene.test_occlusions         <- RaycastingScene.test_occlusions
  RaycastingScene.compute_occupancy       <- RaycastingScene.compute_occupancy  (1 inside, 0 outside)
  RaycastingScene.compute_signed_distance <- RaycastingScene.compute_signed_distance (negative inside)
  RaycastingScene.visible                 no counterpart: is the segment between two points free of the mesh

The ray-triangle test runs in csrc/raycast.hip and nowhere else: device tensors in, device tensors out, CPU tensors are refused
(no CPU fallback).  The unsigned part of the signed distance is meshprep.MeshDistance (csrc/meshdist.hip) on the same mesh.
A ray is ``(ox, oy, oz, dx, dy, dz)``; the direction need not have unit length and ``t`` counts in units of it.  A ray that
holds a NaN or an Inf, or whose direction is zero, hits nothing.  Inside / outside is the parity of the number of crossings
and means something on a closed mesh only; on an open one the three axes of ``nsamples=3`` can disagree, which ``votes`` shows,
and surfd_amd/winding.py (WindingScene: |winding number| >= 1/2) is the answer that survives holes.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple, Union

import torch
from torch import Tensor

from . import _native as N
from .meshprep import MeshDistance, _BvhScene, _check_accel, _check_points, morton_order

BRUTE_FORCE = 1
COUNT_SKIPPED = 2
BVH = 4
COUNT_VISITS = 8


def _check_rays(rays: Tensor, device=None) -> None:
    if rays.dim() != 2 or rays.shape[1] != 6:
        raise ValueError(f"rays must be [R, 6] (origin, direction), got {tuple(rays.shape)}")
    if rays.dtype != torch.float32:
        raise TypeError(f"rays must be float32, got {rays.dtype}")
    if not rays.is_cuda:
        raise RuntimeError("ray casting runs only on the GPU through libsurfd_hip.so (no CPU fallback): move the rays with .cuda()")
    if device is not None and rays.device != device:
        raise RuntimeError(f"rays are on {rays.device}, the mesh is on {device}")


def _check_range(tmin: float, tmax: float) -> Tuple[float, float]:
    tmin, tmax = float(tmin), float(tmax)
    if not (tmin >= 0.0 and math.isfinite(tmin)):
        raise ValueError(f"tmin must be finite and not negative, got {tmin}")
    if math.isnan(tmax):
        raise ValueError("tmax must not be a NaN")
    return tmin, tmax


def _check_nsamples(nsamples: int) -> None:
    if isinstance(nsamples, bool) or not isinstance(nsamples, int) or nsamples not in (1, 3):
        raise ValueError(f"nsamples must be 1 (+z) or 3 (+z, +x, +y), got {nsamples}")


class RaycastingScene(_BvhScene):
    """One mesh, kept for repeated calls.

    The triangles are handed to the library in Morton order of their centroids and every call's rays in Morton order of their
    origins, so that a wave's rays and a tile's triangles are each compact and the kernel's culling bites; results come back in
    the caller's order with the caller's triangle indices.  Two triangles met at the same ``t`` (bit for bit): the one that
    comes first in the Morton order wins.  Host syncs: the constructor checks the vertices and the index range and the
    library's create reads its bad-index flag; the calls themselves do not sync.  One stream at a time per object: the library
    keeps its partial results in a workspace of the handle.

    ``accel="bvh"`` also builds the box hierarchy of csrc/meshbvh.hip (one more host sync); every method then walks it instead
    of the tiles unless ``brute_force=True``, and ``mesh_distance()`` is built with it too.  The results are the same bits."""

    _abi = "surfd_rayscene"

    def __init__(self, vertices: Tensor, triangles: Tensor, accel: str = "tiles"):
        _check_accel(accel)
        self._distance: Optional[MeshDistance] = None
        self.vertices, self.triangles = self._open(vertices, triangles)
        self._set_accel(accel)

    # ---- the two kernels ------------------------------------------------------------------------------------------------------
    def _sorted(self, rays: Tensor):
        _check_rays(rays, self.device)
        R = rays.shape[0]
        if R == 0:
            return rays, None, None
        o = rays[:, :3]
        order = morton_order(torch.where(torch.isfinite(o), o, torch.zeros_like(o)))
        inv = torch.empty_like(order)
        inv[order] = torch.arange(R, device=self.device)
        return rays[order].contiguous(), order, inv

    def _flags(self, brute_force: bool, count_skipped: bool, count_visits: bool = False) -> int:
        use_bvh = self.accel == "bvh" and not brute_force
        if count_visits and not use_bvh:
            raise ValueError("count_visits counts the hierarchy's tests: it needs accel='bvh' and not brute_force")
        return (BRUTE_FORCE if brute_force else 0) | (COUNT_SKIPPED if count_skipped else 0) | (BVH if use_bvh else 0) | \
            (COUNT_VISITS if count_visits else 0)

    def _read_counts(self, count_skipped: bool, count_visits: bool) -> None:
        if count_skipped:
            self.last_skipped_tiles, self.last_total_tiles = self._read_counters("skipped")
        if count_visits:
            self.last_box_tests, self.last_pair_tests = self._read_counters("visits")

    def cast_rays(self, rays: Tensor, tmin: float = 0.0, tmax: float = math.inf, brute_force: bool = False,
                  count_skipped: bool = False, count_visits: bool = False) -> Dict[str, Tensor]:
        """rays [R, 6] -> {"t_hit" [R] float32 (+inf on a miss), "primitive_ids" [R] int64 (-1 on a miss), "primitive_uvs"
        [R, 2] float32, "primitive_normals" [R, 3] float32}: the first triangle met with tmin <= t < tmax.  ``brute_force``
        tests every pair (the correctness baseline; the same bits).  With ``count_skipped`` the number of (wave, tile) visits
        that culling skipped is left in ``last_skipped_tiles`` and their total in ``last_total_tiles`` (one host sync).  With
        ``count_visits`` (``accel="bvh"``) the box tests and pair tests of the call, summed over the rays, are left in
        ``last_box_tests`` and ``last_pair_tests`` (one host sync)."""
        tmin, tmax = _check_range(tmin, tmax)
        flags = self._flags(brute_force, count_skipped, count_visits)
        rs, order, inv = self._sorted(rays)
        R = rays.shape[0]
        t = torch.empty(R, device=self.device, dtype=torch.float32)
        tri = torch.empty(R, device=self.device, dtype=torch.int32)
        uv = torch.empty(R, 2, device=self.device, dtype=torch.float32)
        nrm = torch.empty(R, 3, device=self.device, dtype=torch.float32)
        if R == 0:
            return {"t_hit": t, "primitive_ids": tri.long(), "primitive_uvs": uv, "primitive_normals": nrm}
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_rayscene_cast(self._handle, N.ptr(rs), R, tmin, tmax, flags,
                                                N.ptr(t), N.ptr(tri), N.ptr(uv), N.ptr(nrm), N.stream()))
            self._read_counts(count_skipped, count_visits)
        tri = tri.long()
        ids = torch.where(tri >= 0, self._perm[tri.clamp_min(0)], tri)
        return {"t_hit": t[inv], "primitive_ids": ids[inv], "primitive_uvs": uv[inv], "primitive_normals": nrm[inv]}

    def count_intersections(self, rays: Tensor, tmin: float = 0.0, tmax: float = math.inf, brute_force: bool = False,
                            count_skipped: bool = False, count_visits: bool = False) -> Tensor:
        """rays [R, 6] -> [R] int32: the number of triangles met with tmin <= t < tmax (``count_visits``: as in cast_rays)"""
        tmin, tmax = _check_range(tmin, tmax)
        flags = self._flags(brute_force, count_skipped, count_visits)
        rs, order, inv = self._sorted(rays)
        R = rays.shape[0]
        cnt = torch.empty(R, device=self.device, dtype=torch.int32)
        if R == 0:
            return cnt
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_rayscene_count(self._handle, N.ptr(rs), R, tmin, tmax, flags,
                                                 N.ptr(cnt), N.stream()))
            self._read_counts(count_skipped, count_visits)
        return cnt[inv]

    # ---- what follows from them -----------------------------------------------------------------------------------------------
    def test_occlusions(self, rays: Tensor, tmin: float = 0.0, tmax: float = math.inf, brute_force: bool = False) -> Tensor:
        """rays [R, 6] -> [R] bool: does the ray meet any triangle with tmin <= t < tmax (the count is positive)"""
        return self.count_intersections(rays, tmin, tmax, brute_force=brute_force) > 0

    def compute_occupancy(self, points: Tensor, nsamples: int = 1, brute_force: bool = False,
                          return_votes: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
        """points [N, 3] -> [N] float32, 1 inside and 0 outside: a point is inside when the ray from it along +z crosses the
        mesh an odd number of times; ``nsamples=3`` also asks +x and +y and takes the majority.  ``return_votes`` adds [N] int32,
        the number of axes that said inside: 0 or ``nsamples`` everywhere on a closed mesh, anything on an open one."""
        _check_nsamples(nsamples)
        _check_points("points", points, need_cuda=False)
        _check_points("points", points)
        if points.device != self.device:
            raise RuntimeError(f"points are on {points.device}, the mesh is on {self.device}")
        n = points.shape[0]
        votes = torch.zeros(n, device=self.device, dtype=torch.int32)
        for axis in (2, 0, 1)[:nsamples]:
            rays = torch.zeros(n, 6, device=self.device, dtype=torch.float32)
            rays[:, :3] = points
            rays[:, 3 + axis] = 1.0
            votes += self.count_intersections(rays, brute_force=brute_force) & 1
        occ = (2 * votes > nsamples).float()
        return (occ, votes) if return_votes else occ

    def mesh_distance(self) -> MeshDistance:
        """the closest-point structure of the same mesh (made on first use)"""
        if self._distance is None:
            self._distance = MeshDistance(self.vertices, self.triangles, accel=self.accel)
        return self._distance

    def compute_signed_distance(self, points: Tensor, nsamples: int = 1, brute_force: bool = False) -> Tensor:
        """points [N, 3] -> [N] float32: the distance to the mesh (meshprep.MeshDistance), negative inside (compute_occupancy)"""
        occ = self.compute_occupancy(points, nsamples, brute_force=brute_force)
        dist = self.mesh_distance().closest(points, brute_force=brute_force)[0]
        return torch.where(occ > 0, -dist, dist)

    def visible(self, points_a: Tensor, points_b: Tensor, eps: float = 0.0, brute_force: bool = False) -> Tensor:
        """[N] bool: true where the segment from a to b meets no triangle, i.e. the ray (a, b - a) has no hit with
        eps <= t < 1.  ``eps`` (in units of the segment's length) lets a segment start on the surface."""
        _check_points("points_a", points_a, need_cuda=False)
        _check_points("points_b", points_b, need_cuda=False)
        _check_points("points_a", points_a)
        _check_points("points_b", points_b)
        if points_a.shape != points_b.shape:
            raise ValueError(f"points_a {tuple(points_a.shape)} and points_b {tuple(points_b.shape)} must have the same shape")
        rays = torch.cat([points_a, points_b - points_a], dim=1)
        return ~self.test_occlusions(rays, tmin=eps, tmax=1.0, brute_force=brute_force)
