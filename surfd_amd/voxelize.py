"""Occupancy grids and volumetric IoU on the MI355X path (csrc/voxel.hip).

  voxelize_surface   mesh -> the voxels its triangles touch (conservative: the separating-axis test on closed voxels)
  voxelize_solid     mesh -> parity fill along +z (| surface), and the number of columns with an odd crossing total
  voxelize_winding   mesh -> the voxels whose centre has |winding number| >= threshold (surfd_amd/winding.py): for meshes with holes
  voxelize_points    cloud -> the voxels that hold a point
  VoxelGrid          the bit-packed grid [R, R, W] uint32 (stored as int32), W = ceil(R / 32); .dense() gives bool [R, R, R]
  voxel_iou          paired IoU of grids or packed batches;  voxel_iou_matrix  every a against every b
  is_closed          odd_columns == 0: the snapped mesh is closed over the grid's columns

No reference counterpart (the reference ships no evaluation code).  The grid is the cube [lo, hi]^3 in R^3 closed voxels, axes
(x, y, z) = (i, j, k), 1 <= R <= 512.  One fp32 step (the snap to 1/256 voxel), then integers: a grid has the same bits for any
face order, winding, batch and path (voxelize_winding is the exception: fp64 sums at the voxel centres, and the orientation of
the faces matters).  It runs in the library and nowhere else; CPU tensors are refused (no CPU fallback).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _native as N

FORCE_SMALL = 1                 # SURFD_VOXEL_FORCE_SMALL
FORCE_LARGE = 2                 # SURFD_VOXEL_FORCE_LARGE
MAX_RESOLUTION = 512
PATHS = {None: 0, "default": 0, "small": FORCE_SMALL, "large": FORCE_LARGE}


def words(resolution: int) -> int:
    return (resolution + 31) // 32


def _check_grid(resolution: int, bounds) -> Tuple[int, Tuple[float, float]]:
    R = int(resolution)
    if not 1 <= R <= MAX_RESOLUTION:
        raise ValueError(f"resolution must lie in [1, {MAX_RESOLUTION}], got {resolution}")
    lo, hi = float(bounds[0]), float(bounds[1])
    if not hi > lo:
        raise ValueError(f"bounds must be (lo, hi) with lo < hi, got {bounds}")
    return R, (lo, hi)


def _no_cpu(t: Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what} runs only on the GPU through libsurfd_hip.so (no CPU fallback): move the input with .cuda()")


def _check_mesh(vertices: Tensor, faces: Tensor) -> Tuple[Tensor, Tensor]:
    if not isinstance(vertices, Tensor) or not isinstance(faces, Tensor):
        raise TypeError("vertices and faces must be tensors")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertices must be [V, 3], got {tuple(vertices.shape)}")
    if vertices.dtype != torch.float32:
        raise TypeError(f"vertices must be float32, got {vertices.dtype}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be [F, 3], got {tuple(faces.shape)}")
    if faces.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"faces must be int32 or int64, got {faces.dtype}")
    _no_cpu(vertices, "the voxeliser")
    _no_cpu(faces, "the voxeliser")
    if vertices.device != faces.device:
        raise ValueError(f"vertices are on {vertices.device}, faces on {faces.device}")
    if faces.dtype == torch.int64:         # an index that does not fit int32 must not wrap into [0, V): -1 is dropped and counted
        faces = torch.where((faces < 0) | (faces >= 2 ** 31), torch.full_like(faces, -1), faces)
    return vertices.contiguous(), faces.to(torch.int32).contiguous()


class VoxelGrid:
    """A bit-packed occupancy grid on the device: ``packed`` is int32 [R, R, W] holding the uint32 words (bit k & 31 of word
    k >> 5 of column (i, j) is voxel (i, j, k)); padding bits are zero."""

    def __init__(self, packed: Tensor, resolution: int, bounds=(-1.0, 1.0)):
        R, self.bounds = _check_grid(resolution, bounds)
        if packed.dtype != torch.int32 or tuple(packed.shape) != (R, R, words(R)):
            raise ValueError(f"packed must be int32 [{R}, {R}, {words(R)}], got {packed.dtype} {tuple(packed.shape)}")
        self.packed = packed.contiguous()
        self.resolution = R

    @classmethod
    def empty(cls, resolution: int, bounds=(-1.0, 1.0), device="cuda") -> "VoxelGrid":
        R, _ = _check_grid(resolution, bounds)
        return cls(torch.zeros(R, R, words(R), dtype=torch.int32, device=device), R, bounds)

    @classmethod
    def from_dense(cls, dense: Tensor, bounds=(-1.0, 1.0)) -> "VoxelGrid":
        """bool [R, R, R] -> grid (a layout change in torch, on the tensor's device)"""
        if dense.dim() != 3 or not dense.shape[0] == dense.shape[1] == dense.shape[2]:
            raise ValueError(f"dense must be [R, R, R], got {tuple(dense.shape)}")
        R = dense.shape[0]
        pad = torch.zeros(R, R, words(R) * 32, dtype=torch.int64, device=dense.device)
        pad[:, :, :R] = dense != 0
        w = (pad.reshape(R, R, words(R), 32) << torch.arange(32, device=dense.device)).sum(-1)
        return cls(torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32), R, bounds)

    def dense(self) -> Tensor:
        """bool [R, R, R]"""
        R = self.resolution
        bit = (self.packed.to(torch.int64)[..., None] >> torch.arange(32, device=self.packed.device)) & 1
        return bit.reshape(R, R, -1)[:, :, :R].bool()

    def count(self) -> int:
        """number of occupied voxels (a popcount in the library: the IoU kernel's union of the grid with itself)"""
        return int(_iou(self.packed[None], self.packed[None], self.resolution, True)[1].item())

    def __repr__(self) -> str:
        return f"VoxelGrid(resolution={self.resolution}, bounds={self.bounds}, device={self.packed.device})"


def _out(out: Optional[VoxelGrid], R: int, bounds, device) -> VoxelGrid:
    if out is None:
        return VoxelGrid.empty(R, bounds, device)
    if not isinstance(out, VoxelGrid) or out.resolution != R or out.bounds != bounds:
        raise ValueError(f"out must be a VoxelGrid of resolution {R} and bounds {bounds}, got {out!r}")
    _no_cpu(out.packed, "the voxeliser")
    if out.packed.device != device:
        raise ValueError(f"out is on {out.packed.device}, the input on {device}")
    return out


def _flags(path) -> int:
    if path not in PATHS:
        raise ValueError(f"path must be one of None, 'small', 'large', got {path!r}")
    return PATHS[path]


def _workspace(F: int, R: int, device) -> Tensor:
    return torch.empty(int(N.lib().surfd_voxel_workspace_bytes(F, R)) // 4, dtype=torch.int32, device=device)


def voxelize_surface(vertices: Tensor, faces: Tensor, resolution: int = 32, bounds=(-1.0, 1.0), out: Optional[VoxelGrid] = None,
                     path: Optional[str] = None, return_counts: bool = False):
    """The voxels the mesh's triangles intersect (closed voxels: touching counts).  ``out``: a grid to OR into.  ``path``:
    None, 'small' or 'large': a TEST switch (one code path for every triangle; the grids are bit-identical) — 'small' makes one
    lane walk a triangle's whole box, so keep it to small meshes and coarse grids.  With ``return_counts`` also a
    dict of the dropped (invalid vertex or index) and degenerate (zero snapped area) triangle counts."""
    R, bounds = _check_grid(resolution, bounds)
    flags = _flags(path)
    vertices, faces = _check_mesh(vertices, faces)
    grid = _out(out, R, bounds, vertices.device)
    with torch.cuda.device(vertices.device):
        counts = torch.zeros(2, dtype=torch.int32, device=vertices.device)
        ws = _workspace(faces.shape[0], R, vertices.device)
        N.check(N.lib().surfd_voxel_surface(N.ptr(vertices), vertices.shape[0], N.ptr(faces), faces.shape[0], bounds[0], bounds[1], R, flags,
                                            N.ptr(ws), N.ptr(grid.packed), counts.data_ptr(), counts.data_ptr() + 4, N.stream()))
    if return_counts:
        c = counts.tolist()
        return grid, {"dropped": c[0], "degenerate": c[1]}
    return grid


def voxelize_solid(vertices: Tensor, faces: Tensor, resolution: int = 32, bounds=(-1.0, 1.0), out: Optional[VoxelGrid] = None,
                   path: Optional[str] = None, include_surface: bool = True, return_counts: bool = False):
    """Parity fill along +z, OR-ed with the surface voxels when ``include_surface``.  -> (grid, odd_columns): the number of
    columns whose crossing total is odd, 0 for a closed snapped mesh (the fill of an open mesh leaks along those columns;
    voxelize_winding fills such a mesh without the leak).
    With ``return_counts`` the second value is a dict with 'odd_columns' and 'dropped'."""
    R, bounds = _check_grid(resolution, bounds)
    flags = _flags(path)
    vertices, faces = _check_mesh(vertices, faces)
    grid = _out(out, R, bounds, vertices.device)
    with torch.cuda.device(vertices.device):
        counts = torch.zeros(2, dtype=torch.int32, device=vertices.device)
        ws = _workspace(faces.shape[0], R, vertices.device)
        N.check(N.lib().surfd_voxel_solid(N.ptr(vertices), vertices.shape[0], N.ptr(faces), faces.shape[0], bounds[0], bounds[1], R, flags,
                                          N.ptr(ws), int(bool(include_surface)), N.ptr(grid.packed), counts.data_ptr(), counts.data_ptr() + 4,
                                          N.stream()))
    c = counts.tolist()
    return grid, ({"odd_columns": c[0], "dropped": c[1]} if return_counts else c[0])


def voxelize_winding(vertices: Tensor, faces: Tensor, resolution: int = 32, bounds=(-1.0, 1.0), threshold: float = 0.5,
                     accel: str = "exact", beta: float = 2.0) -> VoxelGrid:
    """The voxels whose centre lies inside the mesh by its generalized winding number: |w| >= ``threshold`` (csrc/winding.hip
    through surfd_amd/winding.py).  A hole costs only its own solid angle, so a mesh with small holes fills as the closed one
    does, where voxelize_solid leaks along every column through a hole.  The centres are
    lo + (arange(R, dtype=float32) + 0.5) * ((hi - lo) / R), built in torch on the device; R^3 x F terms, nothing is culled.  The
    faces must be consistently oriented (all outwards or all inwards); surface voxels are not OR-ed in.  Indices outside
    [0, V) and vertices that are not finite are refused, not dropped.  ``accel="bvh"`` takes the winding numbers from the fast
    path with ``beta`` (an approximation whose cost is logarithmic in F; WindingScene)."""
    from .winding import WindingScene, _check_beta, _check_threshold, _check_winding_accel
    R, bounds = _check_grid(resolution, bounds)
    threshold = _check_threshold(threshold)
    _check_winding_accel(accel)
    _check_beta(beta)
    if not isinstance(vertices, Tensor) or not isinstance(faces, Tensor):
        raise TypeError("vertices and faces must be tensors")
    scene = WindingScene(vertices, faces, accel=accel, beta=beta)
    lo, hi = bounds
    with torch.cuda.device(scene.device):
        c = lo + (torch.arange(R, dtype=torch.float32, device=scene.device) + 0.5) * ((hi - lo) / R)
        centres = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), dim=-1).reshape(-1, 3)
        occ = scene.compute_occupancy(centres, threshold)
    return VoxelGrid.from_dense(occ.reshape(R, R, R) > 0, bounds)


def voxelize_points(points: Tensor, resolution: int = 32, bounds=(-1.0, 1.0), out: Optional[VoxelGrid] = None, return_counts: bool = False):
    """The voxels that hold a point of the cloud [P, 3]; points outside the grid (or NaN) are skipped and counted."""
    R, bounds = _check_grid(resolution, bounds)
    if not isinstance(points, Tensor):
        raise TypeError("points must be a tensor")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [P, 3], got {tuple(points.shape)}")
    if points.dtype != torch.float32:
        raise TypeError(f"points must be float32, got {points.dtype}")
    _no_cpu(points, "the voxeliser")
    points = points.contiguous()
    grid = _out(out, R, bounds, points.device)
    with torch.cuda.device(points.device):
        outside = torch.zeros(1, dtype=torch.int32, device=points.device)
        N.check(N.lib().surfd_voxel_points(N.ptr(points), points.shape[0], bounds[0], bounds[1], R, N.ptr(grid.packed), N.ptr(outside), N.stream()))
    if return_counts:
        return grid, {"outside": int(outside.item())}
    return grid


# ---- IoU --------------------------------------------------------------------------------------------------------------------------
Grids = Union[VoxelGrid, Sequence[VoxelGrid], Tensor]


def _batch(g: Grids):
    """-> (int32 [B, R, R, W], R, the grids' bounds or None for a packed batch, which carries none)"""
    if isinstance(g, VoxelGrid):
        g = [g]
    if isinstance(g, Tensor):
        if g.dtype != torch.int32 or g.dim() != 4 or g.shape[1] != g.shape[2] or g.shape[3] != words(g.shape[1]):
            raise ValueError(f"a packed batch must be int32 [B, R, R, ceil(R / 32)], got {g.dtype} {tuple(g.shape)}")
        _no_cpu(g, "voxel_iou")
        return g.contiguous(), g.shape[1], None
    g = list(g)
    if not g or not all(isinstance(x, VoxelGrid) for x in g):
        raise TypeError("expected a VoxelGrid, a non-empty sequence of them or a packed batch")
    if len({(x.resolution, x.bounds) for x in g}) != 1:
        raise ValueError("the grids differ in resolution or bounds")
    for x in g:
        _no_cpu(x.packed, "voxel_iou")
    return torch.stack([x.packed for x in g]), g[0].resolution, g[0].bounds


def _iou(a: Tensor, b: Tensor, R: int, paired: bool):
    M, Nb = a.shape[0], b.shape[0]
    _no_cpu(a, "voxel_iou")
    _no_cpu(b, "voxel_iou")
    shape = (M,) if paired else (M, Nb)
    with torch.cuda.device(a.device):
        inter = torch.empty(shape, dtype=torch.int32, device=a.device)
        union = torch.empty(shape, dtype=torch.int32, device=a.device)
        iou = torch.empty(shape, dtype=torch.float32, device=a.device)
        N.check(N.lib().surfd_voxel_iou(N.ptr(a), M, N.ptr(b), Nb, R, int(paired), N.ptr(inter), N.ptr(union), N.ptr(iou), N.stream()))
    return inter, union, iou


def _pair(a: Grids, b: Grids):
    ta, Ra, ba = _batch(a)
    tb, Rb, bb = _batch(b)
    if Ra != Rb:
        raise ValueError(f"resolutions differ: {Ra} and {Rb}")
    if ba is not None and bb is not None and ba != bb:
        raise ValueError(f"bounds differ: {ba} and {bb}")
    if ta.device != tb.device:
        raise ValueError(f"a is on {ta.device}, b on {tb.device}")
    return ta, tb, Ra


def voxel_iou(a: Grids, b: Grids, return_counts: bool = False):
    """Paired IoU: grid m of ``a`` against grid m of ``b`` -> float32 [B] (a 0-d tensor for two single VoxelGrids); 1.0 where
    both are empty.  With ``return_counts`` -> (iou, intersection, union), the counts int32."""
    ta, tb, R = _pair(a, b)
    if ta.shape[0] != tb.shape[0]:
        raise ValueError(f"paired IoU needs as many grids in a as in b, got {ta.shape[0]} and {tb.shape[0]}")
    inter, union, iou = _iou(ta, tb, R, True)
    if isinstance(a, VoxelGrid) and isinstance(b, VoxelGrid):
        inter, union, iou = inter[0], union[0], iou[0]
    return (iou, inter, union) if return_counts else iou


def voxel_iou_matrix(a_set: Grids, b_set: Grids, return_counts: bool = False):
    """IoU of every grid of ``a_set`` against every grid of ``b_set`` -> float32 [M, N]; an entry has the same bits whatever M
    and N it is computed in."""
    ta, tb, R = _pair(a_set, b_set)
    inter, union, iou = _iou(ta, tb, R, False)
    return (iou, inter, union) if return_counts else iou


def is_closed(vertices: Tensor, faces: Tensor, resolution: int = 64, bounds=(-1.0, 1.0)) -> bool:
    """True when no column of the grid is crossed an odd number of times: the snapped mesh is closed as far as the
    resolution's columns can tell (a hole that no column centre passes through goes unseen)"""
    return voxelize_solid(vertices, faces, resolution, bounds, include_surface=False)[1] == 0
