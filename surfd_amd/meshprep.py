"""Mesh preprocessing on the MI355X path: mesh -> (surface cloud, query points, UDF labels, gradients), and the distance of
points or meshes to a mesh.  The counterparts of the reference's open3d-based data preparation:

  read_mesh                  <- AutoEncoder/utils.py:13-38               (OBJ only)
  sample_points_uniformly    <- open3d TriangleMesh.sample_points_uniformly as used at utils.py:280, preprocess_udfs.py:126
  sample_points_with_normals no counterpart: the same draw as sample_points_uniformly, with the face normal of every point
  sample_points_evenly       no counterpart: open3d's sample_points_poisson_disk; uniform candidates + cloudsample.farthest_point_sampling
  sample_points_around_pcd   <- AutoEncoder/utils.py:167-220             (same RNG calls in the same order)
  closest_points, MeshDistance <- open3d RaycastingScene.compute_closest_points (utils.py:228-234)
  compute_udf_and_gradients  <- AutoEncoder/utils.py:223-240
  compute_udf_from_mesh      <- AutoEncoder/utils.py:268-314
  compute_sdf_and_gradients  <- AutoEncoder/utils.py:242-264             (the sign comes from surfd_amd/raycast.py, or with
                                                                          sign="winding" from surfd_amd/winding.py)
  compute_sdf_from_mesh      <- AutoEncoder/utils.py:317-363
  is_inside                  no counterpart: open3d's RaycastingScene.compute_occupancy as a bool
  point_to_mesh_distance, mesh_distance   no counterpart: how far a reconstruction is from the mesh it came from

Where the reference takes an open3d mesh (``mesh_o3d``) these take ``(vertices [V, 3] float32, triangles [F, 3] integer)``.
The closest-point search runs in csrc/meshdist.hip and nowhere else: device tensors in, device tensors out, CPU tensors are
refused (no CPU fallback).  The two samplers and read_mesh are plain torch / file plumbing and work on any device.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from . import _native as N


# ---- files --------------------------------------------------------------------------------------------------------------------
def read_mesh(mesh_path, dtype: torch.dtype = torch.float) -> Tuple[Tensor, Tensor]:
    """OBJ file -> (vertices [V, 3] ``dtype``, triangles [F, 3] int64).  Reads ``v x y z [...]`` and ``f`` lines whose corners
    are ``v``, ``v/vt``, ``v/vt/vn`` or ``v//vn`` with positive (1-based) or negative (relative to the vertices read so far)
    indices; polygons are fan-triangulated; every other line is ignored."""
    mesh_path = str(mesh_path)
    if not os.path.exists(mesh_path):
        raise ValueError(f"The mesh file {mesh_path} does not exists.")
    if not mesh_path.lower().endswith(".obj"):
        raise ValueError(f"read_mesh reads OBJ files only, got {mesh_path}")
    verts: List[List[float]] = []
    tris: List[List[int]] = []
    with open(mesh_path) as fh:
        for ln, line in enumerate(fh, 1):
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                if len(parts) < 4:
                    raise ValueError(f"{mesh_path}:{ln}: a vertex needs three coordinates")
                verts.append([float(parts[1]), float(parts[2]), float(parts[3])])
            elif parts[0] == "f":
                corner = []
                for tok in parts[1:]:
                    k = int(tok.split("/")[0])
                    k = k - 1 if k > 0 else len(verts) + k
                    if k < 0 or k >= len(verts):
                        raise ValueError(f"{mesh_path}:{ln}: face corner '{tok}' names a vertex that does not exist")
                    corner.append(k)
                if len(corner) < 3:
                    raise ValueError(f"{mesh_path}:{ln}: a face needs three corners")
                for i in range(1, len(corner) - 1):
                    tris.append([corner[0], corner[i], corner[i + 1]])
    v = torch.tensor(verts, dtype=torch.float64).reshape(-1, 3).to(dtype)
    t = torch.tensor(tris, dtype=torch.long).reshape(-1, 3)
    return v, t


# ---- checks -------------------------------------------------------------------------------------------------------------------
def _check_mesh(vertices: Tensor, triangles: Tensor, need_cuda: bool = True, what: str = "the mesh distance") -> None:
    """shapes and dtypes first, the CPU-tensor refusal last"""
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.shape[0] < 1:
        raise ValueError(f"vertices must be [V, 3] with V >= 1, got {tuple(vertices.shape)}")
    if vertices.dtype != torch.float32:
        raise TypeError(f"vertices must be float32, got {vertices.dtype}")
    if triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.shape[0] < 1:
        raise ValueError(f"triangles must be [F, 3] with F >= 1, got {tuple(triangles.shape)}")
    if triangles.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"triangles must be int32 or int64, got {triangles.dtype}")
    if need_cuda and not (vertices.is_cuda and triangles.is_cuda):
        raise RuntimeError(f"{what} runs only on the GPU through libsurfd_hip.so (no CPU fallback): move the mesh with .cuda()")


def _check_points(name: str, p: Tensor, need_cuda: bool = True) -> None:
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"{name} must be [N, 3], got {tuple(p.shape)}")
    if p.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {p.dtype}")
    if need_cuda and not p.is_cuda:
        raise RuntimeError(f"the mesh distance runs only on the GPU through libsurfd_hip.so (no CPU fallback): move {name} with .cuda()")


# ---- Morton order -------------------------------------------------------------------------------------------------------------
def _spread10(x: Tensor) -> Tensor:
    x = x & 0x3FF
    x = (x | (x << 16)) & 0x030000FF
    x = (x | (x << 8)) & 0x0300F00F
    x = (x | (x << 4)) & 0x030C30C3
    x = (x | (x << 2)) & 0x09249249
    return x


def morton_order(p: Tensor) -> Tensor:
    """the permutation that sorts the points [N, 3] by 30-bit Morton code over their own bounding box (stable)"""
    lo = p.min(0).values
    ext = (p.max(0).values - lo).max().clamp_min(1e-30)
    g = ((p - lo) / ext * 1023.0).clamp(0, 1023).long()
    code = _spread10(g[:, 0]) | (_spread10(g[:, 1]) << 1) | (_spread10(g[:, 2]) << 2)
    return torch.sort(code, stable=True).indices


# ---- closest point ------------------------------------------------------------------------------------------------------------
ACCELS = ("tiles", "bvh")
MESH_BRUTE_FORCE = 1
MESH_COUNT_VISITS = 2


def _check_accel(accel: str) -> None:
    if accel not in ACCELS:
        raise ValueError(f"accel must be 'tiles' or 'bvh', got {accel!r}")


class _MeshScene:
    """What the objects that keep one mesh in the library share (MeshDistance, RaycastingScene, WindingScene,
    IntersectionScene): the handle and its device, ``num_triangles``, the counters the last call left, and ``_open``, the
    constructors' common work.  ``_abi`` is the prefix of the library's functions for the handle."""

    _abi = ""
    _handle = None
    _perm: Optional[Tensor] = None                  # handle index -> the caller's triangle index; None: the caller's order
    last_skipped_tiles: Optional[int] = None
    last_total_tiles: Optional[int] = None
    last_box_tests: Optional[int] = None
    last_pair_tests: Optional[int] = None

    def _fn(self, name: str):
        return getattr(N.lib(), f"{self._abi}_{name}")

    def _open(self, vertices: Tensor, triangles: Tensor, what: str = "the mesh distance", check_values: bool = True,
              morton: bool = True, prepare=None, extra=None) -> Tuple[Tensor, Tensor]:
        """Checks the mesh, hands it to the library's create and returns (vertices, int64 triangles) as the caller ordered
        them.  ``extra()`` gives create's further arguments and runs right after the shape checks.  ``check_values``: the
        finiteness and index-range checks (three host syncs); without them a NaN or a bad index reaches the library, which
        refuses it.  ``prepare(v, t)`` may replace the triangles.  ``morton``: the library gets the triangles in Morton order
        of their centroids and ``_perm`` maps its indices back."""
        _check_mesh(vertices, triangles, what=what)
        args = extra() if extra is not None else ()
        if check_values and not bool(torch.isfinite(vertices).all()):
            raise ValueError("vertices contain NaN or Inf")
        v, t = vertices.contiguous(), triangles.long()
        if check_values and (int(t.min()) < 0 or int(t.max()) >= v.shape[0]):
            raise ValueError(f"triangles name vertices outside [0, {v.shape[0]})")
        if prepare is not None:
            t = prepare(v, t)
        self.device = v.device
        self.num_triangles = int(t.shape[0])
        ts = t
        if morton:                                   # the order only decides how compact the tiles are
            corners = v[t] if check_values else torch.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)[t.clamp(0, v.shape[0] - 1)]
            self._perm = morton_order(corners.mean(1))
            ts = t[self._perm]
        ts = ts.to(torch.int32).contiguous()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._fn("create")(N.ptr(v), v.shape[0], N.ptr(ts), ts.shape[0], *args, N.stream(), C.byref(h)))
        self._handle = h
        assert self._fn("num_triangles")(h) == self.num_triangles
        return v, t

    def _read_counters(self, name: str) -> Tuple[int, int]:
        """the two int64 that the library's ``name`` reads back ("visits", "skipped"): one host sync"""
        a, b = C.c_int64(), C.c_int64()
        N.check(self._fn(name)(self._handle, C.byref(a), C.byref(b), N.stream()))
        return int(a.value), int(b.value)

    def __del__(self):
        try:
            if self._handle is not None:
                self._fn("destroy")(self._handle)
        except Exception:                                       # interpreter shutdown
            pass


class _BvhScene(_MeshScene):
    """a scene that can carry the box hierarchy of csrc/meshbvh.hip (``accel="bvh"``)"""

    def _set_accel(self, accel: str) -> None:
        self.accel = accel
        if accel == "bvh":
            with torch.cuda.device(self.device):
                N.check(self._fn("build_bvh")(self._handle, N.stream()))

    def read_bvh(self) -> dict:
        """the hierarchy (``accel="bvh"`` only) as the library holds it, for tests: {"level_sizes": [levels] ints (level 0 = the
        nodes above the leaves), "boxes": [nodes, 6, 4] float32 (lo.xyz, hi.xyz of a node's 4 children), "leaves": [leaves, 4]
        int32 (the HANDLE's triangle indices, -1 past the end), "perm": handle index -> the caller's}, on the device"""
        levels, leaves, nodes = C.c_int(), C.c_int(), C.c_int()
        sizes = (C.c_int32 * 16)()
        N.check(self._fn("bvh_info")(self._handle, C.byref(levels), C.byref(leaves), C.byref(nodes), sizes, 16))
        boxes = torch.empty(nodes.value, 6, 4, device=self.device, dtype=torch.float32)
        tri = torch.empty(leaves.value, 4, device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            N.check(self._fn("bvh_read")(self._handle, N.ptr(boxes), N.ptr(tri), N.stream()))
        return {"level_sizes": [int(sizes[k]) for k in range(levels.value)], "boxes": boxes, "leaves": tri, "perm": self._perm}


class MeshDistance(_BvhScene):
    """The closest-point structure of one mesh, kept for repeated calls (the role of open3d's RaycastingScene).

    The triangles are handed to the library in Morton order of their centroids and every call's queries in Morton order of
    their positions, so that a wave's queries and a tile's triangles are each compact and the kernel's culling bites; results
    come back in the caller's order with the caller's triangle indices.  Ties in distance go to the triangle that comes first
    in the Morton order.  Host syncs: the constructor checks the vertices and the index range (three) and the library's create
    reads its bad-index flag (one); every ``closest`` call checks that the queries are finite (one).  One stream at a time per
    object: the library keeps its partial results in a workspace of the handle.

    ``accel="bvh"`` also builds the box hierarchy of csrc/meshbvh.hip (one more host sync); ``closest`` then walks it instead of
    the tiles unless ``brute_force=True``.  The results are the same bits either way."""

    _abi = "surfd_mesh"

    def __init__(self, vertices: Tensor, triangles: Tensor, accel: str = "tiles"):
        _check_accel(accel)
        self._open(vertices, triangles)
        self._set_accel(accel)

    def closest(self, queries: Tensor, brute_force: bool = False, count_skipped: bool = False,
                count_visits: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
        """queries [Q, 3] -> (dist [Q] float32, points [Q, 3] float32, tri [Q] int64).  ``brute_force`` tests every pair (the
        correctness baseline; the same bits).  With ``count_skipped`` the number of (wave, tile) visits that culling skipped is
        left in ``last_skipped_tiles`` and their total in ``last_total_tiles`` (one host sync).  With ``count_visits``
        (``accel="bvh"``) the box tests and pair tests of the call, summed over the queries, are left in ``last_box_tests`` and
        ``last_pair_tests`` (one host sync)."""
        use_bvh = self.accel == "bvh" and not brute_force
        if count_visits and not use_bvh:
            raise ValueError("count_visits counts the hierarchy's tests: it needs accel='bvh' and not brute_force")
        _check_points("queries", queries)
        if queries.device != self.device:
            raise RuntimeError(f"queries are on {queries.device}, the mesh is on {self.device}")
        Q = queries.shape[0]
        dist = torch.empty(Q, device=self.device, dtype=torch.float32)
        pts = torch.empty(Q, 3, device=self.device, dtype=torch.float32)
        tri = torch.empty(Q, device=self.device, dtype=torch.int32)
        if Q == 0:
            return dist, pts, tri.long()
        if not bool(torch.isfinite(queries).all()):
            raise ValueError("queries contain NaN or Inf")
        order = morton_order(queries)
        qs = queries[order].contiguous()
        skipped = torch.zeros(1, device=self.device, dtype=torch.int64) if count_skipped else None
        with torch.cuda.device(self.device):
            if use_bvh:
                N.check(N.lib().surfd_mesh_closest_bvh(self._handle, N.ptr(qs), Q, MESH_COUNT_VISITS if count_visits else 0, N.ptr(dist),
                                                       N.ptr(pts), N.ptr(tri), N.ptr(skipped), N.stream()))
                if count_visits:
                    self.last_box_tests, self.last_pair_tests = self._read_counters("visits")
            else:
                N.check(N.lib().surfd_mesh_closest(self._handle, N.ptr(qs), Q, MESH_BRUTE_FORCE if brute_force else 0, N.ptr(dist),
                                                   N.ptr(pts), N.ptr(tri), N.ptr(skipped), N.stream()))
        if count_skipped:
            self.last_skipped_tiles = int(skipped.item())
            self.last_total_tiles = ((Q + 63) // 64) * ((self.num_triangles + 31) // 32)
        inv = torch.empty_like(order)
        inv[order] = torch.arange(Q, device=self.device)
        return dist[inv], pts[inv], self._perm[tri.long()][inv]


def closest_points(vertices: Tensor, triangles: Tensor, queries: Tensor, brute_force: bool = False,
                   accel: str = "tiles") -> Tuple[Tensor, Tensor, Tensor]:
    """(dist [Q], points [Q, 3], tri [Q]): for every query the exact closest point of the mesh, its distance and its triangle.
    ``accel``: "tiles" or "bvh" (MeshDistance); the same bits."""
    _check_accel(accel)
    _check_mesh(vertices, triangles, need_cuda=False)          # shapes and dtypes first, the CPU-tensor refusal last
    _check_points("queries", queries, need_cuda=False)
    _check_mesh(vertices, triangles)
    _check_points("queries", queries)
    return MeshDistance(vertices, triangles, accel=accel).closest(queries, brute_force=brute_force)


# ---- samplers (torch plumbing) ------------------------------------------------------------------------------------------------
def sample_points_uniformly(vertices: Tensor, triangles: Tensor, number_of_points: int, generator: Optional[torch.Generator] = None) -> Tensor:
    """``number_of_points`` points uniform on the surface: a triangle drawn with probability proportional to its area, then
    (1 - sqrt(r1)) a + sqrt(r1) (1 - r2) b + sqrt(r1) r2 c.  The random numbers come from ``generator`` (or the global RNG) of
    the mesh's device."""
    _check_mesh(vertices, triangles, need_cuda=False)
    if number_of_points < 0:
        raise ValueError("number_of_points must not be negative")
    t = triangles.long()
    a, b, c = vertices[t[:, 0]], vertices[t[:, 1]], vertices[t[:, 2]]
    area = torch.linalg.cross((b - a).double(), (c - a).double()).norm(dim=1)
    if not float(area.sum()) > 0:
        raise ValueError("the mesh has no area to sample")
    dev = vertices.device
    pick = torch.multinomial(area / area.sum(), number_of_points, replacement=True, generator=generator) if number_of_points else \
        torch.empty(0, dtype=torch.long, device=dev)
    r = torch.rand(number_of_points, 2, device=dev, generator=generator).double()
    s = r[:, 0].sqrt()[:, None]
    r2 = r[:, 1][:, None]
    # the combination in fp64, rounded once: the point is off its triangle by half an ulp per coordinate at most
    return ((1 - s) * a[pick].double() + s * (1 - r2) * b[pick].double() + s * r2 * c[pick].double()).float()


def sample_points_with_normals(vertices: Tensor, triangles: Tensor, n: int,
                               generator: Optional[torch.Generator] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """``n`` points uniform on the surface with the normal of the triangle each was drawn on -> (points [n, 3] float32, normals
    [n, 3] float32, tri [n] int64: the triangle of every point).  The same random calls in the same order as
    ``sample_points_uniformly``: for the same generator state the points are the same bits.  A face normal is
    (b - a) x (c - a) / |(b - a) x (c - a)| in fp64, rounded once to float32; its sign follows the winding; a triangle without
    area has the zero normal (and, with probability 0, is never drawn)."""
    _check_mesh(vertices, triangles, need_cuda=False)
    if n < 0:
        raise ValueError("n must not be negative")
    t = triangles.long()
    a, b, c = vertices[t[:, 0]], vertices[t[:, 1]], vertices[t[:, 2]]
    cross = torch.linalg.cross((b - a).double(), (c - a).double())
    area = cross.norm(dim=1)
    if not float(area.sum()) > 0:
        raise ValueError("the mesh has no area to sample")
    dev = vertices.device
    pick = torch.multinomial(area / area.sum(), n, replacement=True, generator=generator) if n else \
        torch.empty(0, dtype=torch.long, device=dev)
    r = torch.rand(n, 2, device=dev, generator=generator).double()
    s = r[:, 0].sqrt()[:, None]
    r2 = r[:, 1][:, None]
    points = ((1 - s) * a[pick].double() + s * (1 - r2) * b[pick].double() + s * r2 * c[pick].double()).float()
    length = (cross * cross).sum(1, keepdim=True).sqrt()
    face_normals = torch.where(length > 0, cross / torch.where(length > 0, length, torch.ones_like(length)), torch.zeros_like(cross)).float()
    return points, face_normals[pick], pick


def sample_points_evenly(vertices: Tensor, triangles: Tensor, number_of_points: int, init_factor: int = 5,
                         generator: Optional[torch.Generator] = None) -> Tensor:
    """``number_of_points`` points that cover the surface evenly, [K, 3]: ``sample_points_uniformly(init_factor * K)`` as the
    candidates (already in random order), then farthest point sampling down to K from candidate 0 (surfd_amd/cloudsample.py,
    csrc/cloudfps.hip).  The counterpart of open3d's ``sample_points_poisson_disk(number_of_points, init_factor=5)``.  The mesh
    may live on any device: the candidates are drawn on the mesh's device with ``generator`` (so a CPU mesh and a CPU generator
    give the same candidates as ``sample_points_uniformly``), moved to the GPU for the farthest point sampling, which has no
    CPU path, and the result is moved back to the mesh's device.  ``init_factor = 1`` returns the candidates reordered."""
    from .cloudsample import farthest_point_sampling
    if number_of_points < 1:
        raise ValueError("number_of_points must be positive")
    if isinstance(init_factor, bool) or not isinstance(init_factor, int) or init_factor < 1:
        raise ValueError(f"init_factor must be a positive int, got {init_factor}")
    candidates = sample_points_uniformly(vertices, triangles, init_factor * number_of_points, generator=generator)
    on_gpu = candidates.cuda().contiguous()
    idx, _ = farthest_point_sampling(on_gpu[None], number_of_points)
    return on_gpu[idx[0]].to(vertices.device)


def sample_points_around_pcd(pcd: Tensor, stds: List[float], num_points_per_std: List[int], coords_range: Tuple[float, float],
                             device: str = "cpu") -> Tensor:
    """AutoEncoder/utils.py:167-220: the cloud's points (repeated, then a random remainder drawn without replacement) plus
    Gaussian offsets for every sigma, then ``num_points_per_std[-1]`` uniform points; clipped to ``coords_range``.  The random
    draws are the reference's, in its order: per sigma one multinomial on ``device`` (only where a remainder is needed) and one
    randn on the host, at the end one rand on the host; so a seeded run gives the reference's bits (tests/golden g19)."""
    n = pcd.shape[0]
    lo, hi = coords_range
    cloud = pcd.to(device)
    blocks = []
    for sigma, count in zip(stds, num_points_per_std[:-1]):
        reps, rest = divmod(count, n)
        rows = torch.arange(n, device=device).repeat_interleave(reps)           # every point `reps` times in a row
        if rest:                                                                # then `rest` distinct points, drawn on `device`
            rows = torch.cat((rows, torch.multinomial(torch.ones(n, device=device), rest, replacement=False)))
        blocks.append(cloud[rows] + torch.randn(count, 3).to(device) * sigma)  # the noise is drawn on the host, then moved
    blocks.append(torch.rand(num_points_per_std[-1], 3).to(device) * (hi - lo) + lo)
    return torch.cat(blocks).clamp(lo, hi)


# ---- UDF labels ---------------------------------------------------------------------------------------------------------------
def _as_mesh_distance(vertices, triangles, accel: str = "tiles") -> MeshDistance:
    """a given MeshDistance (triangles None; it keeps its own ``accel``), or a new one"""
    _check_accel(accel)
    return vertices if isinstance(vertices, MeshDistance) and triangles is None else MeshDistance(vertices, triangles, accel=accel)


def compute_udf_and_gradients(vertices: Tensor, triangles: Tensor, queries: Tensor, accel: str = "tiles") -> Tuple[Tensor, Tensor]:
    """AutoEncoder/utils.py:223-240: udf = |q - c| and gradients = F.normalize(q - c) for the closest point c of the mesh (a
    query on the surface gets a zero gradient through F.normalize's eps).  ``vertices`` may be a MeshDistance (triangles None).
    ``accel``: how a new MeshDistance searches ("tiles" or "bvh"; the same bits)."""
    offset = queries - _as_mesh_distance(vertices, triangles, accel).closest(queries)[1]
    return offset.norm(dim=-1), F.normalize(offset, dim=-1)


def compute_udf_from_mesh(vertices: Tensor, triangles: Tensor, num_surface_points: int = 100_000, num_queries_on_surface: int = 10_000,
                          queries_stds: List[float] = [0.003, 0.01, 0.1], num_queries_per_std: List[int] = [5_000, 4_000, 500, 500],
                          coords_range: Tuple[float, float] = (-1.0, 1.0), max_dist: float = 0.1, convert_to_bce_labels: bool = False,
                          use_cuda: bool = True, input_queries: Optional[Tensor] = None,
                          accel: str = "tiles") -> Tuple[Tensor, Tensor, Tensor]:
    """AutoEncoder/utils.py:268-314 -> (queries, values, gradients): a surface cloud, queries around it (or ``input_queries``),
    their UDF clipped to [0, max_dist] and its gradients.  Everything stays on the mesh's device (the reference moves the queries
    to the CPU for open3d); ``num_queries_on_surface`` and ``convert_to_bce_labels`` are unused, as in the reference.
    ``accel``: "tiles" or "bvh" (MeshDistance); the same random numbers and the same bits."""
    _check_accel(accel)
    _check_mesh(vertices, triangles)
    if not use_cuda:
        raise RuntimeError("compute_udf_from_mesh runs only on the GPU through libsurfd_hip.so (no CPU fallback)")
    queries = input_queries
    if queries is None:
        cloud = sample_points_uniformly(vertices, triangles, num_surface_points)
        queries = sample_points_around_pcd(cloud, queries_stds, num_queries_per_std, coords_range, vertices.device)
    udf, gradients = compute_udf_and_gradients(vertices, triangles, queries, accel=accel)
    return queries, udf.clamp(0, max_dist), gradients


# ---- SDF labels ---------------------------------------------------------------------------------------------------------------
SIGN_METHODS = ("parity", "winding")


def _check_method(name: str, method: str) -> None:
    if method not in SIGN_METHODS:
        raise ValueError(f"{name} must be 'parity' or 'winding', got {method!r}")


def _as_scene(vertices, triangles, method: str = "parity", accel: str = "tiles", orient=False):
    """the scene that answers inside / outside by ``method``: a given one of that kind (triangles None), or a new one.  ``accel``
    goes to a new RaycastingScene and its mesh_distance(); a WindingScene has no hierarchy and ignores it.  ``orient`` goes to a new
    WindingScene (a given scene keeps the orientation it was made with); the parity does not depend on the winding."""
    from .raycast import RaycastingScene
    from .winding import WindingScene
    _check_accel(accel)
    kind, other = (RaycastingScene, WindingScene) if method == "parity" else (WindingScene, RaycastingScene)
    if isinstance(vertices, other) and triangles is None:
        raise TypeError(f"a {other.__name__} cannot answer by {method!r}: pass a {kind.__name__} or the mesh itself")
    if isinstance(vertices, kind) and triangles is None:
        return vertices
    if orient is not False and method != "winding":
        raise ValueError("orient belongs to the winding number: the crossing parity does not depend on the faces' winding")
    return RaycastingScene(vertices, triangles, accel=accel) if kind is RaycastingScene else kind(vertices, triangles, orient=orient)


def is_inside(vertices: Tensor, triangles: Tensor, points: Tensor, nsamples: int = 1, method: str = "parity",
              accel: str = "tiles", orient=False) -> Tensor:
    """[N] bool: is the point inside the mesh.  ``method="parity"``: the parity of the number of crossings of the ray from the
    point along +z (csrc/raycast.hip); ``nsamples=3`` also asks +x and +y and takes the majority.  The parity means something on a
    closed mesh only (surfd_amd/raycast.py, ``compute_occupancy(..., return_votes=True)`` tells); on a mesh with holes use
    ``method="winding"``: |winding number| >= 1/2 (surfd_amd/winding.py), which needs consistently oriented faces instead and
    takes no ``nsamples``.  ``vertices`` may be a RaycastingScene, or a WindingScene for "winding" (triangles None).
    ``accel``: how a new RaycastingScene casts ("tiles" or "bvh"; the same answers).  ``orient`` (method="winding" only): True or
    "outward" re-orients the faces first (surfd_amd/meshtopo.py), for meshes whose faces are not consistently oriented."""
    from .raycast import RaycastingScene, _check_nsamples
    from .winding import WindingScene
    _check_method("method", method)
    _check_accel(accel)
    if not (isinstance(vertices, (RaycastingScene, WindingScene)) and triangles is None):
        _check_mesh(vertices, triangles, need_cuda=False)      # shapes and dtypes first, the CPU-tensor refusal last
    _check_points("points", points, need_cuda=False)
    _check_nsamples(nsamples)
    if method == "winding":
        if nsamples != 1:
            raise ValueError("nsamples belongs to method='parity': the winding number casts no rays")
        return _as_scene(vertices, triangles, method, orient=orient).compute_occupancy(points) > 0
    return _as_scene(vertices, triangles, accel=accel, orient=orient).compute_occupancy(points, nsamples) > 0


def compute_sdf_and_gradients(vertices: Tensor, triangles: Tensor, queries: Tensor, sign: str = "parity",
                              accel: str = "tiles", orient=False) -> Tuple[Tensor, Tensor]:
    """AutoEncoder/utils.py:242-264: sdf = the distance to the mesh, negative inside (open3d's compute_signed_distance: the
    parity of the crossings along +z), and gradients = sign(sdf) * F.normalize(q - c) for the closest point c of the mesh.  A
    query on the surface has sdf 0 and a zero gradient.  ``sign="winding"`` takes inside / outside from the winding number
    instead (surfd_amd/winding.py: for meshes with holes).  ``vertices`` may be a RaycastingScene, or a WindingScene for
    "winding" (triangles None).  ``accel``: how a new RaycastingScene casts and measures ("tiles" or "bvh"; the same bits);
    with ``sign="winding"`` it is ignored, a WindingScene has no hierarchy.  ``orient`` (sign="winding" only): as in is_inside."""
    _check_method("sign", sign)
    scene = _as_scene(vertices, triangles, sign, accel, orient=orient)
    sdf = scene.compute_signed_distance(queries)
    offset = queries - scene.mesh_distance().closest(queries)[1]
    return sdf, torch.sign(sdf)[:, None] * F.normalize(offset, dim=-1)


def compute_sdf_from_mesh(vertices: Tensor, triangles: Tensor, num_surface_points: int = 100_000, num_queries_on_surface: int = 10_000,
                          queries_stds: List[float] = [0.003, 0.01, 0.1], num_queries_per_std: List[int] = [5_000, 4_000, 500, 500],
                          coords_range: Tuple[float, float] = (-1.0, 1.0), max_dist: float = 0.1, convert_to_bce_labels: bool = False,
                          use_cuda: bool = True, input_queries: Optional[Tensor] = None,
                          sign: str = "parity", accel: str = "tiles", orient=False) -> Tuple[Tensor, Tensor, Tensor]:
    """AutoEncoder/utils.py:317-363 -> (queries, values, gradients): a surface cloud, queries around it (or ``input_queries``),
    their SDF clipped to [-max_dist, max_dist] and its gradients; in front of them ``num_queries_on_surface`` points drawn on the
    surface with value 0 and gradient 0.  ``convert_to_bce_labels`` turns the values into 1 - values / max_dist, as the
    reference does.  Everything stays on the mesh's device and the random numbers come from that device's global RNG, as in
    compute_udf_from_mesh.  ``sign``: "parity" (the reference's) or "winding", as in compute_sdf_and_gradients; the same
    random numbers are drawn either way.  ``accel`` and ``orient``: as in compute_sdf_and_gradients."""
    _check_method("sign", sign)
    _check_accel(accel)
    _check_mesh(vertices, triangles)
    if not use_cuda:
        raise RuntimeError("compute_sdf_from_mesh runs only on the GPU through libsurfd_hip.so (no CPU fallback)")
    queries = input_queries
    if queries is None:
        cloud = sample_points_uniformly(vertices, triangles, num_surface_points)
        queries = sample_points_around_pcd(cloud, queries_stds, num_queries_per_std, coords_range, vertices.device)
    sdf, gradients = compute_sdf_and_gradients(vertices, triangles, queries, sign, accel=accel, orient=orient)
    values = sdf.clamp(-max_dist, max_dist)
    on_surface = sample_points_uniformly(vertices, triangles, num_queries_on_surface)
    queries = torch.cat([on_surface, queries], dim=0)
    values = torch.cat([torch.zeros(num_queries_on_surface, device=values.device, dtype=values.dtype), values], dim=0)
    gradients = torch.cat([torch.zeros(num_queries_on_surface, 3, device=gradients.device, dtype=gradients.dtype), gradients], dim=0)
    if convert_to_bce_labels:
        values = 1 - values / max_dist
    return queries, values, gradients


# ---- measurement --------------------------------------------------------------------------------------------------------------
def point_to_mesh_distance(points: Tensor, vertices: Tensor, triangles: Tensor, accel: str = "tiles") -> Tensor:
    """[N] exact distances of the points to the mesh (``vertices`` may be a MeshDistance, triangles None).  ``accel``: how a new
    MeshDistance searches ("tiles" or "bvh"; the same bits)."""
    return _as_mesh_distance(vertices, triangles, accel).closest(points)[0]


def mesh_distance(v1: Tensor, t1: Tensor, v2: Tensor, t2: Tensor, n: int = 100_000, generator: Optional[torch.Generator] = None,
                  accel: str = "tiles") -> dict:
    """The two directed mean distances between two meshes and their sum: ``n`` points sampled on the surface of one mesh,
    exact distance to the other.  {"d12": mesh 1 -> mesh 2, "d21": mesh 2 -> mesh 1, "sum": d12 + d21}.  ``accel``: "tiles" or
    "bvh" (MeshDistance); the same numbers."""
    _check_accel(accel)
    _check_mesh(v1, t1)
    _check_mesh(v2, t2)
    p1 = sample_points_uniformly(v1, t1, n, generator=generator)
    p2 = sample_points_uniformly(v2, t2, n, generator=generator)
    d12 = float(point_to_mesh_distance(p1, v2, t2, accel=accel).double().mean())
    d21 = float(point_to_mesh_distance(p2, v1, t1, accel=accel).double().mean())
    return {"d12": d12, "d21": d21, "sum": d12 + d21}
