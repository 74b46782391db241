"""Isotropic remeshing on the MI355X path: the incremental algorithm of Botsch and Kobbelt (2004) to a target edge length L, as
rounds of independent operations on the device.  One iteration splits the edges longer than ``high`` L, collapses those shorter
than ``low`` L, flips edges towards valence 6 (4 on a border) and relaxes the vertices in their tangent planes; with
``project=True`` the vertices that moved are put back onto the INPUT surface after every iteration (the exact closest point,
surfd_amd.meshprep.MeshDistance).  A mesh that lies on the device is remeshed there:

  remesh_isotropic    (vertices, faces[, origin][, stats])
  MeshRemesher        the handle behind it: iterate / positions / emit, for callers that step themselves
  mean_edge_length, triangle_quality      plain torch, outside the contract: a length to ask for and what came of it

tests/meshremesh_ref.py restates the contract sequentially in numpy: every result equals it bit for bit and in the same order
(vertex order, face order, every double, ``origin`` and every count).  The work runs in csrc/meshremesh.hip and nowhere else:
device tensors in, device tensors out, CPU tensors are refused (no CPU fallback).  Vertices are float64 [V, 3] (float32 is widened
exactly), faces int64 [F, 3] (int32 is accepted); vertices come back float64 and faces int64.  Limits: 3 F < 2^31 at any time;
an index outside [0, V) is the library's SURFD_ERR_ARG (a RuntimeError), found on the device and never a fault.  A call works on
the current stream; one stream at a time per handle.

What it keeps: the operations are those of an edge-collapse decimation (surfd_amd.meshsimplify) plus splits and flips that change
no topology, so manifold input stays manifold, borders stay borders (their vertices do not relax; a border edge collapses to its
midpoint, so border corners are cut), components and the Euler characteristic stay, and no face turns against the normal it had
in the input by more than ``flip_cos`` allows.  Out of scope: adaptive (curvature-driven) sizing, feature and crease
preservation, area-weighted centroids, any guarantee that simultaneous relax moves cannot fold a face (each vertex is tested
against its neighbours' old positions), attributes beyond ``origin``, batches of meshes in one launch.

Host syncs: 1 to 2 per round of every stage, 1 per iteration, 1 per emit; ``project`` adds those of MeshDistance.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch
from torch import Tensor

from . import _native as N
from .meshclean import _counts, _mesh

STAT_NAMES = ("vertices", "faces", "splits", "collapses", "border_collapses", "flips", "relaxed", "relax_refused", "split_rounds",
              "collapse_rounds", "flip_rounds", "split_marked", "collapse_refused_valence", "collapse_refused_link",
              "collapse_refused_border", "collapse_refused_opposite", "collapse_refused_long", "collapse_refused_flip",
              "flip_refused_orient", "flip_refused_same", "flip_refused_edge", "flip_refused_degree", "flip_refused_long",
              "flip_refused_fold")


def _rounds(name: str, value) -> int:
    if int(value) != value or value < 0:
        raise ValueError(f"{name} must be an integer that is not negative, got {value}")
    return int(value)


class MeshRemesher:
    """The state of one remeshing: current vertices (a vertex keeps its index, new ones are appended), faces, the normal every
    face had in the input, and ``origin`` per vertex (its input index while it is an input vertex at its input position, else
    -1).  ``low2`` and ``high2`` are the squared edge lengths below which an edge collapses and above which it splits."""

    def __init__(self, vertices: Tensor, faces: Tensor, low2: float, high2: float, flip_cos: float = 0.2, seed: int = 0):
        v, f = _mesh(vertices, faces)
        low2, high2 = float(low2), float(high2)
        if not (0 < low2 < high2 < float("inf")):
            raise ValueError(f"0 < low2 < high2, both finite, is required, got {low2} and {high2}")
        if not (0 <= flip_cos < 1):
            raise ValueError(f"flip_cos must lie in [0, 1), got {flip_cos}")
        self.device = v.device
        self._handle = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_meshremesh_create(N.ptr(v), int(v.shape[0]), N.ptr(f), int(f.shape[0]), low2, high2, float(flip_cos),
                                                    int(seed) & (2 ** 64 - 1), N.stream(), C.byref(self._handle)))

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            N.lib().surfd_meshremesh_destroy(h)
            self._handle = None

    def sizes(self):
        """(vertex slots, faces) now"""
        nv, nf = C.c_int64(), C.c_int64()
        N.check(N.lib().surfd_meshremesh_sizes(self._handle, C.byref(nv), C.byref(nf)))
        return int(nv.value), int(nf.value)

    def iterate(self, split_rounds: int = 4, collapse_rounds: int = 16, flip_rounds: int = 4, relax_sweeps: int = 1,
                relax: float = 1.0) -> Dict[str, int]:
        """one iteration (split, collapse, flip, relax); a dict of STAT_NAMES"""
        c = _counts(len(STAT_NAMES))
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_meshremesh_iterate(self._handle, int(split_rounds), int(collapse_rounds), int(flip_rounds), int(relax_sweeps),
                                                     float(relax), c, N.stream()))
        return dict(zip(STAT_NAMES, (int(x) for x in c)))

    def positions(self):
        """(positions float64 [V_now, 3], origin int64 [V_now]) of every vertex slot"""
        V, _ = self.sizes()
        x = torch.empty(V, 3, device=self.device, dtype=torch.float64)
        o = torch.empty(V, device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_meshremesh_get_positions(self._handle, N.ptr(x), N.ptr(o), N.stream()))
        return x, o.long()

    def set_positions(self, positions: Tensor) -> None:
        V, _ = self.sizes()
        if tuple(positions.shape) != (V, 3) or positions.dtype != torch.float64 or positions.device != self.device:
            raise ValueError(f"positions must be float64 [{V}, 3] on {self.device}")
        p = positions.contiguous()
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_meshremesh_set_positions(self._handle, N.ptr(p), N.stream()))
            torch.cuda.current_stream().synchronize()      # p may be a temporary

    def emit(self):
        """(vertices float64 [V', 3], faces int64 [F', 3], origin int64 [V']): the vertices the faces name, in ascending index"""
        V, F = self.sizes()
        ov = torch.empty(V, 3, device=self.device, dtype=torch.float64)
        of = torch.empty(F, 3, device=self.device, dtype=torch.int32)
        oo = torch.empty(V, device=self.device, dtype=torch.int32)
        c = _counts(2)
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_meshremesh_emit(self._handle, N.ptr(ov), N.ptr(of), N.ptr(oo), c, N.stream()))
        return ov[:c[0]], of[:c[1]].long(), oo[:c[0]].long()


def remesh_isotropic(vertices: Tensor, faces: Tensor, target_edge_length: float, *, iterations: int = 5, low: float = 0.8,
                     high: float = 4.0 / 3.0, split_rounds: int = 4, collapse_rounds: int = 16, flip_rounds: int = 4, relax_sweeps: int = 1,
                     relax: float = 1.0, flip_cos: float = 0.2, seed: int = 0, project: bool = False, accel: str = "tiles",
                     return_origin: bool = False, return_stats: bool = False):
    """(vertices float64 [V', 3], faces int64 [F', 3]) of the mesh remeshed towards edges of length ``target_edge_length`` = L
    (required; ``mean_edge_length`` offers one): ``iterations`` times, edges longer than ``high`` L are split at their midpoints
    (up to ``split_rounds`` rounds), edges shorter than ``low`` L are collapsed where that keeps the surface what it is, turns no
    face by more than ``flip_cos`` (a cosine) allows and makes no edge longer than ``high`` L (up to ``collapse_rounds`` rounds
    of collapses whose hashed priority, ``seed``, is the least around both end points), edges are flipped where that brings the
    valences of the four vertices closer to 6 (4 on a border; up to ``flip_rounds`` rounds), and every interior vertex moves
    ``relax`` in (0, 1] of the way to the mean of its neighbours, within its tangent plane (``relax_sweeps`` sweeps).  The call
    stops early after an iteration that split, collapsed, flipped and moved nothing.  ``project=True``: after every iteration the
    vertices that are no longer input vertices at their input positions are replaced by their closest points on the input mesh
    (fp32, MeshDistance with ``accel``).  The defaults are knobs, not tuned values: ``low`` and ``high`` are Botsch and Kobbelt's,
    ``flip_cos`` is simplify_quadric_decimation's, the rounds bound the work of an iteration.
    ``return_origin``: also int64 [V'], the input vertex an output vertex still is (same bits), else -1; ``return_stats``: also a
    list with one dict of STAT_NAMES per iteration made, the refusals those of the stage's last round."""
    v, f = _mesh(vertices, faces)
    L = float(target_edge_length)
    if not (0 < L < float("inf")):
        raise ValueError(f"target_edge_length must be positive and finite, got {target_edge_length}")
    low, high = float(low), float(high)
    if not (0 < low < high < float("inf")):
        raise ValueError(f"0 < low < high, both finite, is required, got {low} and {high}")
    if not (0 < relax <= 1):
        raise ValueError(f"relax must lie in (0, 1], got {relax}")
    if not (0 <= flip_cos < 1):
        raise ValueError(f"flip_cos must lie in [0, 1), got {flip_cos}")
    iterations = _rounds("iterations", iterations)
    rounds = [_rounds(n, x) for n, x in (("split_rounds", split_rounds), ("collapse_rounds", collapse_rounds), ("flip_rounds", flip_rounds),
                                         ("relax_sweeps", relax_sweeps))]
    if project and accel not in ("tiles", "bvh"):
        raise ValueError(f"accel must be 'tiles' or 'bvh', got {accel!r}")
    low2, high2 = (low * L) * (low * L), (high * L) * (high * L)          # made once, here, in fp64
    if not (0 < low2 < high2 < float("inf")):
        raise ValueError(f"(low L)^2 = {low2} and (high L)^2 = {high2} leave the range of float64")
    r = MeshRemesher(v, f, low2, high2, flip_cos, seed)
    scene = None
    stats: List[Dict[str, int]] = []
    for _ in range(iterations):
        c = r.iterate(*rounds, relax)
        stats.append(c)
        if project and c["faces"]:
            if scene is None:
                from .meshprep import MeshDistance
                scene = MeshDistance(v.float(), f.long(), accel=accel)
            x, o = r.positions()
            idx = torch.nonzero(o < 0).reshape(-1)
            if idx.numel():
                x[idx] = scene.closest(x[idx].float())[1].double()
                r.set_positions(x)
        if c["splits"] == 0 and c["collapses"] == 0 and c["flips"] == 0 and c["relaxed"] == 0:
            break
    ov, of, oo = r.emit()
    out = [ov, of]
    if return_origin:
        out.append(oo)
    if return_stats:
        out.append(stats)
    return tuple(out)


# ---- measures in plain torch (outside the contract: their rounding enters no result) ----------------------------------------------
def _unique_edges(faces: Tensor, V: int):
    """(lo, hi, valence) of the unique edges"""
    f = faces.long()
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    key, count = torch.unique(torch.minimum(a, b) * max(V, 1) + torch.maximum(a, b), return_counts=True)
    return key // max(V, 1), key % max(V, 1), count


def mean_edge_length(vertices: Tensor, faces: Tensor) -> float:
    """the mean length of the unique edges, in float64 torch: a target_edge_length to start from"""
    lo, hi, _ = _unique_edges(faces, int(vertices.shape[0]))
    if lo.numel() == 0:
        raise ValueError("the mesh has no edges")
    v = vertices.double()
    return float((v[hi] - v[lo]).norm(dim=1).mean())


def triangle_quality(vertices: Tensor, faces: Tensor, target_edge_length: Optional[float] = None, low: float = 0.8,
                     high: float = 4.0 / 3.0) -> Dict[str, float]:
    """edge_min / edge_mean / edge_max over the unique edges, edges_in_range (the share within [low L, high L], where L is
    given), min_angle_min / min_angle_mean (the smallest angle per face, degrees) and valence_deviation_mean (the mean
    |deg - t| over the vertices a face names, t = 4 at a border vertex, else 6)"""
    v, f = vertices.double(), faces.long()
    lo, hi, count = _unique_edges(f, int(v.shape[0]))
    if lo.numel() == 0:
        raise ValueError("the mesh has no edges")
    l = (v[hi] - v[lo]).norm(dim=1)
    out = {"edge_min": float(l.min()), "edge_mean": float(l.mean()), "edge_max": float(l.max())}
    if target_edge_length is not None:
        L = float(target_edge_length)
        out["edges_in_range"] = float(((l >= low * L) & (l <= high * L)).double().mean())
    angles = []
    for k in range(3):
        p, q, r = v[f[:, k]], v[f[:, (k + 1) % 3]], v[f[:, (k + 2) % 3]]
        u, w = q - p, r - p
        cs = (u * w).sum(1) / torch.sqrt((u * u).sum(1) * (w * w).sum(1))
        angles.append(torch.rad2deg(torch.acos(cs.clamp(-1.0, 1.0))))
    small = torch.nan_to_num(torch.stack(angles).min(dim=0).values)
    out["min_angle_min"], out["min_angle_mean"] = float(small.min()), float(small.mean())
    V = int(v.shape[0])
    deg = torch.bincount(lo, minlength=V) + torch.bincount(hi, minlength=V)
    border = torch.zeros(V, dtype=torch.bool, device=v.device)
    border[lo[count == 1]] = True
    border[hi[count == 1]] = True
    target = torch.where(border, 4, 6)
    out["valence_deviation_mean"] = float((deg - target).abs()[deg > 0].double().mean())
    return out
