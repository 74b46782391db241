"""Mesh simplification on the MI355X path: vertex clustering on a uniform grid (Rossignac-Borrel) with one representative per
occupied cell, the mean of the cell's vertices or the minimiser of the cell's plane quadric (Lindstrom), which keeps edges and
corners where the mean rounds them.  A mesh that lies on the device is made smaller there:

  simplify_vertex_clustering     (vertices, faces[, vertex_map][, stats])
  simplify_quadric_decimation    (vertices, faces[, vertex_map][, stats]): edge collapses down to a target face count
                                 (csrc/meshdecimate.hip, restated in tests/meshdecimate_ref.py); borders stay where they were,
                                 manifold input stays manifold, sheets are not glued together

tests/meshsimplify_ref.py restates the contract sequentially in numpy: every result equals it bit for bit and in the same order
(vertex order, face order, every double).  The work runs in csrc/meshsimplify.hip and nowhere else: device tensors in, device
tensors out, CPU tensors are refused (no CPU fallback).  Vertices are float64 [V, 3] (float32 is widened exactly), faces int64
[F, 3] (int32 is accepted); vertices come back float64 and faces int64, as surfd_amd.meshclean returns them.  Limits: 3 F < 2^31,
V < 2^31; an index outside [0, V) and a cell index outside [0, 2^21) are the library's SURFD_ERR_ARG (a RuntimeError), found on the
device and never a fault.  Nothing is kept between calls; a call works on the current stream.

Out of scope: for clustering, any guarantee that the output is manifold or free of flipped or folded faces (it pinches two sheets
that pass through one cell); for decimation, any guarantee on non-manifold input (it comes out clean, no more) and the detection
of fans (faces that fold within the flip bound); for both, attributes beyond ``vertex_map`` and batches of meshes in one launch.

Host syncs: 3 per call (the cluster and face counts, the duplicate pass's count, the output sizes), 2 where every face collapses;
``cells=K`` adds the read of the extent.  Decimation: 2 per call and 2 per round.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _native as N
from .meshclean import _counts, _mesh

REPRESENTATIVES = {"mean": 0, "quadric": 1}              # SURFD_SIMPLIFY_MEAN, SURFD_SIMPLIFY_QUADRIC
STAT_NAMES = ("vertices", "faces", "clusters", "collapsed_faces", "duplicate_faces", "fallbacks")
MAX_CELLS = 2 ** 21 - 1                                  # per axis: the cell indices 0 .. cells fit the 21-bit key fields


def _referenced_extent(v: Tensor, f: Tensor) -> float:
    """the largest extent per axis of the vertices that take part (those a face without a non-finite vertex names), in fp64 torch;
    0.0 without one.  Indices outside [0, V) are left to the library: their faces are skipped here."""
    V = int(v.shape[0])
    fl = f.long()
    inside = ((fl >= 0) & (fl < V)).all(dim=1)
    finite = torch.isfinite(v).all(dim=1)
    keep = inside & finite[fl.clamp(0, V - 1)].all(dim=1)
    used = torch.zeros(V, dtype=torch.bool, device=v.device)
    used[fl[keep].reshape(-1)] = True
    if not bool(used.any()):
        return 0.0
    p = v[used]
    return float((p.max(dim=0).values - p.min(dim=0).values).max())


def simplify_vertex_clustering(vertices: Tensor, faces: Tensor, cell: Optional[float] = None, *, cells: Optional[int] = None,
                               representative: str = "quadric", origin: Optional[Sequence[float]] = None, rank_tol: float = 1e-3,
                               return_map: bool = False, return_stats: bool = False):
    """(vertices float64 [V', 3], faces int64 [F', 3]) of the mesh clustered on a grid of ``cell``-sized cubes: every occupied cell
    becomes one vertex, faces with two corners in one cell go, one face stays per set of three cells (the lowest, with its own
    winding, in meshclean.drop_duplicate_faces' order), cells no face names go.  Pass exactly one of ``cell`` and ``cells``: with
    ``cells=K`` the cell is the largest extent of the vertices that take part divided by K.  ``origin``: the corner the grid starts
    from (3 numbers; every vertex that takes part must lie at or above it), by default the minimum of those vertices.
    ``representative``: "quadric" (eigenvalues below ``rank_tol`` times the largest are truncated; the mean where the solve leaves
    the cell's neighbourhood) or "mean".  ``return_map``: also int64 [V], the output vertex of every input vertex or -1;
    ``return_stats``: also a dict of vertices, faces, clusters, collapsed_faces, duplicate_faces and fallbacks."""
    v, f = _mesh(vertices, faces)
    if (cell is None) == (cells is None):
        raise ValueError("pass exactly one of cell and cells")
    if representative not in REPRESENTATIVES:
        raise ValueError(f"representative must be one of {sorted(REPRESENTATIVES)}, got {representative!r}")
    if not (rank_tol > 0 and rank_tol < float("inf")):
        raise ValueError(f"rank_tol must be positive and finite, got {rank_tol}")
    org = None
    if origin is not None:
        o = [float(x) for x in (origin.tolist() if isinstance(origin, Tensor) else origin)]
        if len(o) != 3 or not all(abs(x) < float("inf") for x in o):
            raise ValueError(f"origin must be 3 finite numbers, got {origin}")
        org = (C.c_double * 3)(*o)
    V, F = int(v.shape[0]), int(f.shape[0])
    if cells is not None:
        if int(cells) != cells or not 1 <= int(cells) <= MAX_CELLS:
            raise ValueError(f"cells must be an integer in [1, {MAX_CELLS}], got {cells}")
        cell = _referenced_extent(v, f) / int(cells) if V and F else 1.0
        if V and F and not cell > 0:
            raise ValueError("cells needs a mesh with an extent: the vertices that take part span no axis")
    cell = float(cell)
    if not (cell > 0 and cell < float("inf")):
        raise ValueError(f"cell must be positive and finite, got {cell}")
    ov, of, c = torch.empty_like(v), torch.empty_like(f), _counts(6)
    vmap = torch.empty(V, device=v.device, dtype=torch.int32) if return_map else None
    with torch.cuda.device(v.device):
        N.check(N.lib().surfd_meshsimplify_cluster(N.ptr(v), V, N.ptr(f), F, org, cell, REPRESENTATIVES[representative], float(rank_tol), N.ptr(ov),
                                                   N.ptr(of), N.ptr(vmap) if return_map else None, c, N.stream()))
    out = [ov[:c[0]], of[:c[1]].long()]
    if return_map:
        out.append(vmap.long())
    if return_stats:
        out.append(dict(zip(STAT_NAMES, (int(x) for x in c))))
    return tuple(out)


DECIMATE_STAT_NAMES = ("vertices", "faces", "rounds", "collapses", "border_collapses", "stop", "refused_valence", "refused_link",
                       "refused_border", "refused_opposite", "refused_flip", "refused_nan")
DECIMATE_STOPS = ("target", "stalled", "max_rounds")


def simplify_quadric_decimation(vertices: Tensor, faces: Tensor, target_faces: Optional[int] = None, *, ratio: Optional[float] = None,
                                border_weight: float = 1000.0, flip_cos: float = 0.2, rank_tol: float = 1e-3, spread: int = 4,
                                max_rounds: int = 512, seed: int = 0, return_map: bool = False, return_stats: bool = False):
    """(vertices float64 [V', 3], faces int64 [F', 3]) of the mesh after edge collapses down to ``target_faces`` faces (or
    ``ratio`` times the faces given, rounded down; pass exactly one), by quadric error metrics in rounds of independent collapses:
    every round ranks the valid edges by cost, takes the first ``spread`` times as many as are still to go as candidates, and
    collapses those whose hashed priority (``seed``) is the least around both end points.  An edge is valid when the collapse keeps
    the surface what it is (valence, link condition, borders, no vertex left with two edges) and turns no face by more than
    ``flip_cos`` (the cosine between its old and new normal) allows.  A border edge adds the plane through it perpendicular to its
    face, ``border_weight`` times: borders stay where they were.  The point of a collapse minimises the summed quadric, directions
    whose eigenvalue is below ``rank_tol`` times the largest left at the midpoint.  The call stops at the target, when a round
    finds nothing to collapse ("stalled": the output then has more faces than asked for) or after ``max_rounds``.
    The defaults are knobs, not tuned values: ``border_weight`` and ``flip_cos`` are the customary ones of quadric decimation,
    ``rank_tol`` is simplify_vertex_clustering's, ``spread`` and ``max_rounds`` bound the work of a round and of a call.
    On a closed manifold mesh F' is target_faces or one less; on any mesh F' <= target_faces unless the call stalled.
    ``return_map``: also int64 [V], the output vertex every input vertex ended in, -1 where it took no part; ``return_stats``:
    also a dict of DECIMATE_STAT_NAMES, ``stop`` as one of DECIMATE_STOPS, the refusals those of the last round."""
    v, f = _mesh(vertices, faces)
    if (target_faces is None) == (ratio is None):
        raise ValueError("pass exactly one of target_faces and ratio")
    V, F = int(v.shape[0]), int(f.shape[0])
    if ratio is not None:
        if not 0 <= ratio <= 1:
            raise ValueError(f"ratio must lie in [0, 1], got {ratio}")
        target_faces = int(F * float(ratio))
    if int(target_faces) != target_faces or target_faces < 0:
        raise ValueError(f"target_faces must be an integer that is not negative, got {target_faces}")
    if not (0 <= border_weight < float("inf")):
        raise ValueError(f"border_weight must be finite and not negative, got {border_weight}")
    if not (0 <= flip_cos < 1):
        raise ValueError(f"flip_cos must lie in [0, 1), got {flip_cos}")
    if not (rank_tol > 0 and rank_tol < float("inf")):
        raise ValueError(f"rank_tol must be positive and finite, got {rank_tol}")
    if int(spread) != spread or spread < 1 or int(max_rounds) != max_rounds or max_rounds < 1:
        raise ValueError(f"spread and max_rounds must be integers of at least 1, got {spread} and {max_rounds}")
    ov, of, c = torch.empty_like(v), torch.empty_like(f), _counts(12)
    vmap = torch.empty(V, device=v.device, dtype=torch.int32) if return_map else None
    with torch.cuda.device(v.device):
        N.check(N.lib().surfd_meshsimplify_decimate(N.ptr(v), V, N.ptr(f), F, int(target_faces), float(border_weight), float(flip_cos), float(rank_tol),
                                                    int(spread), int(max_rounds), int(seed) & (2 ** 64 - 1), N.ptr(ov), N.ptr(of),
                                                    N.ptr(vmap) if return_map else None, c, N.stream()))
    out = [ov[:c[0]], of[:c[1]].long()]
    if return_map:
        out.append(vmap.long())
    if return_stats:
        stats = dict(zip(DECIMATE_STAT_NAMES, (int(x) for x in c)))
        stats["stop"] = DECIMATE_STOPS[stats["stop"]]
        out.append(stats)
    return tuple(out)
