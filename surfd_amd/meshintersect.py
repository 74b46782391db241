"""Intersection tests on triangle meshes on the MI355X path: which faces of a mesh pass through other faces of the same mesh
(self-intersections) and which faces of two meshes pass through each other (collisions).  No reference counterpart; the share
of self-intersecting faces is what work on meshing unsigned distance fields reports next to the Chamfer distance, and the first
question about a generated garment: does it cut through itself, or through the body it is draped on.

  lattice_for          the finest lattice that holds the given vertices
  IntersectionScene    one mesh, snapped and kept: self_intersections(), intersections(other)
  self_intersections   (vertices, triangles) -> the dict of IntersectionScene.self_intersections
  mesh_intersections   (v1, t1, v2, t2) -> the dict of IntersectionScene.intersections, one lattice from both meshes

The pair test runs in csrc/meshintersect.hip and nowhere else: device tensors in, device tensors out, CPU tensors are refused
(no CPU fallback).  Every vertex is snapped once to the lattice 2^-L (``q = rint(x * 2^L)`` in fp32, |q| <= 2^19), everything
after that is exact integer arithmetic: there is no epsilon and the answer does not depend on the order of the faces.  Vertices
that snap to the same lattice point are the same point, so an unwelded mesh behaves as the welded one; features finer than
2^-L merge.  Triangles are closed sets: touching counts, and so does a T-junction (a vertex lying on another face's edge
without being one of its corners).  Two faces that share an edge intersect only when they are folded flat onto each other, two
faces with the same three points (duplicates, in either winding) always do.  Faces without area after the snap are reported as
``degenerate`` and intersect nothing.  DESIGN.md section 8.9 states the rules in full.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
from torch import Tensor

from . import _native as N
from .meshprep import _MeshScene

BRUTE_FORCE = 1
COUNT_SKIPPED = 2
SNAP_LOG2 = 19                   # |q| <= 2^19
MAX_LOG2 = 100


def lattice_for(*vertex_tensors: Tensor) -> int:
    """the largest L with max|x| * 2^L <= 2^19 over all tensors given: 19 for anything within [-1, 1].  One host sync per
    tensor on the device."""
    if not vertex_tensors:
        raise ValueError("lattice_for needs at least one tensor")
    m = 0.0
    for v in vertex_tensors:
        if v.numel():
            x = float(v.detach().abs().max())                      # a NaN anywhere makes the maximum a NaN
            if not math.isfinite(x):
                raise ValueError("vertices contain NaN or Inf")
            m = max(m, x)
    if m == 0.0:
        return SNAP_LOG2
    f, e = math.frexp(m)                                           # m = f * 2^e with 0.5 <= f < 1
    return max(-MAX_LOG2, min(MAX_LOG2, SNAP_LOG2 - e + (1 if f == 0.5 else 0)))


def _sorted_pairs(keys: Tensor, perm_a: Tensor, perm_b: Tensor, order: bool) -> Tensor:
    """keys i << 32 | j in the library's indices -> [P, 2] int64 in the caller's, in lexicographic order"""
    a, b = perm_a[keys >> 32], perm_b[keys & 0xFFFFFFFF]
    if order:
        a, b = torch.minimum(a, b), torch.maximum(a, b)
    k = torch.sort((a << 32) | b).values
    return torch.stack([k >> 32, k & 0xFFFFFFFF], 1)


class IntersectionScene(_MeshScene):
    """One mesh, snapped to the lattice 2^-lattice_log2 and kept for repeated calls.

    The triangles are handed to the library in Morton order of their centroids, so that its tiles of 32 faces are compact and
    the culling bites; everything comes back in the caller's indices.  ``lattice_log2=None`` takes ``lattice_for(vertices)``;
    two scenes can be compared only when they were made with the same value.  Host syncs: the constructor (the lattice, the
    library's refusal flags) and every query (the pair count)."""

    _abi = "surfd_isect"

    def __init__(self, vertices: Tensor, triangles: Tensor, lattice_log2: Optional[int] = None):
        def lattice() -> tuple:
            self.lattice_log2 = lattice_for(vertices) if lattice_log2 is None else lattice_log2
            if isinstance(self.lattice_log2, bool) or not isinstance(self.lattice_log2, int):
                raise TypeError(f"lattice_log2 must be an int, got {self.lattice_log2!r}")
            return (self.lattice_log2,)

        # no checks of the values here: a bad index or a NaN must reach the library, which refuses it
        self._open(vertices, triangles, what="mesh intersection", check_values=False, extra=lattice)

    def _unsort(self, x: Tensor) -> Tensor:
        out = torch.empty_like(x)
        out[self._perm] = x
        return out

    def degenerate(self) -> Tensor:
        """[F] bool: the faces without area after the snap"""
        flags = torch.empty(self.num_triangles, device=self.device, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_isect_degenerate(self._handle, N.ptr(flags), None, N.stream()))
        return self._unsort(flags).bool()

    def _run(self, other: Optional["IntersectionScene"], return_pairs: bool, brute_force: bool, count_skipped: bool,
             capacity: Optional[int]):
        L = N.lib()
        flags = (BRUTE_FORCE if brute_force else 0) | (COUNT_SKIPPED if count_skipped else 0)
        fb = self.num_triangles if other is None else other.num_triangles
        hits_a = torch.empty(self.num_triangles, device=self.device, dtype=torch.int32)
        hits_b = None if other is None else torch.empty(fb, device=self.device, dtype=torch.int32)
        count = torch.empty(1, device=self.device, dtype=torch.int64)
        if not return_pairs:
            cap = 0
        elif capacity is None:
            cap = max(4096, 2 * (self.num_triangles + fb))       # a guess; one re-call when the count exceeds it
        else:
            cap = int(capacity)
            if cap < 1:
                raise ValueError(f"capacity must be positive, got {capacity}")
        with torch.cuda.device(self.device):
            while True:
                keys = torch.empty(cap, device=self.device, dtype=torch.int64) if return_pairs else None
                if other is None:
                    N.check(L.surfd_isect_self(self._handle, flags, N.ptr(hits_a), N.ptr(keys), cap, N.ptr(count), N.stream()))
                else:
                    N.check(L.surfd_isect_between(self._handle, other._handle, flags, N.ptr(hits_a), N.ptr(hits_b), N.ptr(keys), cap,
                                                  N.ptr(count), N.stream()))
                n = int(count)
                if not return_pairs or n <= cap:
                    break
                cap = n
            if count_skipped:
                self.last_skipped_tiles, self.last_total_tiles = self._read_counters("skipped")
        return n, hits_a, hits_b, (keys[:n] if return_pairs else None)

    def self_intersections(self, return_pairs: bool = True, brute_force: bool = False, count_skipped: bool = False,
                           capacity: Optional[int] = None) -> Dict[str, object]:
        """-> {"count": the number of intersecting pairs of faces (int), "hits" [F] int32: the pairs each face belongs to,
        "faces" [F] bool: hits > 0, "fraction": the share of the faces with area that intersect another (float),
        "degenerate" [F] bool, and with ``return_pairs`` "pairs" [P, 2] int64: (i, j) with i < j in lexicographic order}.
        ``brute_force`` evaluates every pair (the correctness baseline; the same result).  ``capacity`` sets the first guess of
        the pair buffer (a larger count costs one re-call).  With ``count_skipped`` the number of (wave, tile) visits that
        culling skipped is left in ``last_skipped_tiles`` and their total in ``last_total_tiles``."""
        n, hits, _, keys = self._run(None, return_pairs, brute_force, count_skipped, capacity)
        hits = self._unsort(hits)
        deg = self.degenerate()
        faces = hits > 0
        solid = int((~deg).sum())
        out = {"count": n, "hits": hits, "faces": faces, "fraction": (int(faces.sum()) / solid) if solid else 0.0, "degenerate": deg}
        if return_pairs:
            out["pairs"] = _sorted_pairs(keys, self._perm, self._perm, True)
        return out

    def intersections(self, other: "IntersectionScene", return_pairs: bool = True, brute_force: bool = False,
                      count_skipped: bool = False, capacity: Optional[int] = None) -> Dict[str, object]:
        """the faces of this mesh (a) against those of ``other`` (b), closed triangles, no sharing rule: a vertex of one lying
        exactly on the other counts.  -> {"count", "hits_a" [Fa] int32, "hits_b" [Fb] int32, "faces_a", "faces_b" bool,
        "fraction": the share of a's faces with area that meet b, "degenerate" [Fa] bool (a's), and with ``return_pairs``
        "pairs" [P, 2] int64: (face of a, face of b) in lexicographic order}"""
        if not isinstance(other, IntersectionScene):
            raise TypeError("intersections needs another IntersectionScene")
        if other.device != self.device:
            raise RuntimeError(f"the other mesh is on {other.device}, this one on {self.device}")
        n, hits_a, hits_b, keys = self._run(other, return_pairs, brute_force, count_skipped, capacity)
        hits_a, hits_b = self._unsort(hits_a), other._unsort(hits_b)
        deg = self.degenerate()
        faces_a = hits_a > 0
        solid = int((~deg).sum())
        out = {"count": n, "hits_a": hits_a, "hits_b": hits_b, "faces_a": faces_a, "faces_b": hits_b > 0,
               "fraction": (int(faces_a.sum()) / solid) if solid else 0.0, "degenerate": deg}
        if return_pairs:
            out["pairs"] = _sorted_pairs(keys, self._perm, other._perm, False)
        return out


def self_intersections(vertices: Tensor, triangles: Tensor, lattice_log2: Optional[int] = None, **kw) -> Dict[str, object]:
    """IntersectionScene(vertices, triangles, lattice_log2).self_intersections(**kw)"""
    return IntersectionScene(vertices, triangles, lattice_log2).self_intersections(**kw)


def mesh_intersections(v1: Tensor, t1: Tensor, v2: Tensor, t2: Tensor, lattice_log2: Optional[int] = None, **kw) -> Dict[str, object]:
    """the faces of mesh 1 against those of mesh 2 on one lattice, by default the finest that holds both"""
    if lattice_log2 is None:
        lattice_log2 = lattice_for(v1, v2)
    return IntersectionScene(v1, t1, lattice_log2).intersections(IntersectionScene(v2, t2, lattice_log2), **kw)
