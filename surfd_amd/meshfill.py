"""Hole filling on the MI355X path: every border loop of a mesh that lies on the device, up to ``max_edges`` edges long, is closed
there by its minimum-total-area triangulation (Barequet and Sharir 1995; the area term of Liepa 2003 without the dihedral one).
It takes over where meshclean.fill_small_holes stops (loops of 3 and 4 edges, which is all meshproc and trimesh close).

  fill_holes    the faces with the caps appended, optionally the loop number of every cap and the counts
  hole_sizes    the lengths of all border loops, ascending: what a caller looks at to choose ``max_edges``

tests/meshfill_ref.py restates the contract sequentially in numpy; faces, their order, cap_loop and every count equal it bit
for bit.  The work runs in csrc/meshfill.hip and nowhere else: device tensors in, device tensors out, CPU tensors are refused
(no CPU fallback).  Vertices are float64 [V, 3] (float32 is widened exactly), faces int64 [F, 3] (int32 is accepted); the faces
come back int64, the vertices are not touched.  Limits: 3 F < 2^31, V < 2^31; an index outside [0, V) is the library's
SURFD_ERR_ARG (a RuntimeError), found on the device and never a fault.

A LOOP is a cycle of n >= 3 border vertices that exactly one border half-edge leaves and exactly one enters, listed from its
smallest vertex; loops are numbered in ascending order of that vertex, the ones that stay open included.  Borders through a
vertex where two holes touch, or whose directions collide because the faces are not consistently oriented, are on no loop and
stay open (``irregular_border_edges``).  The caps of a loop run against its border, so they take the orientation of the faces
round it; they come in preorder of the triangulation's recursion, loops in ascending number.  For 3 edges the cap is a rotation
of fill_small_holes' cap; for 4 edges the diagonal is the one of smaller area and MAY DIFFER from fill_small_holes' fixed one.

Host syncs: two per call of fill_holes (the plan's counts, the run's counts; one where no loop is to be filled), one per call of
hole_sizes besides the copy of the lengths.  A call works on the current stream and keeps nothing.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Tuple, Union

import torch
from torch import Tensor

from . import _native as N
from .meshclean import _faces32, _vertices64
from .meshconn import _MeshConnectivity

MAX_EDGES_LIMIT = 1024
COUNT_KEYS = ("loops_filled", "caps", "loops_too_long", "loops_nonfinite", "irregular_border_edges", "border_edges", "longest_filled")


class _Fill(_MeshConnectivity):
    _abi = "surfd_meshfill"
    _what = "the hole filling"
    _vertex_dtypes = (torch.float32, torch.float64)

    def __init__(self, vertices: Tensor, faces: Tensor, max_edges: int):
        """the plan of one mesh: ``counts`` as the plan knows them"""
        self._check(faces, vertices)
        if vertices.device != faces.device:
            raise ValueError(f"vertices and faces must lie on one device, got {vertices.device} and {faces.device}")
        if not isinstance(max_edges, int) or isinstance(max_edges, bool) or not 3 <= max_edges <= MAX_EDGES_LIMIT:
            raise ValueError(f"max_edges must be an integer in [3, {MAX_EDGES_LIMIT}], got {max_edges!r}")
        self.device = faces.device
        self.counts = dict.fromkeys(COUNT_KEYS, 0)
        V, F = int(vertices.shape[0]), int(faces.shape[0])
        f = _faces32(faces, V)
        if V == 0 or F == 0:
            return                                              # no handle, no launch
        v, c, h = _vertices64(vertices), (C.c_int64 * 7)(), C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._fn("plan")(N.ptr(v), V, N.ptr(f), F, max_edges, c, N.stream(), C.byref(h)))
        self._handle = h
        self.counts = dict(zip(COUNT_KEYS, (int(x) for x in c)))

    def sizes(self) -> Tensor:
        n = self.counts["loops_filled"] + self.counts["loops_too_long"]
        out = torch.empty(n, device=self.device, dtype=torch.int32)
        if n:
            with torch.cuda.device(self.device):
                N.check(self._fn("loop_sizes")(self._handle, N.ptr(out), n, N.stream()))
        return out

    def run(self) -> Tuple[Tensor, Tensor]:
        """(caps [caps, 3] int32, cap_loop [caps] int32); ``counts`` become final"""
        rows = self.counts["caps"]
        caps = torch.empty(rows, 3, device=self.device, dtype=torch.int32)
        loop = torch.empty(rows, device=self.device, dtype=torch.int32)
        if self._handle is None or self.counts["loops_filled"] == 0:
            return caps, loop
        c = (C.c_int64 * 7)()
        with torch.cuda.device(self.device):
            N.check(self._fn("run")(self._handle, N.ptr(caps), rows, N.ptr(loop), c, N.stream()))
        self.counts = dict(zip(COUNT_KEYS, (int(x) for x in c)))
        return caps[:self.counts["caps"]], loop[:self.counts["caps"]]


def fill_holes(vertices: Tensor, faces: Tensor, max_edges: int = 128, return_cap_loop: bool = False,
               return_stats: bool = False) -> Union[Tensor, Tuple]:
    """Closes every border loop of 3 .. ``max_edges`` edges (``max_edges`` in [3, 1024]) by its minimum-area triangulation and
    returns the faces [F + caps, 3] int64: the input faces, then the caps.  ``return_cap_loop``: also the loop number of every cap
    [caps] int64; ``return_stats``: also a dict of loops_filled, caps, loops_too_long (longer than ``max_edges``: left open),
    loops_nonfinite (a NaN or Inf among their vertices, or an area that overflows: left open), irregular_border_edges (border edges
    on no loop: left open), border_edges (of the input) and longest_filled.  An empty mesh comes back as it is, without a launch."""
    plan = _Fill(vertices, faces, max_edges)
    caps, loop = plan.run()
    out = faces.long()
    if len(caps):
        out = torch.cat([out, caps.long()])
    res = (out,)
    if return_cap_loop:
        res += (loop.long(),)
    if return_stats:
        res += (dict(plan.counts),)
    return res[0] if len(res) == 1 else res


def hole_sizes(vertices: Tensor, faces: Tensor) -> List[int]:
    """The lengths of all border loops of the mesh in ascending order, from the plan alone (nothing is triangulated): the smallest
    ``max_edges`` that closes every loop is its last entry, where that is at most 1024."""
    plan = _Fill(vertices, faces, MAX_EDGES_LIMIT)
    return sorted(plan.sizes().tolist())
