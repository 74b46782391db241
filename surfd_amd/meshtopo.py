"""Topology of a triangle mesh on the MI355X path: is it closed, is it manifold, how many pieces, how many holes and how large,
are its faces consistently oriented, and if not, make them so.

  MeshTopology                    edges / valences / half-edge lists / face neighbours   <- trimesh's edges_unique, face_adjacency
  MeshTopology.components         pieces by vertex, edge or manifold-edge connectivity   <- Trimesh.split, pymeshlab's components
  MeshTopology.border_loops       the holes: loops of border edges and their sizes       <- Trimesh.outline
  MeshTopology.orientation        a consistent winding per manifold patch                <- trimesh.repair.fix_normals
  MeshTopology.summary            the numbers above as plain ints and bools
  weld_vertices                   coincident vertices become one (exact, no tolerance)   <- Trimesh.merge_vertices
  orient_faces, face_components, keep_components_with_at_least, is_closed                 the one-shot forms

The work runs in csrc/meshtopo.hip and nowhere else: device tensors in, device tensors out, CPU tensors are refused (no CPU
fallback).  Everything is combinatorial: the input is the index array (after an optional exact weld), the outputs are integers
and bools, and each is a function of the input alone (csrc/meshtopo.hip's header states the contract; tests/meshtopo_ref.py
restates it sequentially).  Only the small per-patch arithmetic of ``summary`` (counts per label) is torch on the device arrays.

Definitions.  Half-edge h = 3 f + c runs from t[f, c] to t[f, (c + 1) % 3].  A face with two equal indices is degenerate: it is
listed in ``degenerate`` and takes part in nothing else (rows -1, labels -1, flip 0).  Edges are the distinct unordered pairs
(lo < hi) in ascending order; border = valence 1, manifold = 2, non-manifold >= 3.  A patch is a component under "manifold"
connectivity.  Non-manifold VERTICES (fans) are not detected.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple, Union

import torch
from torch import Tensor

from . import _native as N
from .meshconn import _MeshConnectivity

CONNECTIVITY = {"vertex": 0, "edge": 1, "manifold": 2}      # SURFD_MESHTOPO_VERTEX / _EDGE / _MANIFOLD


class MeshTopology(_MeshConnectivity):
    """The edges of one mesh, kept for repeated questions.  Arrays are computed on first use and kept; index arrays come back as
    int64, masks as bool.  Host syncs: the constructor (the number of edges is read back; ``num_vertices=None`` also reads the
    largest index), ``components`` and ``border_loops`` (the number of components); ``orientation`` and the array properties only
    enqueue.  One stream at a time per object: the library keeps its workspaces in the handle."""

    _abi = "surfd_meshtopo"
    _what = "the mesh topology"

    def __init__(self, triangles: Tensor, num_vertices: Optional[int] = None):
        faces, self.num_edges, self.num_degenerate, self.num_referenced_vertices = self._open(triangles, num_vertices)
        assert faces == self.num_faces
        self.triangles = triangles.long().contiguous()
        self._arrays: Optional[Dict[str, Tensor]] = None
        self._components: Dict[str, Tuple[Tensor, Tensor]] = {}
        self._loops: Optional[Tuple[Tensor, Tensor, Tensor]] = None
        self._orientation: Optional[Tuple[Tensor, Tensor]] = None

    # ---- edges --------------------------------------------------------------------------------------------------------------
    def _read(self) -> Dict[str, Tensor]:
        if self._arrays is None:
            F, E, H = self.num_faces, self.num_edges, 3 * (self.num_faces - self.num_degenerate)
            i32 = dict(device=self.device, dtype=torch.int32)
            a = {"edges": torch.empty(E, 2, **i32), "valence": torch.empty(E, **i32), "edge_offsets": torch.empty(E + 1, **i32),
                 "edge_halfedges": torch.empty(H, **i32), "face_edges": torch.empty(F, 3, **i32), "face_neighbors": torch.empty(F, 3, **i32),
                 "degenerate": torch.empty(F, device=self.device, dtype=torch.uint8)}
            with torch.cuda.device(self.device):
                N.check(N.lib().surfd_meshtopo_read(self._handle, *[N.ptr(a[k]) for k in ("edges", "valence", "edge_offsets", "edge_halfedges",
                                                                                        "face_edges", "face_neighbors", "degenerate")], N.stream()))
            self._arrays = {k: (v.bool() if k == "degenerate" else v.long()) for k, v in a.items()}
        return self._arrays

    edges = property(lambda self: self._read()["edges"], doc="[E, 2] (lo, hi), ascending")
    valence = property(lambda self: self._read()["valence"], doc="[E] the number of half-edges on every edge")
    edge_offsets = property(lambda self: self._read()["edge_offsets"], doc="[E + 1] where an edge's half-edges start in edge_halfedges")
    edge_halfedges = property(lambda self: self._read()["edge_halfedges"], doc="the half-edges 3 f + c of every edge, ascending inside an edge")
    face_edges = property(lambda self: self._read()["face_edges"], doc="[F, 3] the edge of half-edge 3 f + c; -1 in a degenerate face")
    face_neighbors = property(lambda self: self._read()["face_neighbors"], doc="[F, 3] the face across; -1 border or degenerate, -2 non-manifold")
    degenerate = property(lambda self: self._read()["degenerate"], doc="[F] bool: the face has two equal indices")

    # ---- partitions ---------------------------------------------------------------------------------------------------------
    def components(self, connectivity: str = "vertex") -> Tuple[Tensor, Tensor]:
        """(labels [F], sizes [C]): the components under "vertex", "edge" or "manifold" connectivity, numbered in ascending
        order of their lowest face; -1 for a degenerate face."""
        if connectivity not in CONNECTIVITY:
            raise ValueError(f"connectivity must be one of {sorted(CONNECTIVITY)}, got {connectivity!r}")
        if connectivity not in self._components:
            labels = torch.empty(self.num_faces, device=self.device, dtype=torch.int32)
            count = C.c_int64()
            with torch.cuda.device(self.device):
                N.check(N.lib().surfd_meshtopo_components(self._handle, CONNECTIVITY[connectivity], N.ptr(labels), C.byref(count), N.stream()))
            labels = labels.long()
            sizes = torch.bincount(labels[labels >= 0], minlength=int(count.value))
            self._components[connectivity] = (labels, sizes)
        return self._components[connectivity]

    def border_loops(self) -> Tuple[Tensor, Tensor, Tensor]:
        """(labels [B], sizes [L], simple [L]): the loop of every border edge (in edge order: row i belongs to the i-th edge of
        valence 1), the number of edges of every loop, and whether every vertex of the loop touches exactly two of its edges.
        Loops are the components of the border edges under "share a vertex", numbered in ascending order of their lowest edge."""
        if self._loops is None:
            E = self.num_edges
            labels = torch.empty(E, device=self.device, dtype=torch.int32)
            irregular = torch.empty(E, device=self.device, dtype=torch.uint8)
            count = C.c_int64()
            with torch.cuda.device(self.device):
                N.check(N.lib().surfd_meshtopo_border_loops(self._handle, N.ptr(labels), N.ptr(irregular), C.byref(count), N.stream()))
            border = self.valence == 1
            lb = labels.long()[border]
            L = int(count.value)
            sizes = torch.bincount(lb, minlength=L)
            simple = torch.bincount(lb, weights=irregular[border].double(), minlength=L) == 0
            self._loops = (lb, sizes, simple)
        return self._loops

    def _orient(self, vertices: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
        F = self.num_faces
        flip = torch.empty(F, device=self.device, dtype=torch.uint8)
        orientable = torch.empty(F, device=self.device, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_meshtopo_orient(self._handle, N.ptr(vertices), N.ptr(flip), N.ptr(orientable), None, N.stream()))
        labels, sizes = self.components("manifold")
        patch_orientable = torch.ones(len(sizes), device=self.device, dtype=torch.bool)
        live = labels >= 0
        patch_orientable[labels[live]] = orientable[live].bool()           # every face of a patch carries the same value
        return flip.bool(), patch_orientable

    def orientation(self, vertices: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """(flip [F] bool, patch_orientable [P] bool).  flip is the one assignment under which the half-edges of every manifold
        edge run in opposite directions and the lowest face of every patch keeps its winding; all False in a patch that has no
        such assignment (patch_orientable False) and in degenerate faces.  With ``vertices`` [V, 3] float32 every orientable
        patch that is closed (all edges of all its faces have valence 2) is then turned as a whole so that its signed volume
        is positive (a 64-bit fixed-point sum, so it has no order; 0 leaves the patch).  Patch by patch: the shell of a cavity
        ends up outward too."""
        if vertices is None:
            if self._orientation is None:
                self._orientation = self._orient(None)
            return self._orientation
        return self._orient(self._positions(vertices))

    def oriented_triangles(self, vertices: Optional[Tensor] = None) -> Tensor:
        """the triangles [F, 3] with columns 1 and 2 of the flipped faces swapped (``vertices``: outward, see orientation)"""
        flip = self.orientation(vertices)[0]
        t = self.triangles
        return torch.where(flip[:, None], t[:, [0, 2, 1]], t)

    # ---- the numbers --------------------------------------------------------------------------------------------------------
    def summary(self) -> dict:
        """Plain ints and bools.  chi = V - E + F over the vertices, edges and faces of the non-degenerate faces.  Per patch:
        faces, closed, orientable and the genus (2 - chi_patch) / 2 where the patch is closed and orientable, else None."""
        F, E = self.num_faces, self.num_edges
        val = self.valence
        nb, nm, nn = int((val == 1).sum()), int((val == 2).sum()), int((val >= 3).sum())
        live_faces = F - self.num_degenerate
        loops = self.border_loops()
        flip, patch_orientable = self.orientation()
        labels, sizes = self.components("manifold")
        P = len(sizes)
        live = labels >= 0
        lab = labels[live]
        fe = self.face_edges[live]
        face_closed = (val[fe] == 2).all(dim=1) if live_faces else torch.zeros(0, dtype=torch.bool, device=self.device)
        patch_closed = torch.bincount(lab, weights=(~face_closed).double(), minlength=P) == 0
        tv = self.triangles[live]
        pv = torch.bincount(torch.unique(lab[:, None] * max(self.num_vertices, 1) + tv) // max(self.num_vertices, 1), minlength=P)
        pe = torch.bincount(torch.unique(lab[:, None] * max(E, 1) + fe) // max(E, 1), minlength=P)
        chi = (pv - pe + sizes).tolist()
        pc, po, ps = patch_closed.tolist(), patch_orientable.tolist(), sizes.tolist()
        patches = [{"faces": int(ps[i]), "closed": bool(pc[i]), "orientable": bool(po[i]),
                    "genus": (2 - int(chi[i])) // 2 if pc[i] and po[i] else None} for i in range(P)]
        return {
            "faces": F, "degenerate_faces": self.num_degenerate, "referenced_vertices": self.num_referenced_vertices,
            "edges": E, "border_edges": nb, "manifold_edges": nm, "non_manifold_edges": nn,
            "euler_characteristic": self.num_referenced_vertices - E + live_faces,
            "components_vertex": len(self.components("vertex")[1]), "components_edge": len(self.components("edge")[1]),
            "components_manifold": P,
            "border_loops": len(loops[1]), "largest_border_loop": int(loops[1].max()) if len(loops[1]) else 0,
            "closed": self.num_degenerate == 0 and nb == 0 and nn == 0,
            "edge_manifold": nn == 0,
            "orientable": bool(patch_orientable.all()),
            "consistently_oriented": bool(patch_orientable.all()) and not bool(flip.any()),
            "patches": patches,
        }


# ---- one-shot forms -----------------------------------------------------------------------------------------------------------
def weld_vertices(vertices: Tensor, triangles: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(vertices_w [W, 3], triangles_w [F, 3], vertex_map [V]): vertices with equal float32 coordinates become one (-0 equals +0, a
    vertex that holds a NaN equals nothing); the survivor is the lowest index of its class, survivors keep their relative order,
    vertex_map[i] is the new index of vertex i's survivor.  There is no tolerance.  Unreferenced vertices stay."""
    MeshTopology._check(triangles, vertices)
    v = vertices.contiguous()
    V = int(v.shape[0])
    if 3 * V >= 2 ** 31:
        raise ValueError(f"3 V must stay below 2^31, got V = {V}")
    vmap = torch.empty(V, device=v.device, dtype=torch.int32)
    surv = torch.empty(V, device=v.device, dtype=torch.uint8)
    count = C.c_int64()
    with torch.cuda.device(v.device):
        N.check(N.lib().surfd_meshtopo_weld(N.ptr(v), V, N.ptr(vmap), N.ptr(surv), C.byref(count), N.stream()))
    vmap = vmap.long()
    t = triangles.long()
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= V):
        raise ValueError(f"triangles name vertices outside [0, {V})")
    vw = v[surv.bool()]
    assert vw.shape[0] == int(count.value)
    return vw, vmap[t], vmap


def orient_faces(vertices: Tensor, triangles: Tensor, outward: bool = False, weld: bool = False) -> Tuple[Tensor, dict]:
    """(triangles [F, 3] int64, info): the triangles with a consistent winding per manifold patch (MeshTopology.orientation;
    ``outward``: closed patches get a positive volume).  ``weld``: the topology is that of the exactly welded mesh (for soups
    whose faces share no indices); the returned triangles still name the caller's vertices.  info: ``flip`` [F] bool, ``flipped``
    (how many), ``patches``, ``non_orientable`` (the lowest face of every patch that has no consistent winding; those faces stay
    as they are)."""
    MeshTopology._check(triangles, vertices)
    if weld:
        vw, tw, _ = weld_vertices(vertices, triangles)
    else:
        vw, tw = vertices.contiguous(), triangles
    topo = MeshTopology(tw, vw.shape[0])
    flip, patch_orientable = topo.orientation(vw if outward else None)
    labels, _ = topo.components("manifold")
    bad = []
    if not bool(patch_orientable.all()):
        live = labels >= 0
        first = torch.full((len(patch_orientable),), topo.num_faces, device=labels.device, dtype=torch.long)
        first.scatter_reduce_(0, labels[live], torch.nonzero(live)[:, 0], reduce="amin")
        bad = first[~patch_orientable].tolist()
    t = triangles.long()
    out = torch.where(flip[:, None], t[:, [0, 2, 1]], t)
    return out, {"flip": flip, "flipped": int(flip.sum()), "patches": len(patch_orientable), "non_orientable": [int(b) for b in bad]}


def oriented_for_winding(vertices: Tensor, triangles: Tensor, orient: Union[bool, str]) -> Tensor:
    """what the ``orient`` keyword of the winding-number consumers does: False leaves the triangles, True makes every patch
    consistent, "outward" also turns closed patches outward.  A patch that cannot be oriented raises."""
    if orient is False or orient is None:
        return triangles
    if orient is not True and orient != "outward":
        raise ValueError(f"orient must be False, True or 'outward', got {orient!r}")
    out, info = orient_faces(vertices, triangles, outward=(orient == "outward"))
    if info["non_orientable"]:
        raise ValueError(f"the mesh cannot be consistently oriented: the patch of face {info['non_orientable'][0]} is not orientable "
                         f"({len(info['non_orientable'])} such patches)")
    return out


def face_components(triangles: Tensor, num_vertices: Optional[int] = None, connectivity: str = "vertex") -> Tensor:
    """labels [F]: the components of the faces (MeshTopology.components), -1 for a degenerate face"""
    return MeshTopology(triangles, num_vertices).components(connectivity)[0]


def keep_components_with_at_least(vertices: Tensor, faces: Tensor, min_faces: int) -> Tuple[Tensor, Tensor]:
    """(vertices, faces): components (by shared vertices) with fewer than ``min_faces`` faces go, and the vertices only they used
    with them; kept faces and kept vertices stay in order.  The device counterpart of meshproc.keep_components_with_at_least: the
    same kept faces and the same compacted vertices for the same input.  A mesh with degenerate faces is refused (they belong to
    no component here, while meshproc counts them: drop them first)."""
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertices must be [V, 3], got {tuple(vertices.shape)}")
    MeshTopology._check(faces)
    if not vertices.is_cuda:
        raise RuntimeError(MeshTopology._no_cpu())
    f = faces.long()
    if f.shape[0] == 0:
        return vertices, f
    topo = MeshTopology(f, vertices.shape[0])
    if topo.num_degenerate:
        raise ValueError(f"{topo.num_degenerate} faces have two equal indices: drop them first (meshproc.drop_degenerate_faces)")
    labels, sizes = topo.components("vertex")
    kept = f[sizes[labels] >= int(min_faces)]
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=f.device)
    used[kept.reshape(-1)] = True
    remap = torch.cumsum(used.long(), 0) - 1
    return vertices[used], remap[kept]


def is_closed(triangles: Tensor, num_vertices: Optional[int] = None) -> bool:
    """exact: no degenerate face and every edge has valence 2 (voxelize.is_closed is a column-parity approximation)"""
    topo = MeshTopology(triangles, num_vertices)
    return topo.num_degenerate == 0 and bool((topo.valence == 2).all())
