"""The cleaning between the mesh stages on the MI355X path: a mesh that lies on the device is merged, rid of its duplicate and flat
faces and of its small holes there.  The device counterpart of the cleaning functions of surfd_amd.meshproc:

  cull_and_merge          Trimesh.process(validate=False)        <- meshproc.cull_and_merge
  drop_duplicate_faces    Trimesh.remove_duplicate_faces         <- meshproc.drop_duplicate_faces
  drop_degenerate_faces   Trimesh.remove_degenerate_faces        <- meshproc.drop_degenerate_faces
  fill_small_holes        Trimesh.fill_holes (3 and 4 edges)     <- meshproc.fill_small_holes
  clean_until_stable      the cleaning loop of get_mesh_from_udf <- meshproc.clean_until_stable

meshproc is the contract: every result equals meshproc's bit for bit and in the same order (vertex order, face order, every
double).  The work runs in csrc/meshclean.hip and nowhere else: device tensors in, device tensors out, CPU tensors are refused
(no CPU fallback).  Vertices are float64 [V, 3] (float32 is widened exactly, as np.asarray(..., float64) does), faces int64
[F, 3] (int32 is accepted); vertices come back float64 and faces int64.  Limits: 3 F < 2^31, V < 2^31; an index outside [0, V) is
the library's SURFD_ERR_ARG (a RuntimeError), found on the device and never a fault; so is a finite coordinate whose quantised
key would reach 2^62.  Nothing is kept between calls; a call works on the current stream.

Host syncs: each of the four steps reads its counts back once, at its end.  clean_until_stable reads the counts that steer
meshproc's loop: 4 syncs on the fast return (nothing removed, nothing capped: the usual marching-cubes output), otherwise 5 and 2
per round, 3 for a round that removed a face.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple, Union

import torch
from torch import Tensor

from . import _native as N
from .meshconn import _MeshConnectivity

MERGE_TOL = 1e-8          # meshproc.MERGE_TOL


class _Clean(_MeshConnectivity):
    _what = "the mesh cleaning"
    _vertex_dtypes = (torch.float32, torch.float64)


def _faces32(faces: Tensor, num_vertices: int) -> Tensor:
    """the index tensor as the library takes it: int32, contiguous; indices that int32 cannot hold are refused here"""
    F = int(faces.shape[0])
    if 3 * F >= 2 ** 31 or num_vertices >= 2 ** 31:
        raise ValueError(f"3 F and V must stay below 2^31, got F = {F}, V = {num_vertices}")
    if faces.dtype == torch.int64:
        if F and (int(faces.min()) < -2 ** 31 or int(faces.max()) >= 2 ** 31):
            raise ValueError("faces name vertices outside the range of int32")
        faces = faces.to(torch.int32)
    return faces.contiguous()


def _vertices64(vertices: Tensor) -> Tensor:
    return vertices.detach().to(torch.float64).contiguous()


def _counts(n: int):
    return (C.c_int64 * n)()


# ---- the steps on (float64 vertices, int32 faces) -----------------------------------------------------------------------------
def _cull(v: Tensor, f: Tensor, tol: float) -> Tuple[Tensor, Tensor, Tuple[int, int, int]]:
    """(vertices, faces, (non-finite, unreferenced, merged vertices))"""
    V, F = int(v.shape[0]), int(f.shape[0])
    if V == 0 or F == 0:
        return v[:0], f[:0], (0, 0, 0)
    if not tol > 0:
        raise ValueError(f"tol must be positive, got {tol}")
    ov, of, c = torch.empty_like(v), torch.empty_like(f), _counts(5)
    with torch.cuda.device(v.device):
        N.check(N.lib().surfd_meshclean_cull_and_merge(N.ptr(v), V, N.ptr(f), F, 1.0 / float(tol), N.ptr(ov), N.ptr(of), c, N.stream()))
    return ov[:c[0]], of[:c[1]], (int(c[2]), int(c[3]), int(c[4]))


def _dedup(f: Tensor) -> Tensor:
    F = int(f.shape[0])
    if F == 0:
        return f
    of, c = torch.empty_like(f), _counts(1)
    with torch.cuda.device(f.device):
        N.check(N.lib().surfd_meshclean_drop_duplicate_faces(N.ptr(f), F, N.ptr(of), c, N.stream()))
    return of[:c[0]]


def _degen(v: Tensor, f: Tensor, height: float) -> Tensor:
    F = int(f.shape[0])
    if F == 0:
        return f
    of, c = torch.empty_like(f), _counts(1)
    with torch.cuda.device(f.device):
        N.check(N.lib().surfd_meshclean_drop_degenerate_faces(N.ptr(v), int(v.shape[0]), N.ptr(f), F, float(height), N.ptr(of), c, N.stream()))
    return of[:c[0]]


def _fill(v: Tensor, f: Tensor) -> Tuple[Tensor, Tuple[int, int]]:
    """(faces, (3-edge caps, 4-edge caps)); the input itself where nothing is capped"""
    V, F = int(v.shape[0]), int(f.shape[0])
    if F < 3:
        return f, (0, 0)
    rows = min(V, 3 * F // 2)
    caps, c = torch.empty(rows, 3, device=f.device, dtype=torch.int32), _counts(3)
    with torch.cuda.device(f.device):
        N.check(N.lib().surfd_meshclean_fill_small_holes(N.ptr(f), F, V, N.ptr(caps), rows, c, N.stream()))
    return (torch.cat([f, caps[:c[0]]]) if c[0] else f), (int(c[1]), int(c[2]))


def _mesh(vertices: Tensor, faces: Tensor) -> Tuple[Tensor, Tensor]:
    _Clean._check(faces, vertices)
    if vertices.device != faces.device:
        raise ValueError(f"vertices and faces must lie on one device, got {vertices.device} and {faces.device}")
    return _vertices64(vertices), _faces32(faces, int(vertices.shape[0]))


# ---- the public surface -------------------------------------------------------------------------------------------------------
def cull_and_merge(vertices: Tensor, faces: Tensor, tol: float = MERGE_TOL) -> Tuple[Tensor, Tensor]:
    """meshproc.cull_and_merge: faces that name a non-finite vertex go; of the vertices the others name, those whose coordinates
    agree after rint(x / tol) become one (the lowest index stays, with its own coordinates); survivors keep their order, faces are
    re-indexed.  Empty vertices or faces give (0, 3), (0, 3)."""
    v, f = _mesh(vertices, faces)
    v, f, _ = _cull(v, f, tol)
    return v, f.long()


def drop_duplicate_faces(faces: Tensor) -> Tensor:
    """meshproc.drop_duplicate_faces: one face per vertex triple (winding and rotation ignored), the lowest face of each class
    with its own winding, IN ASCENDING ORDER of (largest, middle, smallest index): the array is re-ordered even when nothing goes."""
    _Clean._check(faces)
    return _dedup(_faces32(faces, 0)).long()


def drop_degenerate_faces(vertices: Tensor, faces: Tensor, height: float = MERGE_TOL) -> Tensor:
    """meshproc.drop_degenerate_faces: keeps the triangles whose two heights over the edges leaving corner 0 both exceed
    ``height``; the order of the faces is kept."""
    v, f = _mesh(vertices, faces)
    return _degen(v, f, height).long()


def fill_small_holes(vertices: Tensor, faces: Tensor) -> Tensor:
    """meshproc.fill_small_holes: border loops of exactly 3 or 4 edges are closed against the border's direction (a quad by two
    triangles); the caps follow the input faces in ascending order of their smallest vertex.  Larger holes stay open."""
    v, f = _mesh(vertices, faces)
    return _fill(v, f)[0].long()


def clean_until_stable(vertices: Tensor, faces: Tensor, max_iter: int = 10,
                       return_stats: bool = False) -> Union[Tuple[Tensor, Tensor], Tuple[Tensor, Tensor, Dict[str, int]]]:
    """meshproc.clean_until_stable, step for step: cull, duplicate pass, height test, small holes; the fast return where none of
    them changed a count; otherwise another cull and rounds of (duplicate pass, height test, cull where a face went) until the
    counts stand still.  ``return_stats``: also a dict of what the steps did, each summed over the steps that ran:
    merged_vertices, nonfinite_vertices, unreferenced_vertices, duplicate_faces, degenerate_faces, caps3, caps4 (border loops of
    3 and 4 edges closed) and rounds (the duplicate / height passes, the first included: 1 on the fast return)."""
    v, f = _mesh(vertices, faces)
    st = dict.fromkeys(("merged_vertices", "nonfinite_vertices", "unreferenced_vertices", "duplicate_faces", "degenerate_faces", "caps3", "caps4"), 0)

    def cull(v, f):
        v, f, (nonfinite, unreferenced, merged) = _cull(v, f, MERGE_TOL)
        st["nonfinite_vertices"] += nonfinite; st["unreferenced_vertices"] += unreferenced; st["merged_vertices"] += merged
        return v, f

    def passes(v, f):
        n = len(f)
        f = _dedup(f)
        st["duplicate_faces"] += n - len(f)
        n = len(f)
        f = _degen(v, f, MERGE_TOL)
        st["degenerate_faces"] += n - len(f)
        return f

    v, f = cull(v, f)
    n0 = len(f)
    f = passes(v, f)
    n1 = len(f)
    f, (caps3, caps4) = _fill(v, f)
    st["caps3"] += caps3; st["caps4"] += caps4
    st["rounds"] = 1
    if not (n1 == n0 and len(f) == n1):                     # meshproc's fast return: no step changed a count
        v, f = cull(v, f)
        counts, rounds = (0, 0), 0
        while counts != (len(v), len(f)) and rounds < max_iter:
            n_before = len(f)
            f = passes(v, f)
            counts = (len(v), len(f))
            rounds += 1
            st["rounds"] += 1
            if len(f) != n_before:
                v, f = cull(v, f)
    return (v, f.long(), st) if return_stats else (v, f.long())
