"""What the two objects that keep one mesh CONNECTIVITY in the library share (meshtopo.MeshTopology, meshsmooth.MeshSmoother;
meshprep._MeshScene is the counterpart for the handles that carry vertices): the handle, the checks of the index and vertex
tensors, and ``_open``, the constructors' common work."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native as N

_ABSENT = object()


class _MeshConnectivity:
    """``_abi`` is the prefix of the library's functions for the handle, ``_what`` names the module in the CPU-tensor refusal,
    ``_vertex_dtypes`` are the position dtypes its calls take."""

    _abi = ""
    _what = ""
    _vertex_dtypes: Tuple[torch.dtype, ...] = (torch.float32,)
    _handle = None

    @classmethod
    def _fn(cls, name: str):
        return getattr(N.lib(), f"{cls._abi}_{name}")

    @classmethod
    def _no_cpu(cls) -> str:
        return f"{cls._what} runs only on the GPU through libsurfd_hip.so (no CPU fallback): move the mesh with .cuda()"

    @classmethod
    def _check(cls, triangles=_ABSENT, vertices=_ABSENT) -> None:
        """the tensors that were given: shapes and dtypes first, the CPU-tensor refusal last"""
        if vertices is not _ABSENT:
            if not isinstance(vertices, Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
                raise ValueError(f"vertices must be a tensor [V, 3], got {tuple(getattr(vertices, 'shape', ()))}")
            if vertices.dtype not in cls._vertex_dtypes:
                names = " or ".join(str(d).replace("torch.", "") for d in cls._vertex_dtypes)
                raise TypeError(f"vertices must be {names}, got {vertices.dtype}")
        if triangles is not _ABSENT:
            if not isinstance(triangles, Tensor) or triangles.dim() != 2 or triangles.shape[1] != 3:
                raise ValueError(f"triangles must be a tensor [F, 3], got {tuple(getattr(triangles, 'shape', ()))}")
            if triangles.dtype not in (torch.int32, torch.int64):
                raise TypeError(f"triangles must be int32 or int64, got {triangles.dtype}")
        if any(t is not _ABSENT and not t.is_cuda for t in (vertices, triangles)):
            raise RuntimeError(cls._no_cpu())

    def _open(self, triangles: Tensor, num_vertices: Optional[int]) -> Tuple[int, int, int, int]:
        """Checks the index tensor, hands it to the library's create and returns the four numbers of its counts.  Host syncs:
        create's own, and with ``num_vertices=None`` the read of the largest index."""
        self._check(triangles=triangles)
        self.device = triangles.device
        F = int(triangles.shape[0])
        if num_vertices is None:
            num_vertices = int(triangles.max()) + 1 if F else 0
        if num_vertices < 0:
            raise ValueError(f"num_vertices must not be negative, got {num_vertices}")
        if 3 * F >= 2 ** 31 or int(num_vertices) >= 2 ** 31:
            raise ValueError(f"3 F and V must stay below 2^31, got F = {F}, V = {num_vertices}")
        if F and triangles.dtype == torch.int64 and (int(triangles.min()) < -2 ** 31 or int(triangles.max()) >= 2 ** 31):
            raise ValueError(f"triangles name vertices outside [0, {num_vertices})")
        self.num_vertices = int(num_vertices)
        self.num_faces = F
        ts = triangles.to(torch.int32).contiguous()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._fn("create")(N.ptr(ts), F, self.num_vertices, N.stream(), C.byref(h)))
        self._handle = h
        c = [C.c_int64() for _ in range(4)]
        N.check(self._fn("counts")(h, *[C.byref(x) for x in c]))
        return tuple(int(x.value) for x in c)

    def _positions(self, vertices: Tensor) -> Tensor:
        """the caller's positions, checked against the handle: contiguous and detached"""
        self._check(vertices=vertices)
        if vertices.shape[0] != self.num_vertices or vertices.device != self.device:
            raise ValueError(f"vertices must be [{self.num_vertices}, 3] on {self.device}, got {tuple(vertices.shape)} on {vertices.device}")
        return vertices.detach().contiguous()

    def __del__(self):
        try:
            if self._handle is not None:
                self._fn("destroy")(self._handle)
        except Exception:                                       # interpreter shutdown
            pass
