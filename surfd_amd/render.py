"""Views of a mesh on the MI355X path: depth, normals, masks, a headlight shading and contour drawings.

  look_at, orbit_cameras       cameras, built in fp64 and handed over as fp32 [n, 18]
  Renderer, render_mesh        mesh -> per-pixel buffers (csrc/raster.hip; device tensors in, device tensors out)
  Renderer.contours            buffers -> ink images (the line drawings sketch_clip_tensor expects)
  condition_image / _sketch    a view as the (uint8 RGB, mask) pair of preprocess.masked_crops / the PIL image of
                               preprocess.sketch_clip_tensor
  to_uint8, write_png, read_png  8-bit PNG files through zlib (nothing else is imported)

No reference counterpart: the reference looks at meshes in open3d / pymeshlab windows and takes its condition images from
files.  The renderer is two-sided (the project's surfaces are open and unoriented): no back-face culling, normals turned to the
viewer.  It runs in the library and nowhere else; CPU tensors are refused (no CPU fallback).

A camera is 18 floats: the row-major 3x4 world->camera matrix (camera x right, y down, z forward), then mode (0 perspective,
1 orthographic), fx, fy, cx, cy in pixels and near.  Pixel (i, j) = column i of row j has its centre at (i + 0.5, j + 0.5).
"""
from __future__ import annotations

import ctypes as C
import math
import struct
import zlib
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _native as N

CAMERA_FLOATS = 18
FORCE_SMALL = 1                 # SURFD_RASTER_FORCE_SMALL
FORCE_LARGE = 2                 # SURFD_RASTER_FORCE_LARGE
MAX_VIEWS = 64
MAX_SIZE = 2048
MODES = {"perspective": 0.0, "orthographic": 1.0}


# ---- cameras --------------------------------------------------------------------------------------------------------------------
def _look_at64(eye, target, up) -> np.ndarray:
    e, t, u = (np.asarray(a, np.float64).reshape(3) for a in (eye, target, up))
    fwd = t - e
    if not np.linalg.norm(fwd) > 0:
        raise ValueError("look_at: eye and target coincide")
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, u)
    if not np.linalg.norm(right) > 1e-12:
        raise ValueError("look_at: up is parallel to the viewing direction")
    right = right / np.linalg.norm(right)
    rot = np.stack([right, np.cross(fwd, right), fwd])
    return np.concatenate([rot, -(rot @ e)[:, None]], 1)


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)) -> Tensor:
    """[3, 4] float32 world->camera matrix of a camera at ``eye`` looking at ``target``: rows right, down, forward (fp64 inside)"""
    return torch.from_numpy(_look_at64(eye, target, up).astype(np.float32))


def _size(size) -> Tuple[int, int]:
    H, W = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        raise ValueError(f"size must lie in [1, {MAX_SIZE}], got {(H, W)}")
    return H, W


def make_camera(world_to_camera, mode: str = "perspective", fov_deg: float = 40.0, ortho_half: float = 1.2, size=224, near: float = 0.05) -> Tensor:
    """[18] float32: the matrix plus intrinsics that put the vertical and horizontal field of view ``fov_deg`` (perspective) or the
    half-extent ``ortho_half`` (orthographic) on the shorter image side, principal point at the image centre"""
    if mode not in MODES:
        raise ValueError(f"mode must be 'perspective' or 'orthographic', got {mode!r}")
    H, W = _size(size)
    half = min(H, W) / 2.0
    if mode == "perspective":
        if not 0.0 < fov_deg < 180.0:
            raise ValueError("fov_deg must lie in (0, 180)")
        f = half / math.tan(math.radians(fov_deg) / 2.0)
    else:
        if not ortho_half > 0:
            raise ValueError("ortho_half must be positive")
        f = half / ortho_half
    m = np.asarray(world_to_camera, np.float64).reshape(12)
    return torch.from_numpy(np.concatenate([m, [MODES[mode], f, f, W / 2.0, H / 2.0, near]]).astype(np.float32))


def orbit_cameras(n_views: int, elevation_deg: float = 20.0, distance: float = 2.6, mode: str = "perspective", fov_deg: float = 40.0,
                  size=224, ortho_half: float = 1.2, near: float = 0.05, target=(0.0, 0.0, 0.0)) -> Tensor:
    """[n_views, 18] float32: cameras on a circle around the y axis at ``elevation_deg`` above the xz plane, ``distance`` from
    ``target``, azimuths k * 360 / n_views starting on the +z side"""
    if n_views < 1:
        raise ValueError("n_views must be positive")
    el = math.radians(elevation_deg)
    tg = np.asarray(target, np.float64)
    cams = []
    for k in range(n_views):
        az = 2.0 * math.pi * k / n_views
        eye = tg + distance * np.array([math.cos(el) * math.sin(az), math.sin(el), math.cos(el) * math.cos(az)])
        cams.append(make_camera(_look_at64(eye, tg, (0.0, 1.0, 0.0)), mode, fov_deg, ortho_half, size, near))
    return torch.stack(cams)


# ---- checks ---------------------------------------------------------------------------------------------------------------------
def _check_mesh(vertices: Tensor, faces: Tensor) -> None:
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
    if not vertices.is_contiguous() or not faces.is_contiguous():
        raise ValueError("vertices and faces must be contiguous")
    if not (vertices.is_cuda and faces.is_cuda):
        raise ValueError("the renderer runs only on the GPU through libsurfd_hip.so (no CPU fallback): move the mesh with .cuda()")
    if vertices.device != faces.device:
        raise ValueError(f"vertices are on {vertices.device}, faces on {faces.device}")


def _check_cameras(cameras, max_views: int) -> Tensor:
    if not isinstance(cameras, Tensor):
        raise TypeError("cameras must be a tensor [n_views, 18] (orbit_cameras, make_camera)")
    if cameras.dim() == 1:
        cameras = cameras[None]
    if cameras.dim() != 2 or cameras.shape[1] != CAMERA_FLOATS:
        raise ValueError(f"cameras must be [n_views, {CAMERA_FLOATS}], got {tuple(cameras.shape)}")
    if cameras.dtype != torch.float32:
        raise TypeError(f"cameras must be float32, got {cameras.dtype}")
    if not 1 <= cameras.shape[0] <= max_views:
        raise ValueError(f"{cameras.shape[0]} views, the renderer was made for 1 .. {max_views}")
    cams = cameras.detach().cpu().contiguous()
    if not bool(torch.isfinite(cams).all()):
        raise ValueError("cameras contain NaN or Inf")
    mode, near = cams[:, 12], cams[:, 17]
    if not bool(((mode == 0) | (mode == 1)).all()):
        raise ValueError("camera mode must be 0 (perspective) or 1 (orthographic)")
    if bool((near < 0).any()) or bool(((mode == 0) & (near <= 0)).any()):
        raise ValueError("near must be >= 0 (> 0 for a perspective camera)")
    return cams


# ---- the renderer ---------------------------------------------------------------------------------------------------------------
class Renderer:
    """A render target of ``size`` (int or (H, W)) for up to ``max_views`` views per call; owns the library's key buffer and
    workspace, so keep it for repeated calls.  One stream at a time per object."""

    def __init__(self, size=224, max_views: int = 8, device=None):
        self._handle = None
        self.H, self.W = _size(size)
        if not 1 <= max_views <= MAX_VIEWS:
            raise ValueError(f"max_views must lie in [1, {MAX_VIEWS}], got {max_views}")
        self.max_views = int(max_views)
        if not torch.cuda.is_available():
            raise ValueError("the renderer runs only on the GPU through libsurfd_hip.so (no CPU fallback)")
        dev = torch.device("cuda") if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"the renderer runs only on the GPU (no CPU fallback), got device {dev}")
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_raster_create(self.H, self.W, self.max_views, C.byref(h)))
        self._handle = h

    def render(self, vertices: Tensor, faces: Tensor, cameras: Tensor, vertex_normals: Optional[Tensor] = None, smooth: bool = False,
               light: Optional[Sequence[float]] = None, ambient: float = 0.3, flags: int = 0) -> Dict[str, Tensor]:
        """-> {"face" [n, H, W] int32 (-1 background), "depth" [n, H, W] float32 (camera z, +inf background), "bary" [n, H, W, 3],
        "normal" [n, H, W, 3] (camera space, towards the viewer), "mask" [n, H, W] uint8, "shaded" [n, H, W] float32,
        "dropped" [n] int32 (triangles left out because a vertex is behind ``near`` or far outside the image)}.
        ``smooth`` takes vertex normals from meshproc.vertex_normals_by_angle (host, fp64), ``smooth="device"`` from
        meshsmooth.vertex_normals_by_angle (the same sums on the GPU, the mesh stays there); ``vertex_normals`` [V, 3] float32
        supplies them; otherwise the geometric face normal is used.  ``light`` is a camera-space direction (default: the
        headlight (0, 0, -1)).  ``flags``: FORCE_SMALL / FORCE_LARGE send every triangle down one path (the same bits).
        Host syncs: one for the index range check (F > 0)."""
        _check_mesh(vertices, faces)
        if vertices.device != self.device:
            raise ValueError(f"the mesh is on {vertices.device}, the renderer on {self.device}")
        cams = _check_cameras(cameras, self.max_views)
        if flags not in (0, FORCE_SMALL, FORCE_LARGE):
            raise ValueError(f"flags must be 0, FORCE_SMALL or FORCE_LARGE, got {flags}")
        if not 0.0 <= float(ambient) <= 1.0:
            raise ValueError(f"ambient must lie in [0, 1], got {ambient}")
        lt = None
        if light is not None:
            l64 = np.asarray(light, np.float64).reshape(-1)
            if l64.shape != (3,) or not np.isfinite(l64).all() or not np.linalg.norm(l64) > 0:
                raise ValueError("light must be three finite numbers, not all zero")
            lt = (C.c_float * 3)(*(l64 / np.linalg.norm(l64)))
        V, F, n = vertices.shape[0], faces.shape[0], cams.shape[0]
        if n * max(V, F) >= 2 ** 31:
            raise ValueError("n_views * V and n_views * F must stay below 2^31")
        if vertex_normals is not None and smooth:
            raise ValueError("give vertex_normals or smooth=True, not both")
        if F and V and not bool(torch.isfinite(vertices).all()):
            raise ValueError("vertices contain NaN or Inf")
        if F and (V == 0 or int(faces.min()) < 0 or int(faces.max()) >= V):
            raise ValueError(f"faces name vertices outside [0, {V})")
        if isinstance(smooth, str) and smooth != "device":
            raise ValueError(f"smooth must be False, True or 'device', got {smooth!r}")
        if smooth == "device":
            from .meshsmooth import vertex_normals_by_angle as device_normals
            vertex_normals = device_normals(vertices, faces).float() if V else torch.zeros(0, 3, device=self.device)
        elif smooth:
            from .meshproc import vertex_normals_by_angle
            vn = vertex_normals_by_angle(vertices.cpu().numpy(), faces.cpu().numpy()) if V else np.zeros((0, 3))
            vertex_normals = torch.from_numpy(np.ascontiguousarray(vn, dtype=np.float32)).to(self.device)
        if vertex_normals is not None:
            if not isinstance(vertex_normals, Tensor) or vertex_normals.dtype != torch.float32:
                raise TypeError("vertex_normals must be a float32 tensor")
            if tuple(vertex_normals.shape) != (V, 3) or not vertex_normals.is_contiguous() or vertex_normals.device != self.device:
                raise ValueError(f"vertex_normals must be a contiguous [{V}, 3] tensor on {self.device}")
        f32 = faces if faces.dtype == torch.int32 else faces.to(torch.int32)
        dev, H, W = self.device, self.H, self.W
        out = {"face": torch.empty(n, H, W, device=dev, dtype=torch.int32), "depth": torch.empty(n, H, W, device=dev),
               "bary": torch.empty(n, H, W, 3, device=dev), "normal": torch.empty(n, H, W, 3, device=dev),
               "mask": torch.empty(n, H, W, device=dev, dtype=torch.uint8), "shaded": torch.empty(n, H, W, device=dev),
               "dropped": torch.empty(n, device=dev, dtype=torch.int32)}
        cam_ptr = C.cast(cams.data_ptr(), N.c_f32p)
        with torch.cuda.device(dev):
            N.check(N.lib().surfd_raster_render(self._handle, N.ptr(vertices) if V else None, V, N.ptr(f32) if F else None, F, N.ptr(vertex_normals),
                                                cam_ptr, n, int(flags), lt, float(ambient), N.ptr(out["face"]), N.ptr(out["depth"]),
                                                N.ptr(out["bary"]), N.ptr(out["normal"]), N.ptr(out["mask"]), N.ptr(out["shaded"]),
                                                N.ptr(out["dropped"]), N.stream()))
        return out

    def contours(self, buffers: Dict[str, Tensor], depth_jump: float = 0.05, crease_deg: float = 30.0) -> Tensor:
        """buffers of ``render`` -> ink [n, H, W] uint8: 1 where the mask, the depth (by more than ``depth_jump``) or the normal
        (by more than ``crease_deg`` degrees) breaks against a 4-neighbour; the image border counts as background"""
        mask, depth, normal = buffers["mask"], buffers["depth"], buffers["normal"]
        n = mask.shape[0]
        if tuple(mask.shape) != (n, self.H, self.W) or tuple(depth.shape) != (n, self.H, self.W) or tuple(normal.shape) != (n, self.H, self.W, 3):
            raise ValueError(f"buffers are not those of a {self.H} x {self.W} render")
        if mask.dtype != torch.uint8 or depth.dtype != torch.float32 or normal.dtype != torch.float32:
            raise TypeError("mask must be uint8, depth and normal float32")
        if not all(t.is_cuda and t.device == self.device and t.is_contiguous() for t in (mask, depth, normal)):
            raise ValueError(f"buffers must be contiguous tensors on {self.device} (no CPU fallback)")
        if not 1 <= n <= MAX_VIEWS:
            raise ValueError(f"1 .. {MAX_VIEWS} views per call, got {n}")
        if not depth_jump >= 0 or not 0.0 <= crease_deg <= 180.0:
            raise ValueError("depth_jump must be >= 0 and crease_deg in [0, 180]")
        ink = torch.empty(n, self.H, self.W, device=self.device, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            N.check(N.lib().surfd_raster_contours(self._handle, N.ptr(mask), N.ptr(depth), N.ptr(normal), n, float(depth_jump),
                                                  cos_crease(crease_deg), N.ptr(ink), N.stream()))
        return ink

    def __del__(self):
        try:
            if self._handle is not None:
                N.lib().surfd_raster_destroy(self._handle)
        except Exception:                                       # interpreter shutdown
            pass


def cos_crease(crease_deg: float) -> float:
    """the fp32 threshold the contour kernel compares normals' dot products with"""
    return float(np.float32(math.cos(math.radians(crease_deg))))


def render_mesh(vertices: Tensor, faces: Tensor, n_views: int = 8, size=224, elevation_deg: float = 20.0, distance: float = 2.6,
                mode: str = "perspective", fov_deg: float = 40.0, smooth: bool = False, contours: bool = False, depth_jump: float = 0.05,
                crease_deg: float = 30.0, ambient: float = 0.3, cameras: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """one call: orbit cameras (or ``cameras``) -> the buffers of Renderer.render plus "cameras" and, with ``contours``, "ink" """
    _check_mesh(vertices, faces)
    if cameras is None:
        cameras = orbit_cameras(n_views, elevation_deg, distance, mode=mode, fov_deg=fov_deg, size=size)
    r = Renderer(size, max_views=max(1, min(MAX_VIEWS, cameras.shape[0] if cameras.dim() == 2 else 1)), device=vertices.device)
    out = r.render(vertices, faces, cameras, smooth=smooth, ambient=ambient)
    if contours:
        out["ink"] = r.contours(out, depth_jump, crease_deg)
    out["cameras"] = cameras
    return out


# ---- images ---------------------------------------------------------------------------------------------------------------------
def to_uint8(x, lo: Optional[float] = None, hi: Optional[float] = None, background: int = 255) -> np.ndarray:
    """a float image (tensor or array; non-finite = background) -> uint8 by mapping [lo, hi] (default: its finite range) to
    [0, 255]"""
    a = x.detach().cpu().numpy() if isinstance(x, Tensor) else np.asarray(x)
    a = a.astype(np.float64)
    fin = np.isfinite(a)
    lo = float(a[fin].min()) if lo is None and fin.any() else (0.0 if lo is None else lo)
    hi = float(a[fin].max()) if hi is None and fin.any() else (1.0 if hi is None else hi)
    scale = 255.0 / (hi - lo) if hi > lo else 0.0
    out = np.clip(np.rint((np.where(fin, a, lo) - lo) * scale), 0, 255).astype(np.uint8)
    out[~fin] = background
    return out


def depth_image(buffers: Dict[str, Tensor], view: int) -> np.ndarray:
    """uint8 [H, W]: near = dark, far = light, background white"""
    return to_uint8(buffers["depth"][view])


def normal_image(buffers: Dict[str, Tensor], view: int) -> np.ndarray:
    """uint8 [H, W, 3]: (n + 1) / 2 with the camera's y and z negated (the usual normal-map colours), background white"""
    n = buffers["normal"][view].detach().cpu().numpy() * np.array([1.0, -1.0, -1.0])
    m = buffers["mask"][view].detach().cpu().numpy().astype(bool)
    img = to_uint8(n, -1.0, 1.0)
    img[~m] = 255
    return img


def shaded_image(buffers: Dict[str, Tensor], view: int) -> np.ndarray:
    """uint8 [H, W]: the headlight shading, background white"""
    s = to_uint8(buffers["shaded"][view], 0.0, 1.0)
    s[~buffers["mask"][view].detach().cpu().numpy().astype(bool)] = 255
    return s


def condition_image(buffers: Dict[str, Tensor], view: int) -> Tuple[np.ndarray, np.ndarray]:
    """(uint8 RGB [H, W, 3], mask [H, W] uint8 of 0 / 1): the pair preprocess.masked_crops takes (grey shading on black)"""
    m = buffers["mask"][view].detach().cpu().numpy().astype(np.uint8)
    s = to_uint8(buffers["shaded"][view], 0.0, 1.0) * m
    return np.repeat(s[:, :, None], 3, axis=2), m


def condition_sketch(ink, view: Optional[int] = None):
    """ink [H, W] (or [n, H, W] with ``view``) -> PIL RGB image, black lines on white: what preprocess.sketch_clip_tensor takes"""
    from PIL import Image
    a = ink.detach().cpu().numpy() if isinstance(ink, Tensor) else np.asarray(ink)
    if view is not None:
        a = a[view]
    if a.ndim != 2:
        raise ValueError(f"ink must be [H, W], got {a.shape}")
    g = np.where(a != 0, 0, 255).astype(np.uint8)
    return Image.fromarray(np.repeat(g[:, :, None], 3, axis=2))


def save_views(out_dir, stem: str, buffers: Dict[str, Tensor]) -> list:
    """writes <stem>_v<k>_{shaded,depth,normal}.png (and _ink.png when the buffers hold "ink") for every view -> the paths"""
    import os
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for k in range(buffers["mask"].shape[0]):
        images = {"shaded": shaded_image(buffers, k), "depth": depth_image(buffers, k), "normal": normal_image(buffers, k)}
        if "ink" in buffers:
            images["ink"] = np.asarray(condition_sketch(buffers["ink"], k))
        for name, img in images.items():
            paths.append(os.path.join(out_dir, f"{stem}_v{k}_{name}.png"))
            write_png(paths[-1], img)
    return paths


_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"
_PNG_COLOR = {1: 0, 3: 2, 4: 6}        # channels -> PNG colour type


def write_png(path, image) -> None:
    """uint8 [H, W], [H, W, 1], [H, W, 3] or [H, W, 4] -> an 8-bit PNG file (filter 0, zlib)"""
    a = np.asarray(image)
    if a.dtype != np.uint8:
        raise TypeError(f"write_png takes uint8 images, got {a.dtype}")
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in _PNG_COLOR or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png takes [H, W], [H, W, 3] or [H, W, 4], got {a.shape}")
    H, W, ch = a.shape

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    raw = np.concatenate([np.zeros((H, 1), np.uint8), np.ascontiguousarray(a).reshape(H, W * ch)], 1).tobytes()
    with open(path, "wb") as fh:
        fh.write(_PNG_MAGIC + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, _PNG_COLOR[ch], 0, 0, 0))
                 + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def read_png(path) -> np.ndarray:
    """an 8-bit, non-interlaced grey / RGB / RGBA PNG -> uint8 [H, W] or [H, W, C] (all five row filters)"""
    data = open(path, "rb").read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f"{path} is not a PNG file")
    pos, idat, head = 8, [], None
    while pos + 8 <= len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(tag + body) & 0xFFFFFFFF:
            raise ValueError(f"{path}: chunk {tag!r} fails its checksum")
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
        pos += 12 + n
    if head is None:
        raise ValueError(f"{path}: no IHDR chunk")
    W, H, bits, color, _, _, interlace = head
    ch = {0: 1, 2: 3, 6: 4}.get(color)
    if bits != 8 or ch is None or interlace:
        raise ValueError(f"{path}: only 8-bit non-interlaced grey / RGB / RGBA PNGs are read")
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(H, 1 + W * ch)
    out = np.zeros((H, W * ch), np.int64)
    prev = np.zeros(W * ch, np.int64)
    for j in range(H):
        ft, line = int(raw[j, 0]), raw[j, 1:].astype(np.int64)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft in (1, 3, 4):
            cur = np.zeros(W * ch, np.int64)
            for k in range(W * ch):
                a = cur[k - ch] if k >= ch else 0
                b = prev[k]
                c = prev[k - ch] if k >= ch else 0
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[k] = (line[k] + p) & 255
        else:
            raise ValueError(f"{path}: unknown row filter {ft}")
        out[j] = prev = cur
    img = out.astype(np.uint8).reshape(H, W, ch)
    return img[:, :, 0] if ch == 1 else img
