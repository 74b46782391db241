"""The auto-encoder's point-cloud encoder on the MI355X path: point clouds -> latents.

  Dgcnn                  <- AutoEncoder/models/dgcnn.py:27-115   (same ctor, state_dict keys, forward)
  knn_points             <- pytorch3d.ops.knn_points(x, x, K)    (self-kNN, the only form dgcnn.py:86 uses)
  random_point_sampling  <- utils/utils.py:44-77

``encoder.load_state_dict(ckpt["encoder"], strict=True)`` and ``.cuda().eval()`` work unchanged.  ``forward`` never computes
in torch: kNN, the four EdgeConv blocks and conv_5 + BN + leaky-ReLU + max run in csrc/dgcnn.hip (plain fp32, bitwise
deterministic, every cloud independent of the others in its batch).  Eval mode only, inference only, no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from . import _native as N


class Dgcnn(nn.Module):
    def __init__(self, size_latent: int, k: int = 20, aggregate_ops_local: str = "max", aggregate_ops_global: str = "max"):
        super().__init__()
        self.k = k
        self.size_latent = size_latent
        self.aggreate_ops_local = aggregate_ops_local           # the reference's attribute names (sic)
        self.aggreate_ops_global = aggregate_ops_global
        self.bn_1 = nn.BatchNorm1d(64)
        self.bn_2 = nn.BatchNorm1d(64)
        self.bn_3 = nn.BatchNorm1d(128)
        self.bn_4 = nn.BatchNorm1d(256)
        self.bn_5 = nn.BatchNorm1d(size_latent)
        self.slope = 0.2
        self.conv_1 = nn.Linear(3 * 2, 64, bias=False)
        self.conv_2 = nn.Linear(64 * 2, 64, bias=False)
        self.conv_3 = nn.Linear(64 * 2, 128, bias=False)
        self.conv_4 = nn.Linear(128 * 2, 256, bias=False)
        self.conv_5 = nn.Linear(512, size_latent, bias=False)
        self._handle = None
        self._binder = N.ParamBinder("surfd_dgcnn_set_param", "surfd_dgcnn_finalize")

    # ---- native handle ----------------------------------------------------------------------------
    def _native(self):
        if self.aggreate_ops_local != "max" or self.aggreate_ops_global != "max":
            raise NotImplementedError(
                f"surfd_amd.dgcnn.Dgcnn implements aggregate_ops_local = aggregate_ops_global = 'max' (got "
                f"{self.aggreate_ops_local!r}, {self.aggreate_ops_global!r}); 'avg' and the per-point output are not supported")
        if not self.conv_1.weight.is_cuda:
            raise RuntimeError("Dgcnn runs only on the GPU through libsurfd_hip.so (no CPU fallback); call .cuda() first")
        L = N.lib()
        if self._handle is None:
            h = C.c_void_p()
            N.check(L.surfd_dgcnn_create(self.size_latent, self.k, C.byref(h)))
            self._handle = h
        self._binder.bind(self, self._handle)
        return L, self._handle

    def _check_input(self, x: Tensor) -> Tensor:
        if x.dim() != 3 or x.shape[-1] != 3:
            raise ValueError(f"Dgcnn expects a point cloud [B, N, 3], got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise TypeError(f"Dgcnn expects float32 points, got {x.dtype}")
        if x.shape[1] < self.k:
            raise ValueError(f"Dgcnn needs at least k = {self.k} points per cloud, got N = {x.shape[1]}")
        if not bool(torch.isfinite(x).all()):
            raise ValueError("Dgcnn input contains NaN or Inf")
        if not x.is_cuda:
            raise RuntimeError("Dgcnn runs only on the GPU through libsurfd_hip.so (no CPU fallback): move the points with .cuda()")
        return x.contiguous()

    # ---- forward ----------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x: Tensor, latent_index: Optional[Tensor] = None) -> Tensor:
        """x [B, N, 3] fp32 -> [B, size_latent] (dgcnn.py:77-115); with latent_index [B] its values are appended as one more
        column (dgcnn.py:112-113)."""
        if self.training:
            raise RuntimeError("surfd_amd.dgcnn.Dgcnn is eval-mode only (BatchNorm with running statistics): call .eval() "
                               "(the reference uses the encoder frozen, AutoEncoder/encdec/export_meshes.py:61-100)")
        L, h = self._native()
        x = self._check_input(x)
        B, n, _ = x.shape
        feat = torch.empty(B, self.size_latent, device=x.device, dtype=torch.float32)
        if B:
            N.check(L.surfd_dgcnn_forward(h, N.ptr(x), B, n, N.ptr(feat), N.stream()))
        if latent_index is not None:
            feat = torch.cat((feat, latent_index.unsqueeze(-1)), dim=1)
        return feat

    @torch.no_grad()
    def forward_features(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        """(forward(x), torch.cat((x1, x2, x3, x4), -1) [B, N, 512]): the EdgeConv features conv_5 reads (dgcnn.py:88-100)"""
        if self.training:
            raise RuntimeError("surfd_amd.dgcnn.Dgcnn is eval-mode only: call .eval()")
        L, h = self._native()
        x = self._check_input(x)
        B, n, _ = x.shape
        feat = torch.empty(B, self.size_latent, device=x.device, dtype=torch.float32)
        x1234 = torch.empty(B, n, 512, device=x.device, dtype=torch.float32)
        if B:
            N.check(L.surfd_dgcnn_forward_features(h, N.ptr(x), B, n, N.ptr(feat), N.ptr(x1234), N.stream()))
        return feat, x1234

    def knn(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        """self-kNN with this module's k: (dists [B, N, k] fp32, idx [B, N, k] int64)"""
        L, h = self._native()
        x = self._check_input(x)
        B, n, _ = x.shape
        d = torch.empty(B, n, self.k, device=x.device, dtype=torch.float32)
        i = torch.empty(B, n, self.k, device=x.device, dtype=torch.int32)
        if B:
            N.check(L.surfd_dgcnn_knn(h, N.ptr(x), B, n, N.ptr(d), N.ptr(i), N.stream()))
        return d, i.long()

    def __del__(self):
        try:
            if self._handle is not None:
                N.lib().surfd_dgcnn_destroy(self._handle)
        except Exception:                                       # interpreter shutdown
            pass


_KNN_CACHE = {}


def knn_points(x: Tensor, K: int) -> Tuple[Tensor, Tensor]:
    """pytorch3d.ops.knn_points(x, x, K=K) without lengths: (dists [B, N, K] squared fp32, idx [B, N, K] int64), sorted
    ascending, every point its own first neighbour, ties broken by the lower index (pytorch3d leaves their order undefined)."""
    if not 1 <= K <= 32:
        raise ValueError(f"knn_points supports 1 <= K <= 32, got {K}")
    dev = x.device.index if x.is_cuda else None
    mod = _KNN_CACHE.get((K, dev))
    if mod is None:
        # the kNN needs no weights: a size-1 encoder handle of this k provides the workspace
        mod = Dgcnn(1, k=K).eval()
        if x.is_cuda:
            mod = mod.to(x.device)
        _KNN_CACHE[(K, dev)] = mod
    return mod.knn(x)


def random_point_sampling(pcd: Tensor, num_points: int, inds: Optional[Tensor] = None) -> Tensor:
    """utils/utils.py:44-77: ``num_points`` points drawn uniformly (torch.multinomial on the global RNG, with replacement when
    the cloud is smaller), or the given ``inds``; pcd [NUM_POINTS, D] or [B, NUM_POINTS, D]."""
    batched = pcd.dim() == 3
    if not batched:
        pcd = pcd.unsqueeze(0)
    batch_size, original_num_points, _ = pcd.shape
    if inds is None:
        weights = torch.ones((batch_size, original_num_points), dtype=torch.float).to(pcd.device)
        replacement = original_num_points < num_points
        indices_to_sample = torch.multinomial(weights, num_points, replacement=replacement)
    else:
        indices_to_sample = inds
    batch_indices = torch.arange(batch_size).reshape(batch_size, 1)
    sampled = pcd[batch_indices, indices_to_sample]
    if not batched:
        sampled = torch.squeeze(sampled, dim=0)
    return sampled
