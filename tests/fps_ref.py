"""Yardstick of the farthest point sampling (surfd_amd/cloudsample.py, csrc/cloudfps.hip).  Neither the code under test nor its
output: numpy restatements of the loop the kernel's header states.

  fps_f32     every elementwise operation on float32 arrays in the stated order (d = p_i - p_s per coordinate,
              d2 = (dx dx + dy dy) + dz dz, one rounding per operation; mind = minimum(mind, d2)); np.argmax returns the first of
              equal maxima, which is the lower-index rule.  -> (idx [K] int64, cover2 [K] float32), -1 / 0 beyond n
  fps_f64     the same loop in fp64
  fps_batch   fps_f32 row by row with per-row lengths and starts
  decisions   how clearly every arg-max of a run is decided: (best - second best) / best of mind, per round
  cover2_of   the squared covering radius of a subset against a cloud, in fp64 (for the evenness comparison)

`python tests/fps_ref.py` prints, for the GPU tests' clouds, whether the fp32 and the fp64 index sequences agree and the smallest
relative gap of an arg-max.  Informative only: the GPU tests require equality with fps_f32 whatever the gaps are (the selection
only selects, so equal inputs give equal picks at any gap, exact ties included).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_ref as R  # noqa: E402


def _fps(x, K, n, start, dtype, gaps=None):
    x = np.ascontiguousarray(x, dtype=dtype)
    n = len(x) if n is None else int(n)
    assert 1 <= n <= len(x) and 0 <= start < n and K >= 1
    px, py, pz = x[:n, 0].copy(), x[:n, 1].copy(), x[:n, 2].copy()
    mind = np.full(n, np.inf, dtype)
    idx = np.full(K, -1, np.int64)
    cover2 = np.zeros(K, dtype)
    s = int(start)
    for k in range(min(K, n)):
        idx[k] = s
        dx, dy, dz = px - px[s], py - py[s], pz - pz[s]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == dtype
        mind = np.minimum(mind, d2)
        s = int(mind.argmax())                          # the first of equal maxima: the lower index
        cover2[k] = mind[s]
        if gaps is not None:
            second = np.partition(mind, n - 2)[n - 2] if n > 1 else 0.0
            gaps.append(float((mind[s] - second) / mind[s]) if mind[s] > 0 else 0.0)
    return idx, cover2


def fps_f32(x, K, n=None, start=0):
    """x [N, 3] -> (idx [K] int64, cover2 [K] float32) of the first n points, picking from index `start`"""
    return _fps(x, K, n, start, np.float32)


def fps_f64(x, K, n=None, start=0):
    return _fps(x, K, n, start, np.float64)


def fps_batch(x, K, lengths=None, start=None):
    """x [B, N, 3] -> (idx [B, K] int64, cover2 [B, K] float32)"""
    B = len(x)
    out = [fps_f32(x[b], K, None if lengths is None else lengths[b], 0 if start is None else int(start[b])) for b in range(B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def decisions(x, K, dtype=np.float64):
    """relative gap between the best and the second-best mind of every round (0 = an exact tie, decided by the index)"""
    gaps = []
    _fps(x, K, None, 0, dtype, gaps)
    return np.array(gaps)


def cover2_of(cloud, subset, rows=2048):
    """max over the cloud's points of the squared distance to the nearest point of the subset, in fp64"""
    c, s = np.asarray(cloud, np.float64), np.asarray(subset, np.float64)
    worst = 0.0
    for r0 in range(0, len(c), rows):
        d = ((c[r0:r0 + rows, None, :] - s[None, :, :]) ** 2).sum(-1)
        worst = max(worst, float(d.min(1).max()))
    return worst


# ---- the hand-written example of tests/test_cloudsample_cpu.py --------------------------------------------------------------------
# six points on a line and beside it; point 4 duplicates point 1; from start 0 the first arg-max is a tie between 2 and 5
HAND_POINTS = np.array([[0, 0, 0], [1, 0, 0], [4, 0, 0], [2, 0, 0], [1, 0, 0], [0, 4, 0]], np.float32)
# round 0: pick 0; mind = [0, 1, 16, 4, 1, 16]: tie of 2 and 5 -> 2, cover2 16
# round 1: pick 2; d2 = [16, 9, 0, 4, 9, 32]; mind = [0, 1, 0, 4, 1, 16] -> 5, cover2 16
# round 2: pick 5; d2 = [16, 17, 32, 20, 17, 0]; mind = [0, 1, 0, 4, 1, 0] -> 3, cover2 4
# round 3: pick 3; d2 = [4, 1, 4, 0, 1, 20]; mind = [0, 1, 0, 0, 1, 0]: tie of 1 and its duplicate 4 -> 1, cover2 1
# round 4: pick 1; mind = [0, 0, 0, 0, 0, 0] -> 0 (the lowest index once everything is covered), cover2 0
# round 5: pick 0 again; cover2 0
# rounds 6, 7: nothing left (K > n): -1, 0
HAND_IDX = [0, 2, 5, 3, 1, 0, -1, -1]
HAND_COVER2 = [16.0, 16.0, 4.0, 1.0, 0.0, 0.0, 0.0, 0.0]


SIZES = ((64, 64), (777, 777), (1025, 100), (2048, 512), (8193, 256), (20000, 128))

if __name__ == "__main__":
    for name, make in (("random_cloud", R.random_cloud), ("lattice_cloud", R.lattice_cloud)):
        for N, K in SIZES:
            x = make(1, N, 7)[0]
            i32, c32 = fps_f32(x, K)
            i64, _ = fps_f64(x, K)
            g = decisions(x, K)
            print(f"{name:14s} N = {N:6d} K = {K:4d}: fp32 and fp64 sequences {'identical' if (i32 == i64).all() else 'DIFFER'}; "
                  f"smallest arg-max gap {g.min():.3e}, exact ties in {int((g == 0).sum())} rounds; distinct points {len(np.unique(x, axis=0))}")
    x = R.family("torus", 1, 100000)[0]
    i32, c32 = fps_f32(x, 2048)
    i64, _ = fps_f64(x, 2048)
    print(f"torus          N = 100000 K = 2048: fp32 and fp64 sequences {'identical' if (i32 == i64).all() else 'DIFFER'}; cover2 = {c32[-1]:.6e}")
