"""The contract of csrc/winding.hip restated in numpy, decision for decision.

Generalized winding number w(p) of a triangle mesh: the signed solid angle of the mesh seen from p over 4 pi.  Vertices and
queries are fp32, every operation below is one fp64 IEEE rounding in the order written (numpy never fuses a multiply and an add).

  term   query p, triangle (A, B, C) in the caller's corner order:
         a = A - p, b = B - p, c = C - p, both operands converted to fp64 first;
         la = sqrt((a.x a.x + a.y a.y) + a.z a.z), lb, lc likewise;
         det = (a.x (b.y c.z - b.z c.y) + a.y (b.z c.x - b.x c.z)) + a.z (b.x c.y - b.y c.x);
         ab = (a.x b.x + a.y b.y) + a.z b.z, bc, ca likewise;
         den = ((la lb) lc + ab lc) + (bc la + ca lb);
         theta = atan2(det, den), and theta = +0 when det == 0.
  sum    triangles in the caller's order.  chunk = 256 consecutive triangles, s_c = the left-to-right sum of its theta from +0;
         group = 16 consecutive chunks, S_g = the left-to-right sum of its s_c from +0; Theta = the left-to-right sum of the S_g
         from +0; w = Theta / 6.283185307179586.
  special  a query that holds a NaN or an Inf: w = NaN.

det and den have the same bits as on the device; atan2 is the only operation that may differ, by a few ulp of a value of at most
pi.  Left-to-right sums are np.cumsum(...)[..., -1] (np.sum adds pairwise).
"""
from __future__ import annotations

import numpy as np

F64 = np.float64
CHUNK = 256
GROUP_CHUNKS = 16
TWO_PI = F64(6.283185307179586)
assert TWO_PI.view(np.uint64) == 0x401921FB54442D18


def tolerance(F):
    """|w_gpu - w_ref| <= F 2^-50: each of the two atan2 is within a few ulp of a value <= pi (1.3e-15 in theta, 2.1e-16 in w), the
    summation rounding over terms that differ by that much is of the same order; 2^-50 per triangle is four times that"""
    return F * 2.0 ** -50


def _corners(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float32)
    f = np.asarray(triangles).astype(np.int64)
    return v[f[:, 0]].astype(F64), v[f[:, 1]].astype(F64), v[f[:, 2]].astype(F64)


def _ltr(x):
    """left-to-right sum over the last axis, from +0"""
    if x.shape[-1] == 0:
        return np.zeros(x.shape[:-1], dtype=F64)
    return (F64(0.0) + np.cumsum(x, axis=-1))[..., -1]


def theta(points, A, B, C):
    """[Q, T] fp64: the term of every (query, triangle) pair; A, B, C are [T, 3] fp64, points [Q, 3] fp32 (finite)"""
    p = np.asarray(points, dtype=np.float32).astype(F64)[:, None, :]
    a, b, c = A[None] - p, B[None] - p, C[None] - p
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    bx, by, bz = b[..., 0], b[..., 1], b[..., 2]
    cx, cy, cz = c[..., 0], c[..., 1], c[..., 2]
    la = np.sqrt((ax * ax + ay * ay) + az * az)
    lb = np.sqrt((bx * bx + by * by) + bz * bz)
    lc = np.sqrt((cx * cx + cy * cy) + cz * cz)
    det = (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx)
    ab = (ax * bx + ay * by) + az * bz
    bc = (bx * cx + by * cy) + bz * cz
    ca = (cx * ax + cy * ay) + cz * az
    den = ((la * lb) * lc + ab * lc) + (bc * la + ca * lb)
    return np.where(det == 0.0, F64(0.0), np.arctan2(det, den))


def _blocks(Q, budget=400_000):
    """query blocks such that a block times one chunk of triangles stays small"""
    step = max(1, budget // CHUNK)
    return [(a, min(Q, a + step)) for a in range(0, Q, step)]


def chunk_sums(vertices, triangles, points):
    """[Q, nchunk] fp64: s_c of every query (non-finite queries are evaluated at the origin; winding_number overwrites them)"""
    A, B, C = _corners(vertices, triangles)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    ok = np.isfinite(pts).all(1)
    pts = np.where(ok[:, None], pts, np.float32(0))
    F = len(A)
    nchunk = -(-F // CHUNK)
    out = np.zeros((len(pts), nchunk), dtype=F64)
    for lo, hi in _blocks(len(pts)):
        for c in range(nchunk):
            s = slice(c * CHUNK, min(F, (c + 1) * CHUNK))
            out[lo:hi, c] = _ltr(theta(pts[lo:hi], A[s], B[s], C[s]))
    return out, ok


def winding_number(vertices, triangles, points, group_chunks=GROUP_CHUNKS):
    """[Q] fp64.  ``group_chunks``: the contract is 16; None adds all chunk sums as one left-to-right sum (tests only)"""
    s, ok = chunk_sums(vertices, triangles, points)
    if group_chunks is None:
        total = _ltr(s)
    else:
        ngroup = -(-s.shape[1] // group_chunks)
        S = np.stack([_ltr(s[:, g * group_chunks:(g + 1) * group_chunks]) for g in range(ngroup)], axis=1)
        total = _ltr(S)
    w = total / TWO_PI
    w[~ok] = np.nan
    return w


def winding_number_flat(vertices, triangles, points):
    """the same terms added as ONE left-to-right sum over all triangles: not the contract, the comparison that shows the
    association is stated"""
    A, B, C = _corners(vertices, triangles)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(len(pts), dtype=F64)
    for lo, hi in _blocks(len(pts), budget=400_000 * CHUNK // max(len(A), 1)):
        out[lo:hi] = _ltr(theta(pts[lo:hi], A, B, C))
    return out / TWO_PI


def occupancy(w, threshold=0.5):
    """|w| >= threshold; a NaN is outside"""
    with np.errstate(invalid="ignore"):
        return np.abs(w) >= threshold


def decided(w_ref, F, threshold=0.5):
    """the queries whose occupancy cannot depend on atan2's last bits: ||w_ref| - threshold| > F 2^-50"""
    return np.abs(np.abs(w_ref) - threshold) > tolerance(F)


# ---- the holed sphere of the issue --------------------------------------------------------------------------------------------
def holed_sphere(subdivisions=3, per_hole=32):
    """raycast_ref.icosphere(subdivisions) without the ``per_hole`` faces whose unit centroid direction has the largest component
    along +x, then +y, then +z.  -> (vertices, faces, hole centres [3, 3]: the mean removed-face centroid of each hole)"""
    import raycast_ref as rr
    v, f = rr.icosphere(subdivisions)
    cen = v[f].astype(F64).mean(1)
    unit = cen / np.linalg.norm(cen, axis=1, keepdims=True)
    keep = np.ones(len(f), dtype=bool)
    holes = []
    for axis in range(3):
        score = np.where(keep, unit[:, axis], -np.inf)
        gone = np.argsort(-score, kind="stable")[:per_hole]
        keep[gone] = False
        holes.append(cen[gone].mean(0))
    return v, f[keep], np.array(holes)


def holed_sphere_queries(holes, n=8000, seed=2, radius=0.75):
    """-> (queries [n, 3] fp32, kept [n] bool: more than 0.05 from the sphere and more than 0.35 from every hole centre,
    inside [n] bool: |p| < radius)"""
    q = np.random.default_rng(seed).uniform(-0.8, 0.8, (n, 3)).astype(np.float32)
    r = np.linalg.norm(q.astype(F64), axis=1)
    kept = np.abs(r - radius) > 0.05
    for h in holes:
        kept &= np.linalg.norm(q.astype(F64) - h, axis=1) > 0.35
    return q, kept, r < radius
