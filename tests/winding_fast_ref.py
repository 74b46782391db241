"""The fast path of csrc/winding.hip restated in numpy, decision for decision: the moments of the box
hierarchy's entries, the records a parent keeps for its children, and the walk that replaces a far entry by its dipole term.

The tree is the one of csrc/meshbvh.hip over the handle's triangles (absolute corners): tests/bvh_ref.py builds it.  Vertices
and queries are fp32, converted to fp64 first; every operation below is one fp64 IEEE rounding in the order written.  Only
+ - * / sqrt occur outside the exact term (tests/winding_ref.py: theta), so everything but that term's atan2 has the device's bits.

  moments  triangle (A, B, C) in the caller's corner order, u = B - A, v = C - A:
           n = 0.5 (u x v) with n.x = 0.5 (u.y v.z - u.z v.y), n.y = 0.5 (u.z v.x - u.x v.z), n.z = 0.5 (u.x v.y - u.y v.x);
           a = sqrt((n.x n.x + n.y n.y) + n.z n.z);  c = ((A + B) + C) / 3.
  sums     of an entry: (sum a, sum a c [3], sum n [3]).  A leaf adds its triangles in slot order, left to right from +0, empty
           slots (-1) skipped, the product a c.x formed first.  A node adds the sums of its existing children in ascending order,
           left to right from +0.
  record   of an entry, in slot c of its parent: (p.x, p.y, p.z, N.x, N.y, N.z, R2).  p = sum a c / sum a where sum a > 0, else
           (lo + hi) 0.5 of the entry's fp32 box (converted first);  N = sum n;  R2 = (m.x m.x + m.y m.y) + m.z m.z with
           m.j = (p.j - lo.j) > (hi.j - p.j) ? (p.j - lo.j) : (hi.j - p.j).  The box (-inf, +inf) gives R2 = +inf.
           An absent child slot is (0, 0, 0, 0, 0, 0, -1): no squared radius is negative.
  walk     finite p.  bvh_next / bvh_enter from the root, all four slots of a node wait when it is entered, ascending order.
           For the slot taken: R2 < 0: nothing.  r = p~ - p, d2 = (r.x r.x + r.y r.y) + r.z r.z.
           d2 > (beta beta) R2: S = S + (((N.x r.x + N.y r.y) + N.z r.z) / (d2 sqrt(d2))) 0.5, no descent (a cluster term).
           Otherwise (a NaN compares false) descend; in a leaf S = S + theta of its triangles in slot order (triangle terms).
           w = S / 6.283185307179586.  A query that holds a NaN or an Inf: w = NaN, no terms.

The walk below runs all queries in lockstep, one slot per step and query, as the kernel's lanes do; a query's sum is added in its
own walk order, so its bits do not depend on the other queries."""
from __future__ import annotations

import numpy as np

import bvh_ref as br
import winding_ref as wr

F64 = np.float64
ABSENT = np.array([0, 0, 0, 0, 0, 0, -1], dtype=F64)


def check_beta(beta):
    beta = float(beta)
    if not beta >= 1.0:                                                  # a NaN fails too
        raise ValueError(f"beta must be a finite number >= 1 or +inf, got {beta}")
    return beta


def tolerance(terms):
    """|w_gpu - w_ref| <= max(T, 1) 2^-50, T the query's number of terms: only the triangle terms' atan2 may differ
    (winding_ref.tolerance has the argument)"""
    return np.maximum(np.asarray(terms, dtype=F64), 1.0) * 2.0 ** -50


def triangle_moments(vertices, triangles):
    """-> (a [F], ac [F, 3], n [F, 3]) fp64"""
    v = np.asarray(vertices, dtype=np.float32)
    f = np.asarray(triangles).astype(np.int64)
    A, B, C = (v[f[:, k]].astype(F64) for k in range(3))
    u, w = B - A, C - A
    with np.errstate(all="ignore"):
        n = np.stack([F64(0.5) * (u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]),
                      F64(0.5) * (u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]),
                      F64(0.5) * (u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0])], 1)
        a = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        c = ((A + B) + C) / F64(3.0)
        return a, a[:, None] * c, n


def _records(sums, lo, hi):
    """sums [E, 7], lo / hi [E, 3] float32 -> records [E, 7]"""
    lo, hi = lo.astype(F64), hi.astype(F64)
    with np.errstate(all="ignore"):
        heavy = sums[:, 0] > 0
        p = np.where(heavy[:, None], sums[:, 1:4] / sums[:, 0:1], (lo + hi) * F64(0.5))
        below, above = p - lo, hi - p
        m = np.where(below > above, below, above)
        R2 = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
    return np.concatenate([p, sums[:, 4:7], R2[:, None]], 1)


def _add_children(vals, exists):
    """vals [n, 4, 7], exists [n, 4] -> [n, 7]: left to right from +0 over the children that exist"""
    s = np.zeros((vals.shape[0], 7), dtype=F64)
    with np.errstate(all="ignore"):
        for c in range(br.W):
            s = np.where(exists[:, c:c + 1], s + vals[:, c], s)
    return s


def build(vertices, triangles):
    """-> dict(lay, order, leaves [nleaf, 4], boxes [nodes, 6, 4] (bvh_ref.build), records [nodes, 4, 7] fp64,
    corners (A, B, C) [F, 3] fp64): what WindingScene.read_bvh returns, and what walk() needs"""
    corners, _ = br.corners_absolute(vertices, triangles)
    tree = br.build(corners)
    lay, leaves, boxes = tree["lay"], tree["leaves"], tree["boxes"]
    a, ac, n = triangle_moments(vertices, triangles)
    tri = np.concatenate([a[:, None], ac, n], 1)                         # [F, 7]
    sums = _add_children(tri[np.maximum(leaves, 0)], leaves >= 0)        # the leaves' sums
    records = np.empty((lay["nodes"], br.W, 7), dtype=F64)
    for k in range(lay["levels"]):
        size, off = lay["size"][k], lay["off"][k]
        pad = size * br.W - len(sums)
        exists = (np.arange(size * br.W) < len(sums)).reshape(size, br.W)
        box = boxes[off:off + size]                                      # [size, 6, 4]: the children's boxes
        lo = box[:, :3].transpose(0, 2, 1).reshape(-1, 3)[:len(sums)]
        hi = box[:, 3:].transpose(0, 2, 1).reshape(-1, 3)[:len(sums)]
        rec = np.concatenate([_records(sums, lo, hi), np.tile(ABSENT, (pad, 1))])
        records[off:off + size] = rec.reshape(size, br.W, 7)
        padded = np.concatenate([sums, np.zeros((pad, 7), dtype=F64)]).reshape(size, br.W, 7)
        sums = _add_children(padded, exists)                             # the sums of this level's nodes
    v = np.asarray(vertices, dtype=np.float32)
    f = np.asarray(triangles).astype(np.int64)
    tree.update(records=records, corners=tuple(v[f[:, k]].astype(F64) for k in range(3)), root_sums=sums[0])
    return tree


def theta_pairs(p, A, B, C):
    """winding_ref.theta for pairs: p, A, B, C [n, 3] fp64 -> [n], the same operations in the same order"""
    a, b, c = A - p, B - p, C - p
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    bx, by, bz = b[:, 0], b[:, 1], b[:, 2]
    cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
    la = np.sqrt((ax * ax + ay * ay) + az * az)
    lb = np.sqrt((bx * bx + by * by) + bz * bz)
    lc = np.sqrt((cx * cx + cy * cy) + cz * cz)
    det = (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx)
    ab = (ax * bx + ay * by) + az * bz
    bc = (bx * cx + by * cy) + bz * cz
    ca = (cx * ax + cy * ay) + cz * az
    den = ((la * lb) * lc + ab * lc) + (bc * la + ca * lb)
    return np.where(det == 0.0, F64(0.0), np.arctan2(det, den))


def walk(tree, points, beta):
    """-> (w [Q] fp64, cluster terms [Q], triangle terms [Q]) of the tree of build()"""
    beta = check_beta(beta)
    bb = F64(beta) * F64(beta)
    lay, leaves, A, B, C = tree["lay"], tree["leaves"], *tree["corners"]
    flat = tree["records"].reshape(-1, 7)
    off4 = np.asarray(lay["off"], dtype=np.int64) * br.W
    top = lay["levels"] - 1
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    Q = len(pts)
    ok = np.isfinite(pts).all(1)
    p = np.where(ok[:, None], pts, np.float32(0)).astype(F64)
    S = np.zeros(Q, dtype=F64)
    ncl, ntri = np.zeros(Q, dtype=np.int64), np.zeros(Q, dtype=np.int64)
    level = np.full(Q, top, dtype=np.int64)
    node = np.zeros(Q, dtype=np.int64)
    mask = np.where(ok, np.uint64(15) << np.uint64(br.W * top), np.uint64(0))
    live = np.arange(Q)
    bound = (lay["nodes"] * br.W + 1) * 2
    for _ in range(bound):
        # bvh_next: go up while the nibble of the current level is empty; a lane whose root nibble is empty is done
        while True:
            nib = (mask[live] >> (np.uint64(br.W) * level[live].astype(np.uint64))) & np.uint64(15)
            up = (nib == 0) & (level[live] < top)
            if not up.any():
                break
            level[live[up]] += 1
            node[live[up]] //= br.W
        live = live[nib != 0]
        if len(live) == 0:
            break
        nib = nib[nib != 0]
        c = np.log2((nib & (~nib + np.uint64(1))).astype(F64)).astype(np.int64)          # the lowest set bit
        lv, nd = level[live], node[live]
        mask[live] &= ~(np.uint64(1) << (np.uint64(br.W) * lv.astype(np.uint64) + c.astype(np.uint64)))
        child = nd * br.W + c
        assert (nd < np.asarray(lay["size"])[lv]).all()
        rec = flat[off4[lv] + child]
        there = ~(rec[:, 6] < 0)
        with np.errstate(all="ignore"):
            r = rec[:, 0:3] - p[live]
            d2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
            far = there & (d2 > bb * rec[:, 6])
            term = (((rec[:, 3] * r[:, 0] + rec[:, 4] * r[:, 1]) + rec[:, 5] * r[:, 2]) / (d2 * np.sqrt(d2))) * F64(0.5)
        q = live[far]
        S[q] = S[q] + term[far]
        ncl[q] += 1
        down = there & ~far
        enter = down & (lv > 0)
        q = live[enter]
        level[q] -= 1
        node[q] = child[enter]
        mask[q] |= np.uint64(15) << (np.uint64(br.W) * level[q].astype(np.uint64))
        leaf = down & (lv == 0)
        q, ids = live[leaf], leaves[child[leaf]]
        assert (child[leaf] < lay["nleaf"]).all()
        for i in range(br.L):
            has = ids[:, i] >= 0
            qi, f = q[has], ids[has, i]
            S[qi] = S[qi] + theta_pairs(p[qi], A[f], B[f], C[f])
            ntri[qi] += 1
    else:
        raise AssertionError("the walk does not end")
    w = S / wr.TWO_PI
    w[~ok] = np.nan
    return w, ncl, ntri


def winding_number(vertices, triangles, points, beta=2.0, tree=None):
    """[Q] fp64: the fast path's value"""
    return walk(build(vertices, triangles) if tree is None else tree, points, beta)[0]
