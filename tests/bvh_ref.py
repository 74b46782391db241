"""The mesh hierarchy of surfd_amd/csrc/meshbvh.hip restated in numpy: the index arithmetic of csrc/meshbvh_layout.h, the build
(centroids, 63-bit Morton codes, the stable sort, leaves of L, the boxes of every level) and the two box tests (bvr_cannot_hit of
csrc/raycast.hip, bvm_cannot_improve of csrc/meshdist.hip) in float32, operation for operation.  Every float32 operation is one
numpy float32 operation; fmaf is formed through float64 (the product of two float32 is exact there; the sum is then rounded
twice, which can differ from the fused result in the last bit in rare cases: nothing here depends on that bit except the
comparison with the GPU's boxes, where no fmaf occurs for absolute records).

The pair tests themselves are restated elsewhere: tests/raycast_ref.py (rc_pair) and tests/mesh_udf_ref.py (md_pair, float32)."""
from __future__ import annotations

import numpy as np

L = 4
W = 4
MAX_LEVELS = 16
F32 = np.float32
INF = F32(np.inf)
TAME = F32(2.0 ** 20)
F32_MIN = F32(np.finfo(np.float32).tiny)


# ---- meshbvh_layout.h ---------------------------------------------------------------------------------------------------------
def layout(F):
    """-> dict(F, nleaf, levels, nodes, size [levels], off [levels]); level 0 = the nodes above the leaves, the last = the root"""
    assert F >= 1
    nleaf = (F + L - 1) // L
    size, off, below, total = [], [], nleaf, 0
    while True:
        assert len(size) < MAX_LEVELS
        n = (below + W - 1) // W
        size.append(n)
        off.append(total)
        total += n
        if n == 1:
            break
        below = n
    return dict(F=F, nleaf=nleaf, levels=len(size), nodes=total, size=size, off=off)


def below(lay, level):
    return lay["nleaf"] if level == 0 else lay["size"][level - 1]


def child_count(nbelow, node):
    return max(0, min(W, nbelow - node * W))


def walk(lay, children=None):
    """The walk of bvh_next / bvh_enter with the mask word, every index checked.  children(level, node) -> the W-bit set of the
    children to enter (default: all that exist).  -> (leaves in the order met, steps)"""
    top = lay["levels"] - 1
    if children is None:
        children = lambda level, node: (1 << child_count(below(lay, level), node)) - 1
    level, node = top, 0
    mask = (children(top, 0) & 15) << (W * top)
    leaves, steps = [], 0
    bound = lay["nodes"] + lay["nleaf"]
    while True:
        m = (mask >> (W * level)) & 15
        if m == 0:
            if level >= top:
                break
            level += 1
            node //= W
            continue
        c = (m & -m).bit_length() - 1
        mask &= ~(1 << (W * level + c))
        child = node * W + c
        steps += 1
        assert steps <= bound, "the walk does not end"
        assert 0 <= level <= top and node < lay["size"][level], (level, node)
        assert child < below(lay, level) and c < child_count(below(lay, level), node), (level, node, c)
        assert mask < (1 << 64)
        if level == 0:
            leaves.append(child)
        else:
            level -= 1
            node = child
            mask |= (children(level, node) & 15) << (W * level)
    return leaves, steps


def check_layout(nleaf):
    """what tools/meshbvh_layout_check.cpp checks for one leaf count"""
    F = nleaf * L - (nleaf % 3)
    lay = layout(F)
    assert lay["nleaf"] == nleaf
    depth, cap = 1, W
    while cap < nleaf:
        depth, cap = depth + 1, cap * W
    assert lay["levels"] == depth <= MAX_LEVELS and lay["size"][-1] == 1
    assert lay["off"] == [sum(lay["size"][:k]) for k in range(lay["levels"])] and lay["nodes"] == sum(lay["size"])
    leaves, steps = walk(lay)
    assert leaves == list(range(nleaf))
    assert steps == lay["nodes"] + nleaf - 1


# ---- the build ------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def corners_absolute(vertices, triangles):
    """raycast.hip's records: -> (corners [F, 3, 3] float32, widths [F, 3, 3] = 0)"""
    v = np.asarray(vertices, np.float32)
    c = v[np.asarray(triangles, np.int64)]
    return c, np.zeros_like(c)


def corners_relative(vertices, triangles):
    """meshdist.hip's records (a, ab = fl(b - a), ac = fl(c - a)): the corners a, fl(a + ab), fl(a + ac) and by how much each
    coordinate is widened in a box: 2^-22 (|ab_j| + |v1_j|) + FLT_MIN"""
    v = np.asarray(vertices, np.float32)
    p = v[np.asarray(triangles, np.int64)]
    a = p[:, 0]
    with np.errstate(all="ignore"):
        ab, ac = p[:, 1] - a, p[:, 2] - a
        v1, v2 = a + ab, a + ac
        w1 = _fma(np.abs(ab) + np.abs(v1), F32(2.0 ** -22), F32_MIN)
        w2 = _fma(np.abs(ac) + np.abs(v2), F32(2.0 ** -22), F32_MIN)
    return np.stack([a, v1, v2], 1), np.stack([np.zeros_like(a), w1, w2], 1)


def centroids(corners):
    with np.errstate(all="ignore"):
        return ((corners[:, 0] + corners[:, 1]) + corners[:, 2]) * F32(0.3333333432674407958984375)


def _spread21(x):
    out = np.zeros(len(x), np.uint64)
    for b in range(21):
        out |= ((x >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def morton_codes(g):
    """g [F, 3] float32 centroids -> uint64 codes (63 bits; 2^63 - 1 for a centroid that is not finite)"""
    fin = np.isfinite(g).all(1)
    if fin.any():
        lo, hi = g[fin].min(0), g[fin].max(0)
    else:
        lo, hi = np.full(3, INF), np.full(3, -INF)
    with np.errstate(all="ignore"):
        ext = np.max(hi - lo)
        code = np.full(len(g), np.uint64(0x7FFFFFFFFFFFFFFF))
        if ext > 0:
            x = np.minimum(((g - lo) / ext) * F32(2097151.0), F32(2097151.0))
            q = np.where(fin[:, None], x, 0).astype(np.uint64)
        else:
            q = np.zeros((len(g), 3), np.uint64)
    c = _spread21(q[:, 0]) | (_spread21(q[:, 1]) << np.uint64(1)) | (_spread21(q[:, 2]) << np.uint64(2))
    return np.where(fin, c, code)


def build(corners, widths=None):
    """-> dict(lay, order [F] (the stable sort), leaves [nleaf, 4] int32, boxes [nodes, 6, 4] float32): what
    surfd_*_bvh_read returns for a handle whose records give these corners"""
    corners = np.asarray(corners, np.float32)
    widths = np.zeros_like(corners) if widths is None else widths
    F = len(corners)
    lay = layout(F)
    order = np.argsort(morton_codes(centroids(corners)), kind="stable")
    nleaf = lay["nleaf"]
    leaves = np.full(nleaf * L, -1, np.int32)
    leaves[:F] = order
    leaves = leaves.reshape(nleaf, L)
    with np.errstate(all="ignore"):
        lo_t, hi_t = (corners - widths).min(1), (corners + widths).max(1)           # per triangle
        tame_t = (np.abs(corners) <= TAME).all((1, 2))                               # false for a NaN
    pad = lambda x, fill: np.concatenate([x[order], np.full((nleaf * L - F,) + x.shape[1:], fill, x.dtype)]).reshape(nleaf, L, *x.shape[1:])
    lo = pad(lo_t, INF).min(1)
    hi = pad(hi_t, -INF).max(1)
    tame = pad(tame_t, True).all(1)
    lo[~tame], hi[~tame] = -INF, INF
    boxes = np.empty((lay["nodes"], 6, W), np.float32)
    for k in range(lay["levels"]):
        n = lay["size"][k]
        plo = np.concatenate([lo, np.full((n * W - len(lo), 3), INF, np.float32)]).reshape(n, W, 3)
        phi = np.concatenate([hi, np.full((n * W - len(hi), 3), -INF, np.float32)]).reshape(n, W, 3)
        boxes[lay["off"][k]:lay["off"][k] + n, :3] = plo.transpose(0, 2, 1)
        boxes[lay["off"][k]:lay["off"][k] + n, 3:] = phi.transpose(0, 2, 1)
        lo, hi = plo.min(1), phi.max(1)
    return dict(lay=lay, order=order, leaves=leaves, boxes=boxes)


# ---- the ray's box test (raycast.hip: bvr_setup, bvr_axis, bvr_cannot_hit) ------------------------------------------------------
PARALLEL = F32(2.0 ** -40)
POS_REL, POS_ABS = F32(2.0 ** -16), F32(2.0 ** -60)
T_REL, T_ABS = F32(2.0 ** -20), F32(2.0 ** -100)


def ray_box_skip(lo, hi, rays, tmin, hi_t):
    """lo, hi [N, 3], rays [N, 6], hi_t [N] (tmax, or the best t of a cast) -> [N] bool: bvr_cannot_hit, pair by pair"""
    lo, hi, rays = (np.asarray(x, np.float32) for x in (lo, hi, rays))
    hi_t = np.broadcast_to(np.asarray(hi_t, np.float32), (len(rays),))
    tmin = F32(tmin)
    o, d = rays[:, :3], rays[:, 3:]
    with np.errstate(all="ignore"):
        ad = np.abs(d)
        m = ad.max(1)
        lim = m * PARALLEL
        par = ~(ad >= lim[:, None]) | (ad == 0)
        inv = np.where(par, F32(0), F32(1) / np.where(par, F32(1), d)).astype(np.float32)
        tame = (np.abs(o) <= TAME).all(1) & (m >= F32(2.0 ** -20)) & (m <= TAME)
        a, b = lo - o, hi - o
        M = np.maximum(np.abs(a), np.abs(b)).max(1)
        s = _fma(M, POS_REL, POS_ABS)
        a, b = a - s[:, None], b + s[:, None]
        t1, t2 = a * inv, b * inv
        e = _fma(np.maximum(np.abs(t1), np.abs(t2)), T_REL, T_ABS)
        n, f = np.minimum(t1, t2) - e, np.maximum(t1, t2) + e
        near = np.where(par, -INF, n).max(1)
        far = np.where(par, INF, f).min(1)
        out = (par & ((a > 0) | (b < 0))).any(1) | (near > far) | (far < tmin) | (near > hi_t)
        return tame & (M < INF) & out


# ---- the query's box test (meshdist.hip: bvm_box, bvm_cannot_improve) -----------------------------------------------------------
CULL_MARGIN = F32(2.0 ** -16)


def _dot(ax, ay, az, bx, by, bz):
    return _fma(az, bz, _fma(ay, by, ax * bx))


def point_box(lo, hi, q):
    """-> (D2, F2) float32: the squared distances from q to the box and to its farthest corner"""
    lo, hi, q = (np.asarray(x, np.float32) for x in (lo, hi, q))
    with np.errstate(all="ignore"):
        a, b = lo - q, q - hi
        n = np.maximum(np.maximum(a, b), F32(0))
        f = np.maximum(np.abs(a), np.abs(b))
        return _dot(n[..., 0], n[..., 1], n[..., 2], n[..., 0], n[..., 1], n[..., 2]), _dot(f[..., 0], f[..., 1], f[..., 2], f[..., 0], f[..., 1], f[..., 2])


def point_box_bound(D2, F2, best2):
    """the right-hand side of bvm_cannot_improve: the box is skipped when D2 > this"""
    with np.errstate(all="ignore"):
        best2 = np.asarray(best2, np.float32)
        return _fma(best2 + F2, CULL_MARGIN, best2)


def point_box_skip(lo, hi, q, best2):
    D2, F2 = point_box(lo, hi, q)
    return D2 > point_box_bound(D2, F2, best2)
