"""Yardsticks of the voxeliser (surfd_amd/csrc/voxel.hip, surfd_amd/voxelize.py); numpy only.

  restatement   the kernel's snap in np.float32, then brute force over (triangle, voxel of the clipped box) in int64:
                surface_ref, solid_ref, points_ref, iou_ref.  Every GPU buffer is required equal to it bit for bit.
  second form   the same decisions in Python integers (arbitrary precision) on the same snapped input: hit_big, column_big,
                surface_big, solid_big.  Where the two agree on coordinates at +-2^19 the int64 products did not overflow.

Grid: the cube [lo, hi]^3 in R^3 closed voxels, axes (x, y, z) = (i, j, k); packed along z as uint32 [R, R, W], W = ceil(R / 32),
bit k & 31 of word k >> 5.  DESIGN.md section 8.5 states the rules."""
import numpy as np

SNAP_MAX = 1 << 19
F32 = np.float32


# ---- snap -------------------------------------------------------------------------------------------------------------------------
def scale(lo, hi, R):
    return F32(256.0 * R / (float(F32(hi)) - float(F32(lo))))


def snap(x, lo, hi, R):
    """-> (q int64, valid bool) of fp32 coordinates: q = rint((x - lo) * s), invalid when NaN or |q| > 2^19"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint((np.asarray(x, F32) - F32(lo)) * scale(lo, hi, R))
        valid = np.abs(r) <= F32(SNAP_MAX)
    return np.where(valid, r, 0).astype(np.int64), valid


def snap_mesh(vertices, faces, lo, hi, R):
    """-> (tri int64 [F, 3, 3], ok bool [F]): ok is False for a triangle with an invalid vertex or an index outside [0, V)"""
    vertices, faces = np.asarray(vertices, F32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    q, valid = snap(vertices, lo, hi, R)
    inside = ((faces >= 0) & (faces < len(vertices))).all(1)
    idx = np.where(inside[:, None], faces, 0)
    ok = inside & valid[idx].all((1, 2)) if len(vertices) else inside & False
    tri = q[idx] if len(vertices) else np.zeros((len(faces), 3, 3), np.int64)
    return tri, ok


def pack(dense):
    """bool [..., R, R, R] -> uint32 [..., R, R, W]"""
    dense = np.asarray(dense, bool)
    R = dense.shape[-1]
    W = (R + 31) // 32
    pad = np.zeros(dense.shape[:-1] + (W * 32,), np.uint64)
    pad[..., :R] = dense
    return (pad.reshape(dense.shape[:-1] + (W, 32)) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def unpack(bits, R):
    bits = np.asarray(bits, np.uint32)
    return ((bits[..., :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(bits.shape[:-1] + (-1,))[..., :R]


# ---- surface: int64 restatement ---------------------------------------------------------------------------------------------------
def normal(t):
    a, b = t[1] - t[0], t[2] - t[0]
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.int64)


def sat_parts(t, ci, cj, ck):
    """triangle t int64 [3, 3] against the voxels (ci, cj, ck) (int64 arrays) -> (box, plane, edges): True where NO axis of the
    group separates.  Strict inequalities: touching is no separation."""
    c = np.stack([256 * ci + 128, 256 * cj + 128, 256 * ck + 128], -1)
    v = t[:, None, :] - c[None]                                # [3 vertices, n, 3]
    box = ~((v.min(0) > 128) | (v.max(0) < -128)).any(-1)
    n = normal(t)
    d = (n * v[0]).sum(-1)
    r = 128 * np.abs(n).sum()
    plane = ~((d > r) | (d < -r))
    edges = np.ones(len(ci), bool)
    for e in range(3):
        u, w = v[e], v[(e + 2) % 3]                            # a vertex of the edge and the opposite vertex
        ex, ey, ez = t[(e + 1) % 3] - t[e]
        for eb, ec, b, cc in ((ey, ez, 1, 2), (ez, ex, 2, 0), (ex, ey, 0, 1)):
            pu, pw = eb * u[:, cc] - ec * u[:, b], eb * w[:, cc] - ec * w[:, b]
            rr = 128 * (abs(eb) + abs(ec))
            edges &= ~((np.minimum(pu, pw) > rr) | (np.maximum(pu, pw) < -rr))
    return box, plane, edges


def voxel_box(t, R):
    lo = np.maximum(0, (t.min(0) - 1) >> 8)
    hi = np.minimum(R - 1, t.max(0) >> 8)
    return lo, hi


def surface_snapped(tri, ok, R, dense=None):
    """snapped triangles -> dict(dense bool [R, R, R], dropped, degenerate)"""
    dense = np.zeros((R, R, R), bool) if dense is None else dense
    dropped = degenerate = 0
    for t, good in zip(tri, ok):
        if not good:
            dropped += 1
            continue
        if not normal(t).any():
            degenerate += 1
            continue
        lo, hi = voxel_box(t, R)
        if (lo > hi).any():
            continue
        ci, cj, ck = (g.ravel() for g in np.meshgrid(*(np.arange(a, b + 1, dtype=np.int64) for a, b in zip(lo, hi)), indexing="ij"))
        box, plane, edges = sat_parts(t, ci, cj, ck)
        hit = box & plane & edges
        dense[ci[hit], cj[hit], ck[hit]] = True
    return {"dense": dense, "dropped": dropped, "degenerate": degenerate}


def surface_ref(vertices, faces, R, bounds=(-1.0, 1.0), dense=None):
    tri, ok = snap_mesh(vertices, faces, bounds[0], bounds[1], R)
    out = surface_snapped(tri, ok, R, dense)
    out["bits"] = pack(out["dense"])
    return out


# ---- solid: int64 restatement -----------------------------------------------------------------------------------------------------
def _edge(p, q, sx, sy):
    return (q[0] - p[0]) * (sy - p[1]) - (q[1] - p[1]) * (sx - p[0])


def _top_left(p, q):
    dx, dy = q[0] - p[0], q[1] - p[1]
    return (dy == 0 and dx > 0) or dy < 0


def _inside(e, tl):
    return (e > 0) | ((e == 0) & bool(tl))


def solid_snapped(tri, ok, R):
    """-> dict(fill bool [R, R, R], parity uint8 [R, R], odd_columns, dropped)"""
    fill = np.zeros((R, R, R), bool)
    parity = np.zeros((R, R), np.uint8)
    dropped = 0
    kc = 256 * np.arange(R, dtype=np.int64) + 128
    for t, good in zip(tri, ok):
        if not good:
            dropped += 1
            continue
        a, b, c = t
        a2 = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if a2 == 0:
            continue
        if a2 < 0:
            b, c, a2 = c, b, -a2
        i0, i1 = max(0, (t[:, 0].min() - 128 + 255) >> 8), min(R - 1, (t[:, 0].max() - 128) >> 8)
        j0, j1 = max(0, (t[:, 1].min() - 128 + 255) >> 8), min(R - 1, (t[:, 1].max() - 128) >> 8)
        if i0 > i1 or j0 > j1:
            continue
        ci, cj = (g.ravel() for g in np.meshgrid(np.arange(i0, i1 + 1, dtype=np.int64), np.arange(j0, j1 + 1, dtype=np.int64), indexing="ij"))
        sx, sy = 256 * ci + 128, 256 * cj + 128
        e0, e1, e2 = _edge(b, c, sx, sy), _edge(c, a, sx, sy), _edge(a, b, sx, sy)
        cov = _inside(e0, _top_left(b, c)) & _inside(e1, _top_left(c, a)) & _inside(e2, _top_left(a, b))
        S = e0 * a[2] + e1 * b[2] + e2 * c[2]
        above = S[cov, None] < kc[None, :] * a2                # voxel centres strictly above the crossing
        fill[ci[cov], cj[cov]] ^= above
        parity[ci[cov], cj[cov]] ^= 1
    return {"fill": fill, "parity": parity, "odd_columns": int(parity.sum()), "dropped": dropped}


def solid_ref(vertices, faces, R, bounds=(-1.0, 1.0), include_surface=True):
    tri, ok = snap_mesh(vertices, faces, bounds[0], bounds[1], R)
    out = solid_snapped(tri, ok, R)
    out["dense"] = out["fill"] | surface_snapped(tri, ok, R)["dense"] if include_surface else out["fill"]
    out["bits"] = pack(out["dense"])
    return out


# ---- points, iou ------------------------------------------------------------------------------------------------------------------
def points_ref(points, R, bounds=(-1.0, 1.0)):
    q, valid = snap(np.asarray(points, F32).reshape(-1, 3), bounds[0], bounds[1], R)
    v = np.where(q == 256 * R, R - 1, q >> 8)
    ok = valid.all(1) & ((v >= 0) & (v < R)).all(1)
    dense = np.zeros((R, R, R), bool)
    dense[v[ok, 0], v[ok, 1], v[ok, 2]] = True
    return {"dense": dense, "bits": pack(dense), "outside": int((~ok).sum())}


def popcount(x):
    x = np.asarray(x, np.uint32)
    return np.unpackbits(x.view(np.uint8)).reshape(x.shape + (32,)).sum(-1).astype(np.int64)


def iou_ref(a, b, paired=False):
    """packed uint32 a[M, R, R, W], b[N, R, R, W] -> (inter int32, union int32, iou float32), [M, N] or, paired, [M]"""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    if not paired:
        a, b = a[:, None], b[None]
    inter = popcount(a & b).sum((-1, -2, -3)).astype(np.int32)
    union = popcount(a | b).sum((-1, -2, -3)).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = np.where(union == 0, F32(1), inter.astype(F32) / union.astype(F32)).astype(F32)
    return inter, union, iou


# ---- second form: Python integers -------------------------------------------------------------------------------------------------
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def hit_big(t, i, j, k):
    """t: three vertices of Python ints.  The 13 axes written out as projections of ALL three vertices on every axis
    (the restatement uses two per edge axis): min > r or max < -r separates."""
    c = (256 * i + 128, 256 * j + 128, 256 * k + 128)
    v = [tuple(int(p[a]) - c[a] for a in range(3)) for p in t]
    e = [tuple(v[(m + 1) % 3][a] - v[m][a] for a in range(3)) for m in range(3)]
    axes = [((1, 0, 0)), ((0, 1, 0)), ((0, 0, 1)), _cross(e[0], e[1])]
    for m in range(3):
        for u in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            axes.append(_cross(u, e[m]))
    for ax in axes:
        p = [sum(ax[a] * w[a] for a in range(3)) for w in v]
        r = 128 * sum(abs(x) for x in ax)
        if min(p) > r or max(p) < -r:
            return False
    return True


def surface_big(tri, ok, R):
    dense = np.zeros((R, R, R), bool)
    for t, good in zip(tri, ok):
        t = [[int(x) for x in p] for p in t]
        n = _cross([t[1][a] - t[0][a] for a in range(3)], [t[2][a] - t[0][a] for a in range(3)])
        if not good or n == (0, 0, 0):
            continue
        lo = [max(0, (min(p[a] for p in t) - 1) >> 8) for a in range(3)]
        hi = [min(R - 1, max(p[a] for p in t) >> 8) for a in range(3)]
        for i in range(lo[0], hi[0] + 1):
            for j in range(lo[1], hi[1] + 1):
                for k in range(lo[2], hi[2] + 1):
                    if hit_big(t, i, j, k):
                        dense[i, j, k] = True
    return dense


def column_big(t, i, j, R):
    """-> None (the column's centre is not covered) or the first k in [0, R] whose centre lies strictly above the crossing, found
    with a floor division (the kernel bisects with the comparison)"""
    a, b, c = ([int(x) for x in p] for p in t)
    a2 = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    if a2 == 0:
        return None
    if a2 < 0:
        b, c, a2 = c, b, -a2
    sx, sy = 256 * i + 128, 256 * j + 128
    es = [_edge(b, c, sx, sy), _edge(c, a, sx, sy), _edge(a, b, sx, sy)]
    tl = [_top_left(b, c), _top_left(c, a), _top_left(a, b)]
    if not all(e > 0 or (e == 0 and f) for e, f in zip(es, tl)):
        return None
    S = es[0] * a[2] + es[1] * b[2] + es[2] * c[2]
    return min(R, max(0, (S - 128 * a2) // (256 * a2) + 1))    # smallest k with (256 k + 128) a2 > S


def solid_big(tri, ok, R):
    fill = np.zeros((R, R, R), bool)
    parity = np.zeros((R, R), np.uint8)
    for t, good in zip(tri, ok):
        if not good:
            continue
        for i in range(R):
            for j in range(R):
                k = column_big(t, i, j, R)
                if k is not None:
                    fill[i, j, k:] ^= True
                    parity[i, j] ^= 1
    return fill, parity


# ---- meshes -----------------------------------------------------------------------------------------------------------------------
def box_mesh(lo, hi):
    """12 triangles of the axis-aligned box [lo, hi] (3-vectors), outward winding"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (n >> a) & 1 else lo)[a] for a in range(3)] for n in range(8)], F32)
    f = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]], np.int32)
    return v, f


def sheet(nx=25, ny=40, seed=0):
    """a wavy 2 * nx * ny = 2 000-triangle sheet across [-0.9, 0.9]^2, heights within +-0.45: sub-voxel to few-voxel triangles"""
    x, y = np.meshgrid(np.linspace(-0.9, 0.9, nx + 1), np.linspace(-0.9, 0.9, ny + 1), indexing="ij")
    z = 0.3 * np.sin(3.1 * x) * np.cos(2.3 * y) + 0.15 * np.random.default_rng(seed).uniform(-1, 1, x.shape)
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(F32)
    n = np.arange((nx + 1) * (ny + 1)).reshape(nx + 1, ny + 1)
    a, b, c, d = n[:-1, :-1].ravel(), n[1:, :-1].ravel(), n[1:, 1:].ravel(), n[:-1, 1:].ravel()
    return v, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)


def octahedron(centre, radius):
    c = np.asarray(centre, np.float64)
    v = np.array([c + radius * np.array(d) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))], F32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def icosphere(subdivisions=3, radius=0.8, centre=(0.03, -0.02, 0.05)):
    """20 * 4^subdivisions triangles (3 -> 1 280), closed and consistently wound"""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(centre) + radius * np.array(v)).astype(F32), np.array(f, np.int32)


# ---- hand-made rule cases: coordinates in voxel units, to be voxelised with bounds (0, R) (then s = 256 and q = 256 x exactly) ----
VOXEL_UNITS = lambda R: (0.0, float(R))      # noqa: E731

# a triangle lying exactly in the plane z = 3 (q_z = 768 = 256 * 3): layers k = 2 and k = 3 are both set
PLANE_TRIANGLE = np.array([[1.25, 1.25, 3.0], [5.5, 1.5, 3.0], [2.5, 5.75, 3.0]], F32)
# one vertex exactly on the voxel corner (4, 4, 4), the rest of the (tiny) triangle inside voxel (4, 4, 4): all 8 voxels around the corner
CORNER_TRIANGLE = np.array([[4.0, 4.0, 4.0], [4.25, 4.125, 4.125], [4.125, 4.25, 4.125]], F32)
# found with slanted_search() below (seed 0), R = 8: voxel SLANTED_CLEAR passes the three box axes and the plane test and is
# separated by an edge x axis test alone, so it must stay clear
SLANTED_TRIANGLE = np.array([[3.5, 2.5, 2.0], [1.0, 1.25, 0.0], [0.25, 0.0, 0.5]], F32)
SLANTED_CLEAR = (0, 0, 1)
# spans the whole grid at any R when voxelised with bounds (0, 1): corners of the cube
SPANNING_TRIANGLE = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.25], [0.0, 1.0, 1.0]], F32)


def slanted_search(seed=0, R=8, tries=2000):
    """how SLANTED_TRIANGLE was found: quarter-voxel coordinates, the first triangle with a voxel that only an edge axis clears"""
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        t = rng.integers(0, 4 * 4 + 1, (3, 3)).astype(np.int64) * 64
        if not normal(t).any():
            continue
        lo, hi = voxel_box(t, R)
        ci, cj, ck = (g.ravel() for g in np.meshgrid(*(np.arange(a, b + 1, dtype=np.int64) for a, b in zip(lo, hi)), indexing="ij"))
        box, plane, edges = sat_parts(t, ci, cj, ck)
        only = box & plane & ~edges
        if only.any():
            n = int(np.argmax(only))
            return (t / 256.0).astype(F32), (int(ci[n]), int(cj[n]), int(ck[n]))
    return None


if __name__ == "__main__":
    print(slanted_search())
