"""numpy restatement of csrc/raycast.hip (the contract of DESIGN.md section 8.8), an independent Moeller-Trumbore ray caster
to hold it against, and the meshes / rays of the ray-casting tests.  No GPU, no torch.

The restatement (``pair``, ``cast``, ``count``): inputs fp32, every operation below is ONE fp64 IEEE rounding, written once and
in this order; the kernel equals it bit for bit.

  ray      ok = every component finite and the direction not (0, 0, 0); a ray that is not ok hits nothing.
           kz = the axis of the largest |d| (the lower axis on a tie), kx = kz + 1, ky = kz + 2 (mod 3), exchanged when d[kz] < 0;
           Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
  vertex   P in {A, B, C}:  Pz = P[kz] - o[kz];  Px = (P[kx] - o[kx]) - Sx Pz;  Py = (P[ky] - o[ky]) - Sy Pz.
  edges    U = Cx By - Cy Bx;  V = Ax Cy - Ay Cx;  W = Bx Ay - By Ax;  det = (U + V) + W.  det == 0: no hit.
           s = the sign of det; the edge values s U, s V, s W must each be > 0, or == 0 on an edge that owns its zero:
           with the edge vectors eU = s (B - C), eV = s (C - A), eW = s (A - B) (x and y of the sheared vertices: the triangle
           runs counter-clockwise along them), an edge owns its zero when e.y < 0, or e.y == 0 and e.x < 0 (top-left rule).
  t        T = (U Az + V Bz) + W Cz;  t = float32((Sz T) / det), and -0 counts as +0.  A hit needs tmin <= t < tmax.
  winner   of ``cast``: the smallest (bits of t, triangle index).
  finish   for the winner: uv = float32(V / det), float32(W / det);  n = (B - A) x (C - A) in fp64 of the fp32 vertices (each
           component p q - r s), nn = (nx nx + ny ny) + nz nz, normal = float32(n / sqrt(nn)), zero where nn is 0 or not finite.
  miss     t = +inf, tri = -1, uv = normal = 0, count = 0.
"""
from __future__ import annotations

import numpy as np

F64 = np.float64
MISS_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
class _Rays:
    def __init__(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        o, d = rays[:, :3].astype(F64), rays[:, 3:].astype(F64)
        self.ok = np.isfinite(rays).all(1) & (rays[:, 3:] != 0).any(1)
        d = np.where(self.ok[:, None], d, np.array([0.0, 0.0, 1.0]))
        o = np.where(self.ok[:, None], o, 0.0)
        i = np.arange(len(rays))
        kz = np.argmax(np.abs(d), axis=1)                      # the first maximum: the lower axis on a tie
        kx, ky = (kz + 1) % 3, (kz + 2) % 3
        dz = d[i, kz]
        swap = dz < 0
        kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
        self.kx, self.ky, self.kz = kx, ky, kz
        self.ox, self.oy, self.oz = o[i, kx][:, None], o[i, ky][:, None], o[i, kz][:, None]
        self.Sx, self.Sy, self.Sz = (d[i, kx] / dz)[:, None], (d[i, ky] / dz)[:, None], (1.0 / dz)[:, None]

    def part(self, a, b):
        r = object.__new__(_Rays)
        for k, v in self.__dict__.items():
            setattr(r, k, v[a:b])
        return r


def _shear(r: _Rays, P):
    """P [F, 3] fp64 -> the sheared x, y and the unscaled z of every (ray, vertex) pair, [R, F] each"""
    PT = P.T
    z = PT[r.kz] - r.oz
    x = (PT[r.kx] - r.ox) - r.Sx * z
    y = (PT[r.ky] - r.oy) - r.Sy * z
    return x, y, z


def _owns(s, ex, ey):
    ex, ey = s * ex, s * ey
    return (ey < 0) | ((ey == 0) & (ex < 0))


def _pair_block(r: _Rays, A, B, C, tmin, tmax):
    """-> hit [R, F] bool, t [R, F] float32, and (V, W, det) for the finish"""
    Ax, Ay, Az = _shear(r, A)
    Bx, By, Bz = _shear(r, B)
    Cx, Cy, Cz = _shear(r, C)
    U = Cx * By - Cy * Bx
    V = Ax * Cy - Ay * Cx
    W = Bx * Ay - By * Ax
    det = (U + V) + W
    s = np.where(det > 0, 1.0, -1.0)
    nU, nV, nW = s * U, s * V, s * W
    inside = ((nU > 0) | ((nU == 0) & _owns(s, Bx - Cx, By - Cy))) \
        & ((nV > 0) | ((nV == 0) & _owns(s, Cx - Ax, Cy - Ay))) \
        & ((nW > 0) | ((nW == 0) & _owns(s, Ax - Bx, Ay - By)))
    T = (U * Az + V * Bz) + W * Cz
    with np.errstate(all="ignore"):
        t = ((r.Sz * T) / det).astype(np.float32)
    t = t + np.float32(0.0)                                        # -0 -> +0
    hit = inside & (det != 0) & (t >= np.float32(tmin)) & (t < np.float32(tmax)) & r.ok[:, None]
    return hit, t, V, W, det


def _corners(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float32)
    f = np.asarray(triangles).astype(np.int64)
    return v[f[:, 0]].astype(F64), v[f[:, 1]].astype(F64), v[f[:, 2]].astype(F64)


def _blocks(R, F, budget=1_500_000):
    step = max(1, budget // max(F, 1))
    return [(a, min(R, a + step)) for a in range(0, R, step)]


def pair(vertices, triangles, rays, tmin=0.0, tmax=np.inf):
    """every (ray, triangle) pair: hit [R, F] bool and t [R, F] float32 (small cases only)"""
    A, B, C = _corners(vertices, triangles)
    hit, t, _, _, _ = _pair_block(_Rays(rays), A, B, C, tmin, tmax)
    return hit, t


def count(vertices, triangles, rays, tmin=0.0, tmax=np.inf):
    A, B, C = _corners(vertices, triangles)
    r = _Rays(rays)
    out = np.zeros(len(r.ok), dtype=np.int32)
    for a, b in _blocks(len(out), len(A)):
        out[a:b] = _pair_block(r.part(a, b), A, B, C, tmin, tmax)[0].sum(1)
    return out


def cast(vertices, triangles, rays, tmin=0.0, tmax=np.inf):
    """-> dict(t [R] float32, tri [R] int32, uv [R, 2] float32, normal [R, 3] float32, count [R] int32: what ``count`` gives)"""
    A, B, C = _corners(vertices, triangles)
    r = _Rays(rays)
    R, F = len(r.ok), len(A)
    t_out = np.full(R, np.inf, dtype=np.float32)
    tri = np.full(R, -1, dtype=np.int32)
    uv = np.zeros((R, 2), dtype=np.float32)
    cnt = np.zeros(R, dtype=np.int32)
    fidx = np.arange(F, dtype=np.uint64)[None, :]
    for a, b in _blocks(R, F):
        hit, t, V, W, det = _pair_block(r.part(a, b), A, B, C, tmin, tmax)
        cnt[a:b] = hit.sum(1)
        key = np.where(hit, (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | fidx, MISS_KEY)
        w = key.argmin(1)
        rows = np.arange(b - a)
        got = key[rows, w] != MISS_KEY
        t_out[a:b] = np.where(got, t[rows, w], np.float32(np.inf))
        tri[a:b] = np.where(got, w, -1)
        with np.errstate(all="ignore"):
            uv[a:b, 0] = np.where(got, (V[rows, w] / det[rows, w]).astype(np.float32), 0)
            uv[a:b, 1] = np.where(got, (W[rows, w] / det[rows, w]).astype(np.float32), 0)
    return dict(t=t_out, tri=tri, uv=uv, normal=face_normals(vertices, triangles, tri), count=cnt)


def face_normals(vertices, triangles, tri):
    """the finish kernel's normal of triangle tri[i] (zeros where tri is -1)"""
    A, B, C = _corners(vertices, triangles)
    k = np.maximum(tri, 0)
    e1, e2 = B[k] - A[k], C[k] - A[k]
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                  e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    good = (nn > 0) & np.isfinite(nn) & (tri >= 0)
    with np.errstate(all="ignore"):
        out = (n / np.sqrt(np.where(good, nn, 1.0))[:, None]).astype(np.float32)
    return np.where(good[:, None], out, np.float32(0))


# ---- an independent caster: Moeller-Trumbore in fp64, nothing shared with the code above ---------------------------------------
def mt_cast(vertices, triangles, rays, tmin=0.0, tmax=np.inf, edge=1e-9):
    """-> dict(t [R] fp64 nearest hit or inf, tri [R], t2 [R] second nearest hit or inf, count [R],
    near_edge [R] bool: some triangle is met within ``edge`` (in barycentric units) of its boundary)"""
    v = np.asarray(vertices, dtype=F64)
    f = np.asarray(triangles).astype(np.int64)
    rays = np.asarray(rays, dtype=F64)
    a = v[f[:, 0]]
    e1, e2 = v[f[:, 1]] - a, v[f[:, 2]] - a
    R = len(rays)
    out = dict(t=np.full(R, np.inf), tri=np.full(R, -1, dtype=np.int64), t2=np.full(R, np.inf), count=np.zeros(R, dtype=np.int64),
               near_edge=np.zeros(R, dtype=bool))
    for lo, hi in _blocks(R, len(f), 600_000):
        o, d = rays[lo:hi, None, :3], rays[lo:hi, None, 3:]
        p = np.cross(d, e2[None])
        det = (e1[None] * p).sum(-1)
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = o - a[None]
            bu = (tv * p).sum(-1) * inv
            q = np.cross(tv, e1[None])
            bv = (d * q).sum(-1) * inv
            t = (e2[None] * q).sum(-1) * inv
        bw = 1.0 - bu - bv
        low = np.minimum(np.minimum(bu, bv), bw)
        ranged = (t >= tmin) & (t < tmax) & (det != 0)
        hit = ranged & (low > 0)
        out["near_edge"][lo:hi] = (ranged & (np.abs(low) <= edge)).any(1)
        th = np.where(hit, t, np.inf)
        order = np.argsort(th, axis=1)[:, :2]
        rows = np.arange(hi - lo)
        out["t"][lo:hi] = th[rows, order[:, 0]]
        out["tri"][lo:hi] = np.where(np.isfinite(th[rows, order[:, 0]]), order[:, 0], -1)
        if th.shape[1] > 1:
            out["t2"][lo:hi] = th[rows, order[:, 1]]
        out["count"][lo:hi] = hit.sum(1)
    return out


# ---- meshes -------------------------------------------------------------------------------------------------------------------
def icosphere(subdivisions=3, radius=0.75):
    """closed, convex: 20 * 4^subdivisions triangles, outward counter-clockwise"""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=F64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, dtype=np.int64)


TORUS_R, TORUS_r = 0.55, 0.2


def torus(nu=48, nv=24, R=TORUS_R, r=TORUS_r):
    """closed, not convex, around the z axis: 2 nu nv triangles, outward counter-clockwise"""
    u = np.arange(nu) * (2 * np.pi / nu)
    w = np.arange(nv) * (2 * np.pi / nv)
    uu, ww = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(ww)) * np.cos(uu), (R + r * np.cos(ww)) * np.sin(uu), r * np.sin(ww)], -1).reshape(-1, 3)
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [(a, b, c), (a, c, d)]
    return v.astype(np.float32), np.array(f, dtype=np.int64)


def torus_implicit(p, R=TORUS_R, r=TORUS_r):
    """the signed distance to the analytic torus (negative inside)"""
    p = np.asarray(p, dtype=F64)
    return np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - R) ** 2 + p[:, 2] ** 2) - r


def torus_chord_error(nu=48, nv=24, R=TORUS_R, r=TORUS_r):
    """how far the mesh can lie from the analytic surface: the sagitta of the longest chord in each direction, added"""
    return (R + r) * (1 - np.cos(np.pi / nu)) + r * (1 - np.cos(np.pi / nv))


def cube():
    """the 12 triangles of [-1/2, 1/2]^3, outward counter-clockwise; every face is split along the diagonal from its
    (-, -) to its (+, +) corner in the face's own two axes"""
    v = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], dtype=np.float32)   # index = x + 2 y + 4 z
    f = np.array([(0, 2, 3), (0, 3, 1),     # z = -1/2
                  (4, 5, 7), (4, 7, 6),     # z = +1/2
                  (0, 1, 5), (0, 5, 4),     # y = -1/2
                  (2, 6, 7), (2, 7, 3),     # y = +1/2
                  (0, 4, 6), (0, 6, 2),     # x = -1/2
                  (1, 3, 7), (1, 7, 5)],    # x = +1/2
                 dtype=np.int64)
    return v, f


def cube_flipped():
    """the cube with the winding of every second triangle reversed"""
    v, f = cube()
    f = f.copy()
    f[::2] = f[::2][:, [0, 2, 1]]
    return v, f


def octahedron():
    v = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=np.float32)
    f = np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], dtype=np.int64)
    return v, f


def wavy_sheet(n=24):
    """open: z = 0.1 sin(3 x) cos(2 y) over [-0.8, 0.8]^2, 2 (n - 1)^2 triangles"""
    g = np.linspace(-0.8, 0.8, n)
    x, y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([x, y, 0.1 * np.sin(3 * x) * np.cos(2 * y)], -1).reshape(-1, 3)
    f = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
            f += [(a, b, c), (a, c, d)]
    return v.astype(np.float32), np.array(f, dtype=np.int64)


def spliced_sheet(n=12, seed=5):
    """the wavy sheet with triangles without area (a repeated vertex, three vertices in a line) and needles (one edge 1e-6 of
    the others) spliced in between its own, in random positions"""
    v, f = wavy_sheet(n)
    rng = np.random.default_rng(seed)
    extra_v, extra_f = [], []
    base = len(v)
    for k in range(40):
        a, b = rng.integers(0, base, 2)
        kind = k % 4
        if kind == 0:
            extra_f.append((a, a, b))                                       # a repeated vertex
        elif kind == 1:
            extra_v.append(0.5 * (v[a].astype(F64) + v[b].astype(F64)))     # (nearly) in a line with a and b
            extra_f.append((a, base + len(extra_v) - 1, b))
        elif kind == 2:
            extra_v.append(v[a].astype(F64) + np.array([1e-6, 0, 0]))       # a needle
            extra_f.append((a, base + len(extra_v) - 1, b))
        else:
            extra_f.append((a, b, b))
    v = np.concatenate([v, np.array(extra_v, dtype=np.float32)])
    f = np.concatenate([f, np.array(extra_f, dtype=np.int64)])
    return v, f[rng.permutation(len(f))]


def first_faces(mesh, F):
    v, f = mesh
    return v, f[:F]


MESHES = {"icosphere": icosphere, "torus": torus, "cube": cube, "octahedron": octahedron, "wavy_sheet": wavy_sheet,
          "spliced_sheet": spliced_sheet, "cube_flipped": cube_flipped}


# ---- rays ---------------------------------------------------------------------------------------------------------------------
def random_rays(R, seed, extent=1.0):
    """origins uniform in [-extent, extent]^3, directions isotropic with lengths in [0.5, 2)"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-extent, extent, (R, 3))
    d = rng.normal(size=(R, 3))
    d *= (rng.uniform(0.5, 2.0, (R, 1)) / np.linalg.norm(d, axis=1, keepdims=True))
    return np.concatenate([o, d], 1).astype(np.float32)


def axis_rays(R, seed, extent=1.0):
    """origins as above, directions +-x, +-y, +-z in turn"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-extent, extent, (R, 3))
    d = np.zeros((R, 3))
    k = np.arange(R)
    d[k, k % 3] = np.where((k // 3) % 2 == 0, 1.0, -1.0)
    return np.concatenate([o, d], 1).astype(np.float32)


def cube_lattice(z0):
    """+z rays from z = z0 at every (x, y) of the 1/8 lattice of [-3/4, 3/4]^2"""
    g = np.arange(-6, 7) / 8.0
    x, y = np.meshgrid(g, g, indexing="ij")
    n = x.size
    rays = np.zeros((n, 6), dtype=np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 5] = x.ravel(), y.ravel(), z0, 1.0
    return rays


def octahedron_rays(outside=True):
    """axis-parallel rays through the octahedron's vertices and edge midpoints: from outside (started 2 behind the target
    along the direction) or from the centre (only those whose line passes through the centre, i.e. the vertices)"""
    v, f = octahedron()
    targets = [p for p in v.astype(F64)]
    edges = {tuple(sorted((int(a), int(b)))) for t in f for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
    targets += [0.5 * (v[a].astype(F64) + v[b].astype(F64)) for a, b in sorted(edges)]
    rays = []
    for p in targets:
        for axis in range(3):
            for sgn in (1.0, -1.0):
                d = np.zeros(3)
                d[axis] = sgn
                if outside:
                    rays.append(np.concatenate([p - 2 * d, d]))
                elif np.count_nonzero(p) == 1 and p[axis] != 0:
                    rays.append(np.concatenate([np.zeros(3), d]))
    return np.array(rays, dtype=np.float32)


def aimed_rays(mesh, R, seed, extent=1.0):
    """origins as in random_rays, each ray aimed at a random point of a random triangle of the mesh (so that a small mesh is
    hit often), the target at t between 0.5 and 2"""
    v, f = mesh
    rng = np.random.default_rng(seed)
    o = rng.uniform(-extent, extent, (R, 3))
    k = rng.integers(0, len(f), R)
    w = rng.dirichlet(np.ones(3), R)
    p = (v[f[k]].astype(F64) * w[:, :, None]).sum(1)
    d = (p - o) / rng.uniform(0.5, 2.0, (R, 1))
    return np.concatenate([o, d], 1).astype(np.float32)


def mixed_rays(mesh, R, seed):
    """a third each of random, axis-parallel and aimed rays, interleaved"""
    parts = [random_rays(R, seed), axis_rays(R, seed + 1), aimed_rays(mesh, R, seed + 2)]
    k = np.arange(R)
    return np.stack(parts)[k % 3, k]
