"""The yardstick of the mesh-distance tests (surfd_amd/meshprep.py, csrc/meshdist.hip): mathematics in fp64, small procedural
meshes, and a numpy restatement of the kernel's formulas at fp32 (deterministic; shared by the tests and tools).

  closest_fp64             brute force over all triangles; per triangle the minimum over the projection onto its plane (where
                           that falls inside) and its three edge SEGMENTS.  A different formulation from the kernel's region
                           classification on purpose, and right for degenerate triangles by construction (a zero-area triangle
                           is the union of its edges).
  point_triangle_fp64      the same for pairs (point i, triangle i)
  kernel_formulas_fp32     md_pair / md_prepare_kernel of csrc/meshdist.hip restated in numpy with every operation rounded to
                           fp32 (fmaf through an exact fp64 product): what fp32 costs these formulas against fp64, measured
                           without running the code under test.  It is the source of the tests' distance tolerance.
"""
import numpy as np

F32_MIN = np.float32(np.finfo(np.float32).tiny)
F32_MAX = np.float32(np.finfo(np.float32).max)


# ---- fp64 oracle ------------------------------------------------------------------------------------------------------------
def _segment(p, a, b):
    """closest point of the segment a-b to p (all [..., 3], fp64); a == b gives a"""
    ab = b - a
    den = (ab * ab).sum(-1)
    t = np.where(den > 0, ((p - a) * ab).sum(-1) / np.where(den > 0, den, 1.0), 0.0)
    return a + np.clip(t, 0.0, 1.0)[..., None] * ab


def _triangle(p, a, b, c):
    """closest point of the triangle a-b-c to p and its distance (broadcasting [..., 3], fp64)"""
    best, bd = None, None
    for s0, s1 in ((a, b), (b, c), (c, a)):
        x = _segment(p, s0, s1)
        d = ((p - x) ** 2).sum(-1)
        if best is None:
            best, bd = x, d
        else:
            m = d < bd
            best, bd = np.where(m[..., None], x, best), np.where(m, d, bd)
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    ok = nn > 0
    nn1 = np.where(ok, nn, 1.0)
    x = p - n * (((p - a) * n).sum(-1) / nn1)[..., None]
    # inside: the projection is on the inner side of every edge
    inside = ok
    for s0, s1 in ((a, b), (b, c), (c, a)):
        inside = inside & ((np.cross(s1 - s0, x - s0) * n).sum(-1) >= 0)
    d = ((p - x) ** 2).sum(-1)
    m = inside & (d < bd)
    best, bd = np.where(m[..., None], x, best), np.where(m, d, bd)
    return best, np.sqrt(bd)


def closest_fp64(vertices, triangles, queries, chunk=512):
    """-> (dist [Q], point [Q, 3], tri [Q]) in fp64 (tri: the first triangle at the minimum)"""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64)
    q = np.asarray(queries, np.float64)
    a, b, c = v[t[:, 0]][None], v[t[:, 1]][None], v[t[:, 2]][None]
    dist, point, tri = np.empty(len(q)), np.empty((len(q), 3)), np.empty(len(q), np.int64)
    for i in range(0, len(q), chunk):
        x, d = _triangle(q[i:i + chunk, None], a, b, c)
        j = d.argmin(1)
        r = np.arange(len(j))
        dist[i:i + chunk], point[i:i + chunk], tri[i:i + chunk] = d[r, j], x[r, j], j
    return dist, point, tri


def point_triangle_fp64(vertices, triangles, tri, points):
    """distance of points[i] to triangle tri[i], fp64"""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64)[np.asarray(tri, np.int64)]
    return _triangle(np.asarray(points, np.float64), v[t[:, 0]], v[t[:, 1]], v[t[:, 2]])[1]


# ---- the kernel's formulas at fp32 ------------------------------------------------------------------------------------------
def _f(x):
    return np.asarray(x, np.float32)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _dot(ax, ay, az, bx, by, bz):
    return _fma(az, bz, _fma(ay, by, ax * bx))


def _inv(x):
    ok = (x >= F32_MIN) & (x <= F32_MAX)
    return np.where(ok, np.float32(1) / np.where(ok, x, np.float32(1)), np.float32(0)).astype(np.float32)


def _clamp01(x):
    return np.minimum(np.maximum(x, np.float32(0)), np.float32(1))


def kernel_records_fp32(vertices, triangles):
    """md_prepare_kernel: dict of per-triangle fp32 arrays (edges and inverses in fp32; unit normal and in-plane edge normals
    from the fp64 cross product, rounded once)"""
    v = _f(vertices)
    t = np.asarray(triangles, np.int64)
    p0, p1, p2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    ab, ac, bc = p1 - p0, p2 - p0, p2 - p1
    sq = lambda e: _dot(e[:, 0], e[:, 1], e[:, 2], e[:, 0], e[:, 1], e[:, 2])
    E1, E2, E3 = p1.astype(np.float64) - p0, p2.astype(np.float64) - p0, p2.astype(np.float64) - p1
    n = np.cross(E1, E2)
    nn = (n * n).sum(1)
    area = (nn >= 1e-290) & (nn <= 1e290)
    n = n * np.where(area, 1.0 / np.sqrt(np.where(area, nn, 1.0)), 0.0)[:, None]
    return dict(a=p0, ab=_f(ab), ac=_f(ac), bc=_f(bc), iab=_inv(sq(ab)), ibc=_inv(sq(bc)), iac=_inv(sq(ac)), n=_f(n),
                mab=_f(np.cross(n, E1)), mbc=_f(np.cross(n, E3)), mca=_f(np.cross(n, -E2)), degenerate=~area)


def _segment_fp32(r, e, inv, sgn):
    t = _clamp01(np.float32(sgn) * _dot(e[..., 0], e[..., 1], e[..., 2], r[..., 0], r[..., 1], r[..., 2]) * inv)
    u = np.float32(-sgn) * t
    d = np.stack([_fma(u, e[..., k] + 0 * u, r[..., k]) for k in range(3)], -1)
    return _dot(d[..., 0], d[..., 1], d[..., 2], d[..., 0], d[..., 1], d[..., 2]), d


def _pair_fp32(R, q):
    """md_pair for q [Q, 1, 3] against every record [1, F, ...]: squared distance [Q, F] and q - closest point [Q, F, 3]"""
    ra = q - R["a"][None]
    rb = ra - R["ab"][None]
    rc = ra - R["ac"][None]
    d1, x1 = _segment_fp32(ra, R["ab"][None], R["iab"][None], 1)
    d2, x2 = _segment_fp32(rb, R["bc"][None], R["ibc"][None], 1)
    d3, x3 = _segment_fp32(rc, R["ac"][None], R["iac"][None], -1)
    dot3 = lambda m, r: _dot(m[..., 0] + 0 * r[..., 0], m[..., 1] + 0 * r[..., 0], m[..., 2] + 0 * r[..., 0], r[..., 0], r[..., 1], r[..., 2])
    n = R["n"][None]
    h = dot3(n, ra)
    inside = np.minimum(dot3(R["mab"][None], ra), np.minimum(dot3(R["mbc"][None], rb), dot3(R["mca"][None], rc))) > 0
    de = np.minimum(d1, np.minimum(d2, d3))
    dp = np.where(inside, h * h, np.float32(np.inf)).astype(np.float32)
    dd = np.minimum(de, dp)
    d = np.where((dp == dd)[..., None], h[..., None] * n, np.where((d1 == dd)[..., None], x1, np.where((d2 == dd)[..., None], x2, x3)))
    return dd, _f(d)


def kernel_formulas_fp32(vertices, triangles, queries, chunk=512):
    """-> (dist [Q] fp32, closest [Q, 3] fp32, tri [Q]): minimum under (squared distance, index), sqrt, q - difference"""
    R = kernel_records_fp32(vertices, triangles)
    q = _f(queries)
    dist, point, tri = np.empty(len(q), np.float32), np.empty((len(q), 3), np.float32), np.empty(len(q), np.int64)
    with np.errstate(all="ignore"):
        for i in range(0, len(q), chunk):
            qq = q[i:i + chunk]
            dd, d = _pair_fp32(R, qq[:, None])
            j = dd.argmin(1)                                   # the first index at the minimum
            r = np.arange(len(j))
            dist[i:i + chunk] = np.sqrt(dd[r, j])
            point[i:i + chunk] = qq - d[r, j]
            tri[i:i + chunk] = j
    return dist, point, tri


# ---- procedural meshes ------------------------------------------------------------------------------------------------------
def _grid_triangles(n, m):
    idx = np.arange(n * m).reshape(n, m)
    lo = np.stack([idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:]], -1).reshape(-1, 3)
    hi = np.stack([idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]], -1).reshape(-1, 3)
    return np.concatenate([lo, hi]).astype(np.int64)


def wavy_sheet(n=40):
    """an open surface: z = 0.2 sin(4x) cos(3y) over [-0.8, 0.8]^2, 2 (n - 1)^2 triangles"""
    u, w = np.meshgrid(np.linspace(-0.8, 0.8, n), np.linspace(-0.8, 0.8, n), indexing="ij")
    v = np.stack([u, w, 0.2 * np.sin(4 * u) * np.cos(3 * w)], -1).reshape(-1, 3).astype(np.float32)
    return v, _grid_triangles(n, n)


def _icosahedron():
    g = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
                  [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    return v / np.linalg.norm(v[0]), f


def convex_polyhedron(levels=4, scale=(0.7, 0.55, 0.6)):
    """a closed convex polyhedron: an icosahedron stretched per axis, every face subdivided IN ITS PLANE `levels` times
    (20 * 4^levels triangles, outward orientation).  Returns (vertices fp32, triangles, face [F]: the flat face a triangle is in)."""
    v, f = _icosahedron()
    v = v * np.asarray(scale)
    tris = v[f]                                                 # [20, 3, 3]
    face = np.arange(20)
    for _ in range(levels):
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
        tris = np.concatenate([np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, bc, c], 1), np.stack([ab, bc, ca], 1)])
        face = np.concatenate([face] * 4)
    pts = tris.reshape(-1, 3).astype(np.float32)
    uniq, inv = np.unique(pts, axis=0, return_inverse=True)
    return uniq, inv.reshape(-1, 3).astype(np.int64), face


def spliced_sheet(n=40, seed=5):
    """the wavy sheet with duplicated, zero-area and needle triangles spliced in at random places of the triangle list"""
    v, t = wavy_sheet(n)
    g = np.random.default_rng(seed)
    extra_v, extra_t = [], []
    nv = len(v)

    def add(tri_pts):
        nonlocal nv
        extra_v.append(np.asarray(tri_pts, np.float32))
        extra_t.append([nv, nv + 1, nv + 2])
        nv += 3

    dup = t[g.integers(0, len(t), 40)]                          # exact duplicates (reuse the sheet's vertices)
    for _ in range(30):                                         # two coincident vertices: a segment
        p, d = g.uniform(-0.9, 0.9, 3), g.normal(0, 0.05, 3)
        add([p, p + d, p] if _ % 2 else [p, p, p + d])
    for _ in range(10):                                         # three coincident vertices: a point
        p = g.uniform(-0.9, 0.9, 3)
        add([p, p, p])
    for _ in range(30):                                         # three distinct collinear vertices
        p, d = g.uniform(-0.9, 0.9, 3), g.normal(0, 0.05, 3)
        s = g.uniform(0.1, 0.9)
        add([[p, p + np.float32(s) * d, p + d], [p + d, p, p + np.float32(s) * d], [p, p + d, p + np.float32(s) * d]][_ % 3])
    for _ in range(60):                                         # needles: aspect 1e2 .. 1e4
        p, d = g.uniform(-0.9, 0.9, 3), g.normal(0, 0.08, 3)
        o = np.cross(d, g.normal(0, 1, 3))
        o = o / np.linalg.norm(o) * np.linalg.norm(d) * 10.0 ** g.uniform(-4, -2)
        add([[p, p + d, p + 0.5 * d + o], [p, p + o, p + d], [p + d, p, p + o]][_ % 3])
    v2 = np.concatenate([v] + extra_v).astype(np.float32)
    t2 = np.concatenate([t, dup, np.asarray(extra_t, np.int64)])
    return v2, t2[g.permutation(len(t2))]


def needle_mesh(seed=13, count=400):
    """long needle triangles alone: edges of normal(0, 0.3) per axis, aspect (height over length) log-uniform over
    2^-20 .. 10^-2, in the three vertex layouts of spliced_sheet (apex over the middle, short edge at either end)"""
    g = np.random.default_rng(seed)
    vs, ts = [], []
    for i in range(count):
        p, d = g.uniform(-0.6, 0.6, 3), g.normal(0, 0.3, 3)
        o = np.cross(d, g.normal(0, 1, 3))
        o = o / np.linalg.norm(o) * np.linalg.norm(d) * 2.0 ** g.uniform(-20, np.log2(1e-2))
        vs.append(np.asarray([[p, p + d, p + 0.5 * d + o], [p, p + o, p + d], [p + d, p, p + o]][i % 3], np.float32))
        ts.append([3 * i, 3 * i + 1, 3 * i + 2])
    return np.concatenate(vs).astype(np.float32), np.asarray(ts, np.int64)


def zero_area_mesh(seed=9, count=200):
    """only zero-area triangles: segments (two coincident vertices), collinear triples and points"""
    g = np.random.default_rng(seed)
    vs, ts = [], []
    for i in range(count):
        p, d = g.uniform(-0.8, 0.8, 3).astype(np.float32), g.normal(0, 0.1, 3).astype(np.float32)
        kind = i % 4
        if kind == 0:
            tri = [p, p + d, p + d]
        elif kind == 1:
            tri = [p + d, p, p + d]
        elif kind == 2:
            tri = [p, p + np.float32(2) * d, p + d]             # collinear up to the rounding of the sums, b beyond c
        else:
            tri = [p, p, p]
        vs.append(np.asarray(tri, np.float32))
        ts.append([3 * i, 3 * i + 1, 3 * i + 2])
    return np.concatenate(vs).astype(np.float32), np.asarray(ts, np.int64)


def area_ladder(seed=3, count=64):
    """disjoint triangles whose areas span two orders of magnitude (for the sampler's area weights)"""
    g = np.random.default_rng(seed)
    vs, ts = [], []
    for i in range(count):
        size = 0.02 * 10.0 ** (i / (count - 1))                 # edge 0.02 .. 0.2: area x 100
        p = g.uniform(-0.7, 0.7, 3)
        e1, e2 = g.normal(0, 1, 3), g.normal(0, 1, 3)
        e1 /= np.linalg.norm(e1)
        e2 -= e1 * (e1 @ e2)
        e2 /= np.linalg.norm(e2)
        vs.append(np.stack([p, p + size * e1, p + size * e2]))
        ts.append([3 * i, 3 * i + 1, 3 * i + 2])
    return np.concatenate(vs).astype(np.float32), np.asarray(ts, np.int64)


def triangle_areas_fp64(vertices, triangles):
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64)
    return 0.5 * np.linalg.norm(np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]), axis=1)


def write_obj(path, vertices, triangles):
    with open(path, "w") as f:
        for p in np.asarray(vertices, np.float64):
            f.write(f"v {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n")
        for t in np.asarray(triangles):
            f.write(f"f {t[0] + 1} {t[1] + 1} {t[2] + 1}\n")


# ---- the tests' queries and the measured tolerance --------------------------------------------------------------------------
QUERY_STDS = [0.003, 0.01, 0.1]


def pipeline_queries(vertices, triangles, seed, per_sigma=6000, uniform=2000, cloud=3000):
    """queries made the way the pipeline makes them, on the CPU (so that they are the same on every machine): a surface cloud
    from sample_points_uniformly, sample_points_around_pcd at the reference's three sigmas, and uniform points.  fp32 [N, 3]"""
    import torch
    from surfd_amd.meshprep import sample_points_around_pcd, sample_points_uniformly
    g = torch.Generator().manual_seed(seed)
    pcd = sample_points_uniformly(torch.from_numpy(np.asarray(vertices, np.float32)), torch.from_numpy(np.asarray(triangles, np.int64)), cloud, generator=g)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    q = sample_points_around_pcd(pcd, QUERY_STDS, [per_sigma] * 3 + [uniform], (-1.0, 1.0), "cpu")
    torch.random.set_rng_state(state)
    return q.numpy().astype(np.float32)


def test_queries(name, v, t, seed):
    """the queries of a test mesh: pipeline-made; for the needle mesh half of them are uniform in [-1, 1]^3 (far queries are
    where thin triangles are hardest)"""
    if name == "needles":
        return pipeline_queries(v, t, seed, per_sigma=3400, uniform=10000)
    return pipeline_queries(v, t, seed)


def test_meshes():
    """name -> (vertices, triangles, query seed): the meshes of the distance tests"""
    pv, pt, _ = convex_polyhedron()
    return {"wavy_sheet": (*wavy_sheet(), 101), "convex_polyhedron": (pv, pt, 102), "spliced_sheet": (*spliced_sheet(), 103),
            "zero_area": (*zero_area_mesh(), 104), "needles": (*needle_mesh(), 106)}


def measure_fp32_restatement():
    """largest |dist32 - dist64| of kernel_formulas_fp32 against closest_fp64 on the tests' own meshes and queries"""
    worst = {}
    for name, (v, t, seed) in test_meshes().items():
        q = test_queries(name, v, t, seed)
        d64 = closest_fp64(v, t, q)[0]
        d32 = kernel_formulas_fp32(v, t, q)[0]
        worst[name] = float(np.abs(d32.astype(np.float64) - d64).max())
        print(f"{name}: {len(t)} triangles, {len(q)} queries, max |dist32 - dist64| = {worst[name]:.3e}", flush=True)
    print(f"largest: {max(worst.values()):.3e}")
    return worst


if __name__ == "__main__":
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure_fp32_restatement()
