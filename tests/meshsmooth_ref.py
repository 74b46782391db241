"""Sequential numpy restatement of the contract of csrc/meshsmooth.hip: Laplacian smoothing, the umbrella
operator over all half-edges and over the border polyline, Taubin smoothing and vertex normals, with the ARITHMETIC WRITTEN OUT:

    dot(a, b)   = (a0 b0 + a1 b1) + a2 b2
    cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)
    norm(a)     = sqrt((a0 a0 + a1 a1) + a2 a2)

No einsum, no np.linalg.norm, no np.cross: np.einsum("ij,ij->i") differs from the dot above in the last bit on a good part of
random rows, which is why meshproc.laplacian_smooth itself cannot be the bit oracle of the device.  Sums per vertex run in the
order np.add.at applies its operands (one after the other, in index order): first every half-edge that leaves the vertex,
ascending, then every half-edge that arrives.  Everything is fp64; fp32 positions are converted first.

Also here: the meshes the tests share (small ones by hand, sheets, icospheres).
"""
import numpy as np


# ---- arithmetic -------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def cross3(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def norm3(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def _mesh(vertices, faces):
    return np.array(vertices, dtype=np.float64, copy=True).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)


# ---- connectivity -----------------------------------------------------------------------------------------------------------
def halfedges(faces):
    """(origin, destination, opposite) of half-edge h = 3 f + c, each [3 F]"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return faces.reshape(-1), faces[:, [1, 2, 0]].reshape(-1), faces[:, [2, 0, 1]].reshape(-1)


def border_halfedges(faces):
    """bool [3 F]: the half-edge's unordered vertex pair occurs exactly once among all half-edges (faces with repeated indices
    take part)"""
    v0, v1, _ = halfedges(faces)
    if len(v0) == 0:
        return np.zeros(0, dtype=bool)
    lo, hi = np.minimum(v0, v1), np.maximum(v0, v1)
    _, inverse, counts = np.unique(np.stack([hi, lo], axis=1), axis=0, return_inverse=True, return_counts=True)
    return counts[inverse.reshape(-1)] == 1


def border_records(faces):
    """(src, dst): per border edge (lo, hi), the edges ascending in (hi, lo): first every lo -> hi, then every hi -> lo.  Applied
    in this order, a vertex meets its border neighbours above it ascending, then those below it ascending."""
    v0, v1, _ = halfedges(faces)
    b = border_halfedges(faces)
    lo, hi = np.minimum(v0, v1)[b], np.maximum(v0, v1)[b]
    order = np.lexsort((lo, hi))
    lo, hi = lo[order], hi[order]
    return np.concatenate([lo, hi]), np.concatenate([hi, lo])


def counts(faces):
    """(border half-edges, border vertices)"""
    src, _ = border_records(faces)
    return len(src) // 2, len(np.unique(src))


# ---- sweeps -----------------------------------------------------------------------------------------------------------------
def cot_weights(p, v0, v1, v2):
    a, b = p[v1] - p[v2], p[v0] - p[v2]
    cr = norm3(cross3(a, b))
    d = dot3(a, b)
    w = np.zeros(len(v0))
    ok = cr > 0
    w[ok] = d[ok] / cr[ok]
    return w


def laplacian(vertices, faces, steps=3, cotangent=True, boundary=True):
    p, faces = _mesh(vertices, faces)
    if len(faces) == 0:
        return p
    v0, v1, v2 = halfedges(faces)
    border = border_halfedges(faces) if boundary else np.zeros(len(v0), dtype=bool)
    inner = ~border
    i0, i1, i2 = v0[inner], v1[inner], v2[inner]
    b0, b1 = v0[border], v1[border]
    on = np.zeros(len(p), dtype=bool)
    on[b0] = True
    on[b1] = True
    for _ in range(steps):
        w = cot_weights(p, i0, i1, i2) if cotangent else np.ones(len(i0))
        acc, cnt = np.zeros_like(p), np.zeros(len(p))
        np.add.at(acc, i0, p[i1] * w[:, None])              # the half-edges that leave a vertex, ascending
        np.add.at(acc, i1, p[i0] * w[:, None])              # then those that arrive
        np.add.at(cnt, i0, w)
        np.add.at(cnt, i1, w)
        acc[on] = p[on]                                      # a border vertex forgets what its inner half-edges gathered
        cnt[on] = 1.0
        np.add.at(acc, b0, p[b1])
        np.add.at(acc, b1, p[b0])
        np.add.at(cnt, b0, 1.0)
        np.add.at(cnt, b1, 1.0)
        q = p.copy()                                         # Jacobi: every vertex reads the previous positions
        move = cnt > 0
        q[move] = (p[move] + acc[move]) / (cnt[move, None] + 1.0)
        p = q
    return p


def umbrella(vertices, faces, k0, k1=None, sweeps=1, neighbours="all"):
    p, faces = _mesh(vertices, faces)
    k1 = k0 if k1 is None else k1
    if len(faces) == 0:
        return p
    if neighbours == "border":
        src, dst = border_records(faces)
    else:
        v0, v1, _ = halfedges(faces)
        src, dst = np.concatenate([v0, v1]), np.concatenate([v1, v0])
    deg = np.zeros(len(p))
    np.add.at(deg, src, 1.0)
    move = deg > 0
    for s in range(sweeps):
        k = k1 if s % 2 else k0
        acc = np.zeros_like(p)
        np.add.at(acc, src, p[dst])
        q = p.copy()
        q[move] = p[move] + k * (acc[move] / deg[move, None] - p[move])
        p = q
    return p


def smooth_borders(vertices, faces, lam=0.3, iterations=20):
    return umbrella(vertices, faces, lam, lam, iterations, "border")


def taubin(vertices, faces, steps=10, lam=0.5, mu=-0.53):
    return umbrella(vertices, faces, lam, mu, 2 * steps, "all")


def vertex_normals(vertices, faces, weight="angle"):
    """(unit, raw)"""
    p, faces = _mesh(vertices, faces)
    raw = np.zeros_like(p)
    if len(faces):
        tri = p[faces]
        n = cross3(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        if weight == "angle":
            ln = norm3(n)
            unit = np.zeros_like(n)
            ok = ln > 0
            unit[ok] = n[ok] / ln[ok, None]
            n = unit
        for c in range(3):                                   # corners ascending in (c, f)
            term = n
            if weight == "angle":
                a, b = tri[:, (c + 1) % 3] - tri[:, c], tri[:, (c + 2) % 3] - tri[:, c]
                cs = dot3(a, b) / np.maximum(norm3(a) * norm3(b), 1e-300)
                term = n * np.arccos(np.clip(cs, -1.0, 1.0))[:, None]
            np.add.at(raw, faces[:, c], term)
    ln = norm3(raw)
    unit = np.zeros_like(raw)
    ok = ln > 0
    unit[ok] = raw[ok] / ln[ok, None]
    return unit, raw


def valence(faces, num_vertices):
    """corners per vertex"""
    return np.bincount(np.asarray(faces, dtype=np.int64).reshape(-1), minlength=num_vertices)


# ---- meshes -----------------------------------------------------------------------------------------------------------------
def sheet(n, noise=0.2, seed=0, shuffle=True):
    """an open n x n-vertex sheet over [0, n - 1]^2 with seeded noise in all three coordinates; 2 (n - 1)^2 faces, shuffled"""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([ii, jj, np.zeros_like(ii)], axis=-1).reshape(-1, 3).astype(np.float64) + noise * rng.standard_normal((n * n, 3))
    a = (ii[:-1, :-1] * n + jj[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)])
    if shuffle:
        f = f[rng.permutation(len(f))]
    return v, f.astype(np.int64)


def icosphere(level, noise=0.0, seed=0):
    """the unit icosphere, 20 * 4^level faces (midpoints found by sorting, so level 8 is affordable), with seeded noise"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    v /= np.sqrt((v * v).sum(axis=1, keepdims=True))
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], dtype=np.int64)
    for _ in range(level):
        e = np.sort(np.stack([f, f[:, [1, 2, 0]]], 2).reshape(-1, 2), 1)
        uniq, inv = np.unique(e[:, 0] * len(v) + e[:, 1], return_inverse=True)
        mid = v[uniq // len(v)] + v[uniq % len(v)]
        m = inv.reshape(-1, 3) + len(v)
        v = np.concatenate([v, mid / np.sqrt((mid * mid).sum(axis=1, keepdims=True))])
        a, b, c, ab, bc, ca = f[:, 0], f[:, 1], f[:, 2], m[:, 0], m[:, 1], m[:, 2]
        f = np.stack([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1), np.stack([ab, bc, ca], 1)], 1).reshape(-1, 3)
    if noise:
        v = v + noise * np.random.default_rng(seed).standard_normal(v.shape)
    return v, f


def fan(n=70, seed=3):
    """n triangles around vertex 0 (valence above the wave size), the rim open between the last and the first spoke"""
    rng = np.random.default_rng(seed)
    ang = np.linspace(0.0, 1.9 * np.pi, n + 1)
    v = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(ang), np.sin(ang), 0.1 * rng.standard_normal(n + 1)], 1)])
    f = np.stack([np.zeros(n, dtype=np.int64), np.arange(1, n + 1), np.arange(2, n + 2)], 1)
    return v, f


def shapes():
    """name -> (vertices float64, faces int64): the smallest meshes at which the kernels can go wrong"""
    rng = np.random.default_rng(11)
    tet_v = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 1.0, 0.1], [0.3, 0.2, 0.9]])
    tet_f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
    s5v, s5f = sheet(5, 0.2, seed=1)
    out = {
        "empty": (rng.standard_normal((3, 3)), np.zeros((0, 3), dtype=np.int64)),
        "one_triangle": (np.array([[0.0, 0.0, 0.0], [1.0, 0.2, 0.1], [0.1, 1.0, 0.3]]), np.array([[0, 1, 2]])),
        "two_triangles": (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [0.0, 1.0, 0.2], [1.1, 0.9, -0.3]]), np.array([[0, 1, 2], [2, 1, 3]])),
        "tetrahedron": (tet_v, tet_f),
        "sheet5": (s5v, s5f),
        "sheet40": sheet(40, 0.2, seed=2),
        "icosphere2": icosphere(2, 0.02, seed=4),
        "fan70": fan(70),
        # three triangles on the edge (0, 1): inner by the count rule
        "three_on_an_edge": (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.3, 1.0, 0.0], [0.4, -0.2, 1.0], [0.5, -1.0, -0.2]]),
                             np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]])),
        # a face with two equal indices between ordinary ones: its half-edge 1 -> 1 is a border half-edge from a vertex to itself
        "repeated_index": (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.2], [0.0, 1.0, 0.1], [1.0, 1.0, 0.4], [2.0, 0.3, 0.0]]),
                           np.array([[0, 1, 2], [1, 1, 3], [2, 1, 3], [1, 4, 3]])),
        # vertices 0, 1, 4 on one line: the face (0, 1, 4) has no area, w = 0 there
        "zero_area": (np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.5, 1.0, 0.2], [0.7, -1.0, 0.1], [1.0, 0.0, 0.0]]),
                      np.array([[0, 4, 2], [4, 1, 2], [0, 1, 4], [0, 3, 1]])),
        # vertex 4 is named by no face: it stays
        "unreferenced": (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [0.0, 1.0, 0.2], [1.1, 0.9, -0.3], [5.0, 5.0, 5.0]]), np.array([[0, 1, 2], [2, 1, 3]])),
    }
    return {k: (np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int64).reshape(-1, 3)) for k, (v, f) in out.items()}


WELL_CONDITIONED = ("sheet5", "sheet40", "icosphere2")        # no degenerate faces: the cotangents are bounded
