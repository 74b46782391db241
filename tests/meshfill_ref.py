"""Sequential restatement of the contract of csrc/meshfill.hip: border loops of any length up to
``max_edges`` are closed by their minimum-total-area triangulation (Barequet and Sharir; the area term of Liepa 2003 without the
dihedral one), one plain Python loop per rule, the arithmetic written out.  It is the yardstick of tests/test_meshfill_cpu.py
and tests/test_gpu_meshfill.py, not a product path.

    border      half-edge 3 f + c runs t[f, c] -> t[f, (c + 1) % 3]; it is a BORDER half-edge iff its unordered pair occurs once among
                all 3 F half-edges (faces with repeated indices take part, as in meshclean_ref.border_out_next).  out(u) / in(u) count
                the border half-edges that leave / enter u, nxt(u) is where the one leads where out(u) == 1.
    loops       u is REGULAR iff out(u) == 1 and in(u) == 1.  A loop is a cycle u0 -> nxt(u0) -> ... -> u0 of n >= 3 regular vertices
                listed from its smallest vertex u0; loops are numbered in ascending u0, the ones that stay open included.  Border
                half-edges on no loop are ``irregular_border_edges``.  n > max_edges: the loop stays open (``loops_too_long``).
    listing     r_m = u_((n - m) mod n): the border reversed, so that the caps take the orientation of the faces round them.
    DP          W[i][i+1] = 0; W[i][j] = min over i < k < j of S = (W[i][k] + W[k][j]) + A(i, k, j) with a = P_k - P_i, b = P_j - P_i,
                c = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), A = sqrt((c0 c0 + c1 c1) + c2 c2) * 0.5, every operation rounded
                once.  The winner is the least (S, k) in the order: a number before a NaN, the smaller S, the smaller k.  A loop whose
                W[0][n-1] is not finite stays open (``loops_nonfinite``).
    caps        n - 2 rows (r_i, r_k, r_j) in PREORDER of the recursion: the triangle of (i, j), everything of (i, k), everything of
                (k, j).  Output faces: the input faces, then the caps of the filled loops in ascending loop number.

numpy only, every mesh seeded.
"""
import math

import numpy as np

COUNT_KEYS = ("loops_filled", "caps", "loops_too_long", "loops_nonfinite", "irregular_border_edges", "border_edges", "longest_filled")
MAX_EDGES_LIMIT = 1024


# ---- the rules ----------------------------------------------------------------------------------------------------------------
def border_in_out_next(faces):
    """(out, inn, nxt) over the border half-edges, as dicts by vertex"""
    rows = np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist()
    half = [(t[c], t[(c + 1) % 3]) for t in rows for c in range(3)]
    count = {}
    for u, w in half:
        key = (min(u, w), max(u, w))
        count[key] = count.get(key, 0) + 1
    out, inn, nxt = {}, {}, {}
    for u, w in half:
        if count[(min(u, w), max(u, w))] == 1:
            out[u] = out.get(u, 0) + 1
            inn[w] = inn.get(w, 0) + 1
            nxt[u] = w
    return out, inn, nxt


def loops(faces):
    """([loop, ...] in ascending smallest vertex, each listed along the border from that vertex; the number of border half-edges)"""
    out, inn, nxt = border_in_out_next(faces)
    regular = {u for u in out if out[u] == 1 and inn.get(u, 0) == 1}
    found, seen = [], set()
    for u0 in sorted(regular):
        if u0 in seen:
            continue
        walk, u = [u0], nxt[u0]
        while u != u0 and u in regular and u not in seen:
            walk.append(u)
            u = nxt[u]
        seen.update(walk)
        if u == u0 and len(walk) >= 3:                       # u0 is the smallest: a smaller vertex of the cycle would have walked it
            found.append(walk)
    return found, sum(out.values())


def area(p, q, r):
    a = [q[0] - p[0], q[1] - p[1], q[2] - p[2]]
    b = [r[0] - p[0], r[1] - p[1], r[2] - p[2]]
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    s = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
    return (math.sqrt(s) if s >= 0.0 else math.nan) * 0.5    # s is a NaN or >= 0 (squares); inf -> inf


def better(s, k, bs, bk):
    """(s, k) before (bs, bk): a number before a NaN, the smaller sum, the smaller k"""
    ns, nb = s != s, bs != bs
    if ns != nb:
        return nb
    if not ns and s != bs:
        return s < bs
    return k < bk


def triangulate(points):
    """(total, [(i, k, j), ...] in preorder) of the listing's positions; total is W[0][n-1]"""
    n = len(points)
    P = [[float(c) for c in p] for p in points]
    W = [[0.0] * n for _ in range(n)]
    K = [[0] * n for _ in range(n)]
    for d in range(2, n):
        for i in range(n - d):
            j = i + d
            bs, bk = math.nan, n
            for k in range(i + 1, j):
                s = (W[i][k] + W[k][j]) + area(P[i], P[k], P[j])
                if better(s, k, bs, bk):
                    bs, bk = s, k
            W[i][j], K[i][j] = bs, bk
    rows, stack = [], [(0, n - 1)]
    while stack:
        i, j = stack.pop()
        k = K[i][j]
        rows.append((i, k, j))
        if j - k >= 2:
            stack.append((k, j))
        if k - i >= 2:
            stack.append((i, k))
    return W[0][n - 1], rows


def triangulate_spans(points):
    """triangulate() with every span d = j - i evaluated at once in numpy: the same operations on the same operands, one rounding
    each, so the same bits (tests/test_meshfill_cpu.py pins the two against each other); what fill_holes runs, since the plain
    loops take minutes at a thousand edges"""
    n = len(points)
    P = np.asarray(points, dtype=np.float64).reshape(n, 3)
    W = np.zeros((n, n))
    K = np.zeros((n, n), dtype=np.int64)
    with np.errstate(all="ignore"):
        for d in range(2, n):
            i = np.arange(n - d)[:, None]
            k = i + np.arange(1, d)[None, :]
            j = i + d
            a, b = P[k] - P[i], P[j] - P[i]
            c0 = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
            c1 = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
            c2 = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
            S = (W[i, k] + W[k, j]) + np.sqrt((c0 * c0 + c1 * c1) + c2 * c2) * 0.5
            nan = np.isnan(S)
            first = np.argmin(np.where(nan, np.inf, S), axis=1)          # the first least number; an Inf is a number
            alone = nan[np.arange(n - d), first]                         # the row holds NaNs only: its first, or an Inf further on
            first = np.where(alone, np.argmax(~nan, axis=1), first)      # argmax of all-False is 0: the smallest k
            W[i[:, 0], j[:, 0]] = S[np.arange(n - d), first]
            K[i[:, 0], j[:, 0]] = k[np.arange(n - d), first]
    rows, stack = [], [(0, n - 1)]
    while stack:
        i, j = stack.pop()
        k = int(K[i, j])
        rows.append((i, k, j))
        if j - k >= 2:
            stack.append((k, j))
        if k - i >= 2:
            stack.append((i, k))
    return float(W[0, n - 1]), rows


def fill_holes(vertices, faces, max_edges=128):
    """(faces with the caps appended [F + caps, 3] int64, cap_loop [caps] int64, counts)"""
    if not 3 <= max_edges <= MAX_EDGES_LIMIT:
        raise ValueError(f"max_edges must lie in [3, {MAX_EDGES_LIMIT}], got {max_edges}")
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    st = dict.fromkeys(COUNT_KEYS, 0)
    if len(f) == 0 or len(v) == 0:
        return f, np.zeros(0, dtype=np.int64), st
    found, st["border_edges"] = loops(f)
    st["irregular_border_edges"] = st["border_edges"] - sum(len(w) for w in found)
    caps, cap_loop = [], []
    pts = v.tolist()
    for number, walk in enumerate(found):
        n = len(walk)
        if n > max_edges:
            st["loops_too_long"] += 1
            continue
        r = [walk[(n - m) % n] for m in range(n)]
        total, rows = triangulate_spans([pts[u] for u in r])
        if not math.isfinite(total):
            st["loops_nonfinite"] += 1
            continue
        st["loops_filled"] += 1
        st["longest_filled"] = max(st["longest_filled"], n)
        caps += [[r[i], r[k], r[j]] for i, k, j in rows]
        cap_loop += [number] * len(rows)
    st["caps"] = len(caps)
    out = np.vstack([f, np.array(caps, dtype=np.int64).reshape(-1, 3)])
    return out, np.array(cap_loop, dtype=np.int64), st


def hole_sizes(faces):
    """the lengths of all loops, ascending"""
    return sorted(len(w) for w in loops(faces)[0])


def best_total_exhaustive(points):
    """the least total area over ALL triangulations of the polygon, by plain recursion without a table (n <= 10 or so)"""
    P = [[float(c) for c in p] for p in points]

    def rec(i, j):
        if j - i < 2:
            return [0.0]
        return [(a + b) + area(P[i], P[k], P[j]) for k in range(i + 1, j) for a in rec(i, k) for b in rec(k, j)]
    return min(rec(0, len(P) - 1))


# ---- meshes -------------------------------------------------------------------------------------------------------------------
def ring(n, seed=0, rotate=0, noise=0.15):
    """a noisy, non-planar ring of n vertices fanned to a far apex: n faces, the ring its only border.  ``rotate`` shifts the
    numbering of the ring so that the loop's smallest vertex sits ``rotate`` steps further along the border."""
    rng = np.random.default_rng(seed)
    t = 2.0 * np.pi * np.arange(n) / n
    p = np.stack([np.cos(t), np.sin(t), np.zeros(n)], axis=1) + noise * rng.standard_normal((n, 3)) * (2.0 * np.pi / n)
    p[:, 2] += 0.2 * np.sin(3 * t)
    name = (np.arange(n) + rotate) % n                       # position on the ring -> vertex index
    v = np.zeros((n + 1, 3))
    v[name] = p
    v[n] = [0.0, 0.0, 5.0]
    f = np.stack([name, np.roll(name, -1), np.full(n, n)], axis=1)
    return v, f.astype(np.int64)


def flat_hexagon():
    """a flat regular hexagon ring fanned to an apex: every triangulation of the hole has the same area in exact arithmetic"""
    t = 2.0 * np.pi * np.arange(6) / 6
    v = np.vstack([np.stack([np.cos(t), np.sin(t), np.zeros(6)], axis=1), [[0.0, 0.0, 3.0]]])
    f = np.array([[i, (i + 1) % 6, 6] for i in range(6)], dtype=np.int64)
    return v, f


def flat_grid_hole(n=5, lo=1, hi=4):
    """a flat n x n grid of unit quads (integer coordinates, every area exact) with the quads [lo, hi)^2 removed"""
    v = np.array([[x, y, 0.0] for y in range(n + 1) for x in range(n + 1)], dtype=np.float64)
    f = []
    for y in range(n):
        for x in range(n):
            if lo <= x < hi and lo <= y < hi:
                continue
            a = y * (n + 1) + x
            b, c, d = a + 1, a + n + 1, a + n + 2
            f += [[a, b, d], [a, d, c]]
    return v, np.array(f, dtype=np.int64)


SHEET_BLOCKS = ((4, 4, 12), (22, 6, 9), (8, 24, 4), (24, 24, 2))      # (x0, y0, side) in quads


def bumped_sheet(n=40, drop=0.05, seed=0, blocks=SHEET_BLOCKS):
    """an n x n sheet of quads with a relief, two triangles per quad, a seeded share of its faces removed, except that the outer
    ring of quads stays (the outer border is ONE loop of 4 n edges) and that square blocks of quads go with the ring round each
    kept (loops of 4 side edges).  The random removals give loops of 3 and more edges and, where two of them touch in a vertex,
    irregular borders.  n = 40, seed 0: loops of 3 .. 16, 36, 48 and 160 edges, 112 irregular border edges."""
    g = np.arange(n + 1) / n
    x, y = np.meshgrid(g, g, indexing="xy")
    v = np.stack([x.ravel(), y.ravel(), 0.1 * np.sin(9 * x.ravel()) * np.cos(7 * y.ravel())], axis=1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    i, j = i.ravel(), j.ravel()
    a = j * (n + 1) + i
    b, c, d = a + 1, a + n + 1, a + n + 2
    f = np.stack([np.stack([a, b, d], axis=1), np.stack([a, d, c], axis=1)], axis=1).reshape(-1, 3)
    keep = np.random.default_rng(seed).random(len(f)) >= drop
    keep |= np.repeat((i == 0) | (j == 0) | (i == n - 1) | (j == n - 1), 2)
    for x0, y0, side in blocks:
        keep |= np.repeat((i >= x0 - 1) & (i <= x0 + side) & (j >= y0 - 1) & (j <= y0 + side), 2)
        keep &= ~np.repeat((i >= x0) & (i < x0 + side) & (j >= y0) & (j < y0 + side), 2)
    return v, f[keep].astype(np.int64)


def icosphere(level):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [list(np.array(p, dtype=np.float64) / np.linalg.norm(p)) for p in v]
    for _ in range(level):
        mid, g = {}, []
        for a, b, c in f:
            m = []
            for p, q in ((a, b), (b, c), (c, a)):
                key = (min(p, q), max(p, q))
                if key not in mid:
                    x = (np.array(v[p]) + np.array(v[q])) / 2.0
                    mid[key] = len(v)
                    v.append(list(x / np.linalg.norm(x)))
                m.append(mid[key])
            g += [[a, m[0], m[2]], [b, m[1], m[0]], [c, m[2], m[1]], [m[0], m[1], m[2]]]
        f = g
    return np.array(v, dtype=np.float64), np.array(f, dtype=np.int64)


def punched_icosphere(level=3, apart=3):
    """an icosphere with the stars of a greedy set of vertices pairwise more than ``apart`` edges apart removed: loops of 5 and 6
    edges, no two of them closer than one ring of faces, so no cap can repeat an edge of the mesh.  (vertices, faces, stars removed)"""
    v, f = icosphere(level)
    nb = [set() for _ in range(len(v))]
    for a, b, c in f.tolist():
        nb[a] |= {b, c}; nb[b] |= {a, c}; nb[c] |= {a, b}
    blocked, centres = set(), []
    for u in range(len(v)):
        if u in blocked:
            continue
        centres.append(u)
        ball, front = {u}, {u}
        for _ in range(apart):
            front = set().union(*(nb[w] for w in front)) - ball
            ball |= front
        blocked |= ball
    drop = set(centres)
    keep = np.array([not (set(t) & drop) for t in f.tolist()])
    return v, f[keep], len(centres)


def side_by_side(meshes, gap=4.0):
    """the meshes in one, each shifted along x, indices offset: loops of several lengths (and kinds) in one call"""
    vs, fs, base = [], [], 0
    for n, (v, f) in enumerate(meshes):
        vs.append(np.asarray(v, dtype=np.float64) + [gap * n, 0.0, 0.0])
        fs.append(np.asarray(f, dtype=np.int64) + base)
        base += len(v)
    return np.vstack(vs), np.vstack(fs)
