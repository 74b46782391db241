"""Sequential restatement of the contract of csrc/meshclean.hip: the cleaning functions of
surfd_amd.meshproc in the ORDER-FREE form the device builds, one plain Python loop per rule, with the arithmetic written out.

    cull_and_merge         key = (rint(x s), rint(y s), rint(z s)) as int64, s = 1 / tol; a class is the set of participating
                           vertices with one key, its survivor the lowest index; no lexicographic order anywhere
    drop_duplicate_faces   faces in ascending (largest, middle, smallest index, face), the first of every run survives
    drop_degenerate_faces  cross = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), |x| = sqrt((x0 x0 + x1 x1) + x2 x2)
    fill_small_holes       out(u), nxt(u) over the border half-edges; every vertex tests its own cycle; a cap lies at the slot of
                           its smallest vertex (no two caps share one), so ascending slots are the stable sort of meshproc
    clean_until_stable     meshproc's sequence with the counts that steer it, and the stats the device reports

tests/test_meshclean_cpu.py pins every function here to meshproc bit for bit; tests/test_gpu_meshclean.py pins the device to
meshproc.  Also here: the meshes both share (shapes()), the smallest at which each rule can go wrong; and, apart from them, the
meshes at size (big_shapes(): merges across the whole index range, duplicates among thousands of faces) and the families padded(),
relabelled(), side_by_side() and first_soups().  numpy only, every one seeded.
"""
import math

import numpy as np

KEY_LIMIT = 2.0 ** 62
STAT_KEYS = ("merged_vertices", "nonfinite_vertices", "unreferenced_vertices", "duplicate_faces", "degenerate_faces", "caps3", "caps4", "rounds")


def new_stats():
    return dict.fromkeys(STAT_KEYS, 0)


def _mesh(vertices, faces):
    return np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)


# ---- the four rules ---------------------------------------------------------------------------------------------------------
def quantise(x, scale):
    """the int64 key of one coordinate; ValueError beyond the range numpy's conversion defines"""
    q = x * scale
    if not abs(q) < KEY_LIMIT:
        raise ValueError(f"coordinate {x!r} is beyond the key range")
    return int(np.rint(q))                                   # ties to even; -0.0 -> 0


def cull_and_merge(vertices, faces, tol=1e-8, stats=None):
    v, f = _mesh(vertices, faces)
    if len(v) == 0 or len(f) == 0:
        return v[:0].reshape(0, 3), f[:0]
    scale = 1.0 / tol
    finite = [all(math.isfinite(c) for c in row) for row in v]
    kept = [t for t in f.tolist() if all(finite[i] for i in t)]
    part = [False] * len(v)
    for t in kept:
        for i in t:
            part[i] = True
    for i, row in enumerate(v):                              # numpy converts every finite vertex, taking part or not
        if finite[i]:
            for c in row:
                quantise(c, scale)
    survivor_of, rep = {}, [-1] * len(v)
    for i in range(len(v)):
        if part[i]:
            rep[i] = survivor_of.setdefault(tuple(quantise(c, scale) for c in v[i]), i)
    survivors = [i for i in range(len(v)) if part[i] and rep[i] == i]
    new = {s: n for n, s in enumerate(survivors)}
    if stats is not None:
        stats["nonfinite_vertices"] += finite.count(False)
        stats["unreferenced_vertices"] += sum(1 for i in range(len(v)) if finite[i] and not part[i])
        stats["merged_vertices"] += sum(part) - len(survivors)
    return v[survivors].reshape(-1, 3), np.array([[new[rep[i]] for i in t] for t in kept], dtype=np.int64).reshape(-1, 3)


def drop_duplicate_faces(faces, stats=None):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    rows = f.tolist()
    order = sorted(range(len(rows)), key=lambda i: (sorted(rows[i])[::-1], i))
    first = [i for n, i in enumerate(order) if n == 0 or sorted(rows[i]) != sorted(rows[order[n - 1]])]
    if stats is not None:
        stats["duplicate_faces"] += len(rows) - len(first)
    return f[first].reshape(-1, 3)


def _height_ok(p0, p1, p2, height):
    a = [p1[j] - p0[j] for j in range(3)]
    b = [p2[j] - p0[j] for j in range(3)]
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def norm(x):
        s = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]
        return math.sqrt(s) if s >= 0.0 else math.nan       # s is a NaN or >= 0 (squares); inf -> inf
    area = norm(c) * 0.5
    la, lb = norm(a), norm(b)
    with np.errstate(all="ignore"):
        ha = float(np.float64(2.0 * area) / np.float64(la)) if la > 1e-8 else 0.0
        hb = float(np.float64(2.0 * area) / np.float64(lb)) if lb > 1e-8 else 0.0
    return ha > height and hb > height


def drop_degenerate_faces(vertices, faces, height=1e-8, stats=None):
    v, f = _mesh(vertices, faces)
    pts = v.tolist()
    keep = [n for n, t in enumerate(f.tolist()) if _height_ok(pts[t[0]], pts[t[1]], pts[t[2]], height)]
    if stats is not None:
        stats["degenerate_faces"] += len(f) - len(keep)
    return f[keep].reshape(-1, 3)


def border_out_next(faces):
    """(out, nxt): per vertex the number of border half-edges that leave it and, where that is 1, where the one leads"""
    rows = np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist()
    half = [(t[c], t[(c + 1) % 3]) for t in rows for c in range(3)]
    count = {}
    for u, w in half:
        count[(min(u, w), max(u, w))] = count.get((min(u, w), max(u, w)), 0) + 1
    out, nxt = {}, {}
    for u, w in half:
        if count[(min(u, w), max(u, w))] == 1:
            out[u] = out.get(u, 0) + 1
            nxt[u] = w
    return out, nxt


def fill_small_holes(vertices, faces, stats=None):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) < 3:
        return f
    out, nxt = border_out_next(f)
    slot = {}                                                # smallest vertex of a cap -> the cap
    for u0 in out:                                           # any order: every vertex tests its own cycle
        if out[u0] != 1:
            continue
        loop, u = [u0], nxt[u0]
        while u != u0 and len(loop) < 4 and out.get(u, 0) == 1:
            loop.append(u)
            u = nxt[u]
        if u != u0 or len(loop) not in (3, 4) or min(loop) != u0:
            continue
        r = loop[::-1]
        caps = [r] if len(r) == 3 else [[r[0], r[1], r[2]], [r[2], r[3], r[0]]]
        for cap in caps:
            assert min(cap) not in slot
            slot[min(cap)] = cap
        if stats is not None:
            stats["caps3" if len(r) == 3 else "caps4"] += 1
    if not slot:
        return f
    return np.vstack([f, np.array([slot[m] for m in sorted(slot)], dtype=np.int64)])


def clean_until_stable(vertices, faces, max_iter=10):
    """(vertices, faces, stats): the sequence of meshproc.clean_until_stable; every count in stats is summed over the steps run,
    "rounds" are the duplicate / degenerate passes, the first one included (1 on the fast return)"""
    st = new_stats()
    st["rounds"] = 1
    v, f0 = cull_and_merge(vertices, faces, stats=st)
    f = drop_duplicate_faces(f0, st)
    n_dedup = len(f)
    f = drop_degenerate_faces(v, f, stats=st)
    n_degen = len(f)
    f = fill_small_holes(v, f, st)
    if n_dedup == len(f0) and n_degen == n_dedup and len(f) == n_degen:
        return v, f, st
    v, f = cull_and_merge(v, f, stats=st)
    counts, rounds = (0, 0), 0
    while counts != (len(v), len(f)) and rounds < max_iter:
        n_before = len(f)
        f = drop_duplicate_faces(f, st)
        f = drop_degenerate_faces(v, f, stats=st)
        counts = (len(v), len(f))
        rounds += 1
        st["rounds"] += 1
        if len(f) != n_before:
            v, f = cull_and_merge(v, f, stats=st)
    return v, f, st


# ---- meshes -----------------------------------------------------------------------------------------------------------------
_OCTA_V = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
# the four faces at the top vertex 4 in order round it, then the four at the bottom vertex 5
_OCTA_F = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
_TETRA_V = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
_TETRA_F = [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]
_CUBE_V = [[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)]
_CUBE_F = [[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]]


def _soup():
    h, up, down = 1.0 / 512.0, 4.9e-9, 5.1e-9
    v = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1],         # 0-3   a tetrahedron
         [1 + 4e-9, 0, 0],                                   # 4     within 1e-8 of 1: merged
         [-0.0, 0.0, -0.0],                                  # 5     -0.0 against 0.0: merged with 0
         [math.nan, 0, 0],                                   # 6     a NaN vertex
         [5, 5, 5],                                          # 7     named by no face
         [h, 2, 0], [h + up, 2, 0], [h - down, 2, 0],        # 8-10  195312.5 -> 195312 (even below); + up -> 195313; - down -> 195312
         [3 * h, 3, 0], [3 * h + up, 3, 0], [3 * h - down, 3, 0],      # 11-13 585937.5 -> 585938 (even above); + up -> 585938; - down -> 585937
         [-h, 4, 0],                                         # 14    -195312.5 -> -195312
         [2, 0, 0]]                                          # 15    on the line through 0 and 1
    f = [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2],
         [4, 5, 2],                                          # (1, 0, 2) after the merge: a rotation of face 0
         [3, 4, 5],                                          # (3, 1, 0): face 1 reversed
         [6, 0, 1],                                          # names the NaN vertex
         [0, 1, 15],                                         # collinear
         [2, 2, 3],                                          # a repeated index
         [8, 11, 14], [9, 12, 14], [10, 13, 14]]             # (8, 11, 14), (9, 11, 14), (8, 13, 14) after the merge
    return np.array(v, dtype=np.float64), np.array(f, dtype=np.int64)


def sheet(n, drop=0.05, seed=0):
    """an n x n sheet of quads over [0, 1]^2 with a gentle relief, two triangles per quad, a seeded share of the faces removed"""
    g = np.arange(n + 1) / n
    x, y = np.meshgrid(g, g, indexing="xy")
    v = np.stack([x.ravel(), y.ravel(), 0.05 * np.sin(5 * x.ravel()) * np.cos(3 * y.ravel())], axis=1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    a = (j * (n + 1) + i).ravel()
    b, c, d = a + 1, a + n + 1, a + n + 2
    f = np.stack([np.stack([a, b, d], axis=1), np.stack([a, d, c], axis=1)], axis=1).reshape(-1, 3)
    keep = np.random.default_rng(seed).random(len(f)) >= drop
    return v, f[keep].astype(np.int64)


def shapes():
    """name -> (vertices [V, 3] float64, faces [F, 3] int64)"""
    A = lambda v, f: (np.array(v, dtype=np.float64), np.array(f, dtype=np.int64))      # noqa: E731
    out = {"tetrahedron": A(_TETRA_V, _TETRA_F),
           "octahedron_minus_one": A(_OCTA_V, _OCTA_F[1:]),                                        # a 3-hole
           "cube_minus_quad": A(_CUBE_V, _CUBE_F[2:]),                                             # a 4-hole
           # a pentagonal bipyramid without the five faces at its top vertex 6: a 5-edge hole, and vertex 6 named by no face
           "pentagon_hole": A([[math.cos(2 * math.pi * k / 5), math.sin(2 * math.pi * k / 5), 0] for k in range(5)] + [[0, 0, -1], [0, 0, 1]],
                              [[(k + 1) % 5, k, 5] for k in range(5)]),
           # the top faces 0 and 2 meet in vertex 4 only: two 3-holes, two border half-edges leave vertex 4
           "octahedron_minus_two": A(_OCTA_V, [_OCTA_F[k] for k in (1, 3, 4, 5, 6, 7)]),
           "tetrahedron_and_triangle": A(_TETRA_V + [[3, 0, 0], [4, 0, 0], [3, 1, 0]], _TETRA_F + [[4, 5, 6]]),
           "tetrahedron_and_two_triangles": A(_TETRA_V + [[3, 0, 0], [4, 0, 0], [3, 1, 0], [4, 1, 0]], _TETRA_F + [[4, 5, 6], [5, 7, 6]]),
           "soup": _soup(),
           "sheet64": sheet(64)}
    return out


def random_soup(rng):
    """4 - 8 vertices on a coarse lattice (so vertices coincide and faces are collinear) with perturbations around the merge
    tolerance, 3 - 13 faces, every other soup with repeated indices inside faces"""
    nv, nf = int(rng.integers(4, 9)), int(rng.integers(3, 14))
    v = rng.integers(0, 2, size=(nv, 3)).astype(np.float64) / 512.0 * rng.choice([1.0, 3.0, 64.0])
    v += rng.choice([0.0, 0.0, 4.9e-9, -5.1e-9, 2e-8], size=v.shape)
    if rng.random() < 0.2:
        v[int(rng.integers(nv)), int(rng.integers(3))] = rng.choice([np.nan, np.inf])
    if rng.random() < 0.5:
        f = rng.integers(0, nv, size=(nf, 3))
    else:
        f = np.array([rng.choice(nv, size=3, replace=False) for _ in range(nf)])
    return v, f.astype(np.int64)


def first_soups(n=400, seed=7):
    """the first n soups of random_soup(default_rng(seed)): one generator stream, so a shorter list is a prefix of a longer one"""
    rng = np.random.default_rng(seed)
    return [random_soup(rng) for _ in range(n)]


# ---- meshes at size (big_shapes) and families of small ones (padded, relabelled, side_by_side) -------------------------------------
TORUS_VERTICES, TORUS_FACES = 96 * 88, 2 * 96 * 88           # raycast_ref.torus(96, 88): 8 448 and 16 896
SOUP_SHIFT = (-0.25, 0.125, -0.5)
JITTER = 4e-9                                                # 0.4 of a key: splits a class where a coordinate lies within 0.4 of a rounding edge


def unwelded(mesh, seed, shift=(0.0, 0.0, 0.0), jitter=0.0):
    """every face gets three vertices of its own (V = 3 F), faces and vertex labels shuffled, all coordinates shifted: the copies
    of one vertex keep equal bits and lie anywhere in the index range.  jitter: each coordinate of each copy moves by 0, +jitter
    or -jitter"""
    v, f = _mesh(*mesh)
    rng = np.random.default_rng(seed)
    f = f[rng.permutation(len(f))]
    pts = v[f.reshape(-1)] + np.asarray(shift, dtype=np.float64)
    if jitter:
        pts = pts + rng.choice([0.0, jitter, -jitter], size=pts.shape)
    label = rng.permutation(len(pts))                        # corner c of face k is vertex label[3 k + c]
    out = np.empty_like(pts)
    out[label] = pts
    return out, label.reshape(-1, 3).astype(np.int64)


FAN_EXTRA, FAN_NAN, FAN_NAN_FACES = 3000, 500, 40
FAN_APEX = (0.03125, -0.0625, 0.125)


def fan(n=5000, seed=5):
    """a disc of n triangles round one apex, unwelded (V = 3 n: the apex class has n members over the whole index range, every rim
    class 2), then FAN_EXTRA finite vertices that no face names (copies of fan corners, so each coincides with a class it must not
    join), FAN_NAN all-NaN vertices and FAN_NAN_FACES faces that each name one of them, all labels shuffled.  The x keys have both
    signs, so the vertices that take no part sort between the classes of positive and of negative x; the highest label among them
    goes to a copy of the rim vertex of the lowest x, the class that follows them in the device's order."""
    ang = np.arange(n) * (2.0 * np.pi / n)
    v = np.vstack([[FAN_APEX], np.stack([FAN_APEX[0] + np.cos(ang), FAN_APEX[1] + np.sin(ang), np.full(n, FAN_APEX[2])], axis=1)])
    k = np.arange(n)
    sv, sf = unwelded((v, np.stack([np.zeros(n, dtype=np.int64), 1 + k, 1 + (k + 1) % n], axis=1)), seed)
    rng = np.random.default_rng(seed + 1)
    extra = sv[rng.integers(0, len(sv), size=FAN_EXTRA)]
    extra[0] = v[1 + int(np.argmin(v[1:, 0]))]               # the rim vertex of the lowest x
    extra[1:64] = v[0]                                       # and copies of the apex
    nan_f = np.stack([rng.integers(0, len(sv), FAN_NAN_FACES), rng.integers(0, len(sv), FAN_NAN_FACES),
                      len(sv) + FAN_EXTRA + rng.choice(FAN_NAN, FAN_NAN_FACES, replace=False)], axis=1)
    allv = np.vstack([sv, extra, np.full((FAN_NAN, 3), np.nan)])
    allf = np.vstack([sf, nan_f])[rng.permutation(n + FAN_NAN_FACES)]
    perm = rng.permutation(len(allv))                        # vertex i becomes perm[i]
    top = len(sv) + int(np.argmax(perm[len(sv):]))           # the vertex with the highest label of those that take no part
    perm[[len(sv), top]] = perm[[top, len(sv)]]
    out = np.empty_like(allv)
    out[perm] = allv
    return out, perm[allf].astype(np.int64)


def doubled_sheet(seed=3):
    """sheet(64) with every face present two or three times (about 3 in 5 twice), each copy rotated by 0, 1 or 2 corners and about 2
    in 5 reversed, all faces shuffled"""
    v, f = sheet(64)
    rng = np.random.default_rng(seed)
    g = f[np.repeat(np.arange(len(f)), rng.choice([2, 3], size=len(f), p=[0.6, 0.4]))]
    g = np.take_along_axis(g, (np.arange(3)[None, :] + rng.integers(0, 3, size=(len(g), 1))) % 3, axis=1)
    rev = rng.random(len(g)) < 0.4
    g[rev] = g[rev][:, ::-1]
    return v, g[rng.permutation(len(g))].astype(np.int64)


_big = {}


def big_shapes():
    """name -> (vertices, faces): the meshes at size, built once and read-only.  Not part of shapes(): the parametrised tests over
    every function keep their run time"""
    if not _big:
        import raycast_ref
        torus = raycast_ref.torus(96, 88)
        assert torus[0].shape == (TORUS_VERTICES, 3) and torus[1].shape == (TORUS_FACES, 3)
        _big.update(torus_soup=unwelded(torus, 1, SOUP_SHIFT), torus_soup_jitter=unwelded(torus, 1, SOUP_SHIFT, JITTER), fan=fan(),
                    doubled_sheet=doubled_sheet())
        for v, f in _big.values():
            v.setflags(write=False); f.setflags(write=False)
    return _big


def loop_vertices(faces):
    """the vertices that exactly one border half-edge leaves, ascending"""
    out, _ = border_out_next(faces)
    return sorted(u for u in out if out[u] == 1)


PAD_SIZES = (255, 256, 257, 65535, 65536, 65537)
PAD_NAMES = ("octahedron_minus_one", "cube_minus_quad")


def padded(name, V, top=True, split=False):
    """(vertices, faces, new): a toy solid of shapes() inside V vertices, vertex i of the solid as new[i], every other vertex an
    unreferenced (0, 0, 0).  top: the solid takes the highest labels, the vertices of its border loop V - 1, V - 2, ... and the
    others below them; not top: the lowest labels, the loop first.  The loop's vertices keep their order among themselves, so the
    caps of the padded solid are the caps of the solid, re-indexed: same rows, same rotation, same order.
    split (with top): the loop stays at the top and the other vertices go to 0, 1, ... except one, m, which lies HALF THE KEY RANGE
    below a loop vertex L with which it shares a neighbour o among the others: at new[L] - 2^(b - 1), b the bits of an index
    below V.  The edges (L, o) and (m, o) then differ in the highest bit of the hole pass's sort key alone, and the faces are
    re-ordered so that a half-edge of (m, o) lies between the two of (L, o): a stable sort that left that bit out would part
    them.  (V = 2^k + 1: only V - 1 has that bit and no such pair exists; m stays with the others.)"""
    v, f = shapes()[name]
    loop = loop_vertices(f)
    rest = [i for i in range(len(v)) if i not in loop]
    new = np.empty(len(v), dtype=np.int64)
    if top and split:
        bits = 1
        while (1 << bits) < V:
            bits += 1
        edges = {frozenset(e) for t in f.tolist() for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
        L, m, o = next((L, m, o) for L in loop[::-1] for m in rest for o in rest if frozenset((L, o)) in edges and frozenset((m, o)) in edges)
        with_L = [k for k, t in enumerate(f.tolist()) if L in t and o in t]
        with_m = [k for k, t in enumerate(f.tolist()) if m in t and o in t]
        first = ([k for k in with_L if k not in with_m] + with_L)[0]
        second = [k for k in with_m if k != first][0]
        f = f[[first, second] + [k for k in range(len(f)) if k not in (first, second)]]
        new[loop] = np.arange(V - len(loop), V)
        others = [i for i in rest if i != m]
        new[others] = np.arange(len(others))
        new[m] = max(new[L] - (1 << (bits - 1)), len(others))
        assert new[m] < V - len(loop)
    elif top:
        new[rest] = np.arange(V - len(v), V - len(loop))
        new[loop] = np.arange(V - len(loop), V)
    else:
        new[loop] = np.arange(len(loop))
        new[rest] = np.arange(len(loop), len(v))
    out = np.zeros((V, 3), dtype=np.float64)
    out[new] = v
    return out, new[f], new


def relabelled(name, seed):
    """a toy solid of shapes() under a seeded random permutation of its vertex labels"""
    v, f = shapes()[name]
    perm = np.random.default_rng(seed).permutation(len(v))
    out = np.empty_like(v)
    out[perm] = v
    return out, perm[f]


RELABEL_SEEDS = {"cube_minus_quad": 64, "octahedron_minus_one": 16}


def relabellings():
    """[(name, seed, vertices, faces)]: cube_minus_quad under 64 permutations and octahedron_minus_one under 16"""
    return [(name, seed) + relabelled(name, seed) for name in sorted(RELABEL_SEEDS) for seed in range(RELABEL_SEEDS[name])]


def loop_pattern(faces):
    """the rank pattern of the one small loop of a toy solid: the ranks of its vertices among themselves, listed along the border
    from the smallest (which has rank 0).  A 4-loop has 6 patterns, a 3-loop 2."""
    out, nxt = border_out_next(faces)
    loop = [min(u for u in out if out[u] == 1)]
    while nxt[loop[-1]] != loop[0]:
        loop.append(nxt[loop[-1]])
    return tuple(sorted(loop).index(u) for u in loop)


def side_by_side(meshes, seed=None, gap=4.0):
    """the meshes as disjoint components of one, component k moved by k gap along x so that no two vertices coincide; with a seed
    all vertex labels are shuffled, so the loops' vertices interleave"""
    vs, fs, base = [], [], 0
    for k, (v, f) in enumerate(meshes):
        vs.append(np.asarray(v, dtype=np.float64) + np.array([k * gap, 0.0, 0.0]))
        fs.append(np.asarray(f, dtype=np.int64) + base)
        base += len(v)
    v, f = np.vstack(vs), np.vstack(fs)
    if seed is None:
        return v, f
    perm = np.random.default_rng(seed).permutation(len(v))
    out = np.empty_like(v)
    out[perm] = v
    return out, perm[f]
