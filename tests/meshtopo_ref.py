"""The contract of surfd_amd/meshtopo.py restated sequentially in numpy and plain Python: edges by sorting, every partition by one
textbook union-find walked pair by pair, the orientation by a breadth-first walk from the lowest face of every patch.  Nothing
here mirrors how the kernels work (no double cover, no atomics); it is the yardstick the device arrays are compared with,
exactly: every output is an integer or a bool.  Also the small meshes the tests share."""
from collections import deque

import numpy as np


# ---- edges --------------------------------------------------------------------------------------------------------------------
def build(triangles, num_vertices=None):
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    F = len(t)
    V = int(num_vertices) if num_vertices is not None else (int(t.max()) + 1 if F else 0)
    assert F == 0 or (t.min() >= 0 and t.max() < V)
    degenerate = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])
    a, b = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)              # half-edge h = 3 f + c runs a[h] -> b[h]
    live = np.repeat(~degenerate, 3)
    h = np.nonzero(live)[0]
    lo, hi = np.minimum(a[h], b[h]), np.maximum(a[h], b[h])
    order = np.lexsort((h, hi, lo))
    h, lo, hi = h[order], lo[order], hi[order]
    head = np.ones(len(h), dtype=bool)
    head[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    eid = np.cumsum(head) - 1
    E = int(head.sum())
    edges = np.stack([lo[head], hi[head]], 1).reshape(E, 2)
    edge_offsets = np.concatenate([np.nonzero(head)[0], [len(h)]]).astype(np.int64)
    valence = np.diff(edge_offsets)
    face_edges = np.full(3 * F, -1, dtype=np.int64)
    face_edges[h] = eid
    face_neighbors = np.full(3 * F, -1, dtype=np.int64)
    s = edge_offsets[:-1][valence == 2]
    face_neighbors[h[s]], face_neighbors[h[s + 1]] = h[s + 1] // 3, h[s] // 3
    face_neighbors[h[valence[eid] >= 3]] = -2
    return {"F": F, "V": V, "E": E, "triangles": t, "degenerate": degenerate, "edges": edges, "valence": valence,
            "edge_offsets": edge_offsets, "edge_halfedges": h, "face_edges": face_edges.reshape(F, 3),
            "face_neighbors": face_neighbors.reshape(F, 3), "referenced": int(len(np.unique(t[~degenerate])))}


# ---- union-find ---------------------------------------------------------------------------------------------------------------
class _Sets:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, x):
        p = self.p
        r = x
        while p[r] != r:
            r = p[r]
        while p[x] != r:
            p[x], x = r, p[x]
        return r

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.p[max(a, b)] = min(a, b)


def _number(keys, live):
    """labels in ascending order of the first live item that carries a key, -1 for the others"""
    labels = np.full(len(keys), -1, dtype=np.int64)
    seen = {}
    for i, (k, ok) in enumerate(zip(keys, live)):
        if ok:
            labels[i] = seen.setdefault(k, len(seen))
    return labels, np.bincount(labels[labels >= 0], minlength=len(seen)).astype(np.int64)


def components(topo, connectivity):
    t, deg, F = topo["triangles"], topo["degenerate"], topo["F"]
    if connectivity == "vertex":
        s = _Sets(topo["V"])
        for f in range(F):
            if not deg[f]:
                s.union(int(t[f, 0]), int(t[f, 1])); s.union(int(t[f, 1]), int(t[f, 2]))
        keys = [s.find(int(t[f, 0])) for f in range(F)]
    else:
        assert connectivity in ("edge", "manifold")
        s = _Sets(F)
        off, he, val = topo["edge_offsets"], topo["edge_halfedges"], topo["valence"]
        for e in range(topo["E"]):
            if connectivity == "manifold" and val[e] != 2:
                continue
            for i in range(off[e] + 1, off[e + 1]):
                s.union(int(he[off[e]]) // 3, int(he[i]) // 3)
        keys = [s.find(f) for f in range(F)]
    return _number(keys, ~deg)


def border_loops(topo):
    """(labels per border edge in edge order, sizes, simple)"""
    border = np.nonzero(topo["valence"] == 1)[0]
    s = _Sets(topo["E"])
    at = {}
    for e in border:
        for v in topo["edges"][e]:
            at.setdefault(int(v), []).append(int(e))
    for es in at.values():
        for e in es[1:]:
            s.union(es[0], e)
    labels, sizes = _number([s.find(int(e)) for e in border], np.ones(len(border), dtype=bool))
    simple = np.ones(len(sizes), dtype=bool)
    for v, es in at.items():
        if len(es) != 2:
            simple[labels[np.searchsorted(border, es[0])]] = False
    return labels, sizes, simple


# ---- orientation --------------------------------------------------------------------------------------------------------------
VOLUME_K = 30


def signed_volume_terms(vertices, triangles):
    """the integer the contract assigns to every face: rint(det(v0, v1, v2) 2^k / M^3), M the power of two >= max |coordinate|"""
    v = np.asarray(vertices, dtype=np.float32)
    fin = np.abs(v[np.isfinite(v)])
    m = float(fin.max()) if len(fin) else 0.0
    ex = 0
    if m > 0:
        fr, ex = np.frexp(np.float64(m))
        if fr == 0.5:
            ex -= 1
    p = v.astype(np.float64)[np.asarray(triangles, dtype=np.int64)]
    v0, v1, v2 = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        cx = v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1]
        cy = v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2]
        cz = v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]
        det = (v0[:, 0] * cx + v0[:, 1] * cy) + v0[:, 2] * cz
        scaled = det * np.ldexp(1.0, VOLUME_K - 3 * int(ex))
    ok = np.isfinite(scaled) & (np.abs(scaled) < 9.0e18)
    return [int(np.rint(x)) if o else 0 for x, o in zip(scaled, ok)]


def orientation(topo, vertices=None):
    """(flip [F] bool, patch_orientable [P] bool): a breadth-first walk over the manifold edges from the lowest face of every
    patch; a face met again with the other winding makes the patch non-orientable (its flips are then all False).  With
    vertices: closed orientable patches are then turned so that their integer volume is positive."""
    F, val = topo["F"], topo["valence"]
    nb, fe, tl = topo["face_neighbors"].tolist(), topo["face_edges"].tolist(), topo["triangles"].tolist()
    labels, sizes = components(topo, "manifold")
    flip = np.zeros(F, dtype=bool)
    patch_orientable = np.ones(len(sizes), dtype=bool)
    seen = np.zeros(F, dtype=bool)
    for f0 in range(F):
        if labels[f0] < 0 or seen[f0]:
            continue
        seen[f0] = True
        members, ok = [f0], True
        todo = deque([f0])
        while todo:
            f = todo.popleft()
            for c in range(3):
                g = nb[f][c]
                if g < 0:
                    continue
                d = fe[g].index(fe[f][c])
                same_direction = (tl[f][c] < tl[f][(c + 1) % 3]) == (tl[g][d] < tl[g][(d + 1) % 3])
                want = bool(flip[f]) ^ bool(same_direction)          # g's flip so that the two half-edges run in opposite directions
                if not seen[g]:
                    seen[g] = True
                    flip[g] = want
                    members.append(g); todo.append(g)
                elif bool(flip[g]) != want:
                    ok = False
        if not ok:
            patch_orientable[labels[f0]] = False
            flip[members] = False
    if vertices is not None and F:
        terms = signed_volume_terms(vertices, topo["triangles"])
        face_closed = np.array([labels[f] >= 0 and all(val[fe[f][c]] == 2 for c in range(3)) for f in range(F)])
        for p in range(len(sizes)):
            members = np.nonzero(labels == p)[0]
            if patch_orientable[p] and face_closed[members].all():
                vol = sum(-terms[f] if flip[f] else terms[f] for f in members)
                if vol < 0:
                    flip[members] = ~flip[members]
    return flip, patch_orientable


def oriented(triangles, flip):
    t = np.asarray(triangles, dtype=np.int64).copy()
    t[flip] = t[flip][:, [0, 2, 1]]
    return t


def same_direction_manifold_edges(triangles):
    """how many valence-2 edges carry two half-edges that run in the same direction, counted straight from the index array
    (not through build()): the property an oriented mesh must have is that this is 0"""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    a, b = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)
    und = np.minimum(a, b) * (int(t.max()) + 1 if len(t) else 1) + np.maximum(a, b)
    _, inv, cnt = np.unique(und, return_inverse=True, return_counts=True)
    forward = np.bincount(inv, weights=(a < b), minlength=len(cnt))
    return int(((cnt == 2) & (forward != 1)).sum())


# ---- weld ---------------------------------------------------------------------------------------------------------------------
def weld(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float32)
    first, vmap_old = {}, np.empty(len(v), dtype=np.int64)
    for i, p in enumerate(v):
        if np.isnan(p).any():
            vmap_old[i] = i
            continue
        key = tuple(float(x) + 0.0 for x in p)                    # -0.0 + 0.0 = +0.0
        vmap_old[i] = first.setdefault(key, i)
    survivor = vmap_old == np.arange(len(v))
    new = np.cumsum(survivor) - 1
    vmap = new[vmap_old]
    return v[survivor], vmap[np.asarray(triangles, dtype=np.int64)], vmap


# ---- the numbers --------------------------------------------------------------------------------------------------------------
def summary(topo):
    val = topo["valence"]
    deg = topo["degenerate"]
    t, fe = topo["triangles"], topo["face_edges"]
    labels, sizes = components(topo, "manifold")
    flip, po = orientation(topo)
    loops = border_loops(topo)
    patches = []
    for p in range(len(sizes)):
        m = np.nonzero(labels == p)[0]
        closed = bool((val[fe[m]] == 2).all())
        chi = len(np.unique(t[m])) - len(np.unique(fe[m])) + len(m)
        patches.append({"faces": int(len(m)), "closed": closed, "orientable": bool(po[p]),
                        "genus": (2 - chi) // 2 if closed and po[p] else None})
    nb, nm, nn = int((val == 1).sum()), int((val == 2).sum()), int((val >= 3).sum())
    live = int((~deg).sum())
    return {
        "faces": topo["F"], "degenerate_faces": int(deg.sum()), "referenced_vertices": topo["referenced"],
        "edges": topo["E"], "border_edges": nb, "manifold_edges": nm, "non_manifold_edges": nn,
        "euler_characteristic": topo["referenced"] - topo["E"] + live,
        "components_vertex": len(components(topo, "vertex")[1]), "components_edge": len(components(topo, "edge")[1]),
        "components_manifold": len(sizes),
        "border_loops": len(loops[1]), "largest_border_loop": int(loops[1].max()) if len(loops[1]) else 0,
        "closed": int(deg.sum()) == 0 and nb == 0 and nn == 0, "edge_manifold": nn == 0,
        "orientable": bool(po.all()), "consistently_oriented": bool(po.all()) and not bool(flip.any()),
        "patches": patches,
    }


def keep_components_with_at_least(vertices, faces, min_faces):
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    labels, sizes = components(build(faces, len(vertices)), "vertex")
    kept = faces[sizes[labels] >= min_faces]
    used = np.zeros(len(vertices), dtype=bool)
    used[kept] = True
    return np.asarray(vertices)[used], (np.cumsum(used) - 1)[kept]


# ---- meshes -------------------------------------------------------------------------------------------------------------------
def band(n=16, twist=False):
    """n quads (2 n triangles) around a ring: an annulus, or with ``twist`` a Moebius band.  Vertices 2 i (bottom) and 2 i + 1
    (top) of column i; the last quad closes onto column 0, upside down when twisted."""
    ang = np.arange(n) * (2 * np.pi / n)
    half = ang / 2 if twist else np.zeros(n)
    v = []
    for a, h in zip(ang, half):
        for s in (-1, 1):
            r = 1 + 0.3 * s * np.cos(h)
            v.append((r * np.cos(a), r * np.sin(a), 0.3 * s * np.sin(h)))
    f = []
    for i in range(n):
        a, b = 2 * i, 2 * i + 1
        if i + 1 < n:
            c, d = 2 * (i + 1), 2 * (i + 1) + 1
        else:
            c, d = (1, 0) if twist else (0, 1)
        f += [(a, c, d), (a, d, b)]
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.int64)


def strip(n=100_000):
    """n triangles in a row between two rails: diameter n, one border loop of n + 2 edges"""
    k = np.arange(n)
    f = np.stack([k, k + 1, k + 2], 1)
    f[1::2] = f[1::2][:, [0, 2, 1]]                                # alternate so that the strip is consistently oriented
    v = np.stack([(np.arange(n + 2) // 2).astype(np.float32), (np.arange(n + 2) % 2).astype(np.float32), np.zeros(n + 2, np.float32)], 1)
    return v, f.astype(np.int64)


def turned_and_shuffled(faces, fraction=0.4, seed=0):
    """(faces with a seeded fraction turned and the order shuffled, the permutation, the turned mask in the new order)"""
    rng = np.random.default_rng(seed)
    f = np.asarray(faces, dtype=np.int64).copy()
    turned = rng.random(len(f)) < fraction
    f[turned] = f[turned][:, [0, 2, 1]]
    perm = rng.permutation(len(f))
    return f[perm], perm, turned[perm]


def two_cubes(share="edge"):
    """two unit cubes that share one edge (valence 4) or one vertex, as one mesh with shared indices"""
    from raycast_ref import cube
    v, f = cube()
    shift = np.array([1, 1, 0] if share == "edge" else [1, 1, 1], dtype=np.float32)
    v2 = v + shift
    vmap = np.arange(8) + 8
    for i in range(8):
        j = np.nonzero((v == v2[i]).all(1))[0]
        if len(j):
            vmap[i] = j[0]
    keep = vmap >= 8
    new = np.cumsum(keep) - 1 + 8
    vmap = np.where(keep, new, vmap)
    return np.concatenate([v, v2[keep]]), np.concatenate([f, vmap[f]])


def interleaved_copies(v, f, copies=64):
    """disjoint copies of one mesh, their faces interleaved face by face (copy c's face i is face i * copies + c)"""
    fs = np.stack([f + c * len(v) for c in range(copies)], 1).reshape(-1, 3)
    vs = np.concatenate([v + np.float32(3 * c) for c in range(copies)])
    return vs, fs


def exploded(v, f):
    """every face gets three vertices of its own"""
    return v[f.reshape(-1)], np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3)
