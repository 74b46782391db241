"""Yardsticks of the mesh intersection tests (surfd_amd/csrc/meshintersect.hip, surfd_amd/meshintersect.py); numpy only.

  restatement   the kernel's snap in np.float32, then every decision in int64, vectorised over pairs: ``verdicts``,
                ``self_pairs``, ``between_pairs``, ``result``.  Every GPU buffer is required equal to it.
  second form   the same decisions written again for one pair in Python integers (arbitrary precision): ``verdict_big``.
                Where the two agree on coordinates at +-2^19 no int64 product overflowed.

The contract of one pair:

  snap      q = rint(x * 2^L) in fp32 (the product with a power of two is exact: one rounding), converted to an integer; a NaN
            or |q| > 2^19 is refused.  Two vertices are the same point when their snapped coordinates are equal.
  o3        o3(a, b, c, d) = ((b - a) x (c - a)) . (d - a), the dot product summed as (x + y) + z: differences <= 2^20, cross
            components <= 2^41, every partial sum < 3 * 2^61.
  o2        the 2-D orientation after dropping the axis of the largest |normal component| of the triangle concerned (the lower
            axis on a tie); the kept axes are (axis + 1, axis + 2) mod 3.  Values <= 2^41.
  degenerate  a triangle whose normal (b - a) x (c - a) is (0, 0, 0): reported, intersects nothing.
  segment pq against triangle abc, both closed:  sp = sign o3(a, b, c, p), sq = sign o3(a, b, c, q).  Both strictly on one side:
            no.  Both zero: yes iff p or q lies in the triangle (o2(a, b, .), o2(b, c, .), o2(c, a, .) all >= 0 or all <= 0) or pq
            meets an edge (closed 2-D segment test: the four o2 signs differ pairwise, or one is zero and its point lies in the
            other segment's box on both kept axes).  Otherwise: yes iff o3(p, q, a, b), o3(p, q, b, c), o3(p, q, c, a) are all >= 0
            or all <= 0.
  closed test  some edge of A meets B or some edge of B meets A.
  verdict   inside one mesh, by the number k of points the two triangles share:  0: the closed test (touching counts);
            1: the edge of A opposite the shared point meets B, or the edge of B opposite it meets A (a T-junction counts);
            2: the corners c of A and d of B opposite the shared edge uw have o3(u, w, c, d) == 0 and o2(u, w, c), o2(u, w, d)
            of equal sign in A's projection (a fold laid flat); 3: yes (duplicates).  Between two meshes: the closed test.
"""
from __future__ import annotations

import numpy as np

import raycast_ref as rr

SNAP_MAX = 1 << 19
F32 = np.float32
I64 = np.int64


# ---- snap -------------------------------------------------------------------------------------------------------------------------
def snap(x, L):
    """-> (q int64, valid bool) of fp32 coordinates"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(x, F32) * F32(2.0 ** L))
        valid = np.abs(r) <= F32(SNAP_MAX)
    return np.where(valid, r, 0).astype(I64), valid


def snap_mesh(vertices, faces, L):
    """-> tri int64 [F, 3, 3]; raises ValueError where the library's create refuses"""
    vertices, faces = np.asarray(vertices, F32).reshape(-1, 3), np.asarray(faces, I64).reshape(-1, 3)
    if not len(faces) or ((faces < 0) | (faces >= len(vertices))).any():
        raise ValueError("no faces, or an index outside [0, V)")
    q, valid = snap(vertices, L)
    if not valid.all():
        raise ValueError(f"{int((~valid).any(1).sum())} vertices are NaN or beyond the lattice")
    return q[faces]


def lattice_for(*vertex_arrays):
    """the largest L with max|x| * 2^L <= 2^19"""
    m = max(float(np.abs(np.asarray(v, F32)).max()) for v in vertex_arrays)
    if m == 0:
        return 19
    f, e = np.frexp(m)                                   # m = f * 2^e, 0.5 <= f < 1
    return int(19 - e + (1 if f == 0.5 else 0))


# ---- the restatement: int64, vectorised over pairs --------------------------------------------------------------------------------
def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1],
                     u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _o3(a, b, c, d):
    return _dot(_cross(b - a, c - a), d - a)


def normals(tri):
    return _cross(tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :])


def drop_axis(n):
    return np.argmax(np.abs(n), axis=-1)                  # the first maximum: the lower axis on a tie


def _pick(p, k):
    return np.take_along_axis(p, k[..., None], -1)[..., 0]


def _o2(p, q, r, ax):
    u, v = (ax + 1) % 3, (ax + 2) % 3
    return (_pick(q, u) - _pick(p, u)) * (_pick(r, v) - _pick(p, v)) - (_pick(q, v) - _pick(p, v)) * (_pick(r, u) - _pick(p, u))


def _same_side(x, y, z):
    return ((x >= 0) & (y >= 0) & (z >= 0)) | ((x <= 0) & (y <= 0) & (z <= 0))


def _in_box(x, p, q, ax):
    ok = np.ones(x.shape[:-1], bool)
    for k in ((ax + 1) % 3, (ax + 2) % 3):
        xs, ps, qs = _pick(x, k), _pick(p, k), _pick(q, k)
        ok &= (np.minimum(ps, qs) <= xs) & (xs <= np.maximum(ps, qs))
    return ok


def _seg_seg(p, q, a, b, ax):
    s1, s2 = np.sign(_o2(p, q, a, ax)), np.sign(_o2(p, q, b, ax))
    s3, s4 = np.sign(_o2(a, b, p, ax)), np.sign(_o2(a, b, q, ax))
    return ((s1 != s2) & (s3 != s4)) | ((s1 == 0) & _in_box(a, p, q, ax)) | ((s2 == 0) & _in_box(b, p, q, ax)) \
        | ((s3 == 0) & _in_box(p, a, b, ax)) | ((s4 == 0) & _in_box(q, a, b, ax))


def seg_tri(p, q, T, n, ax):
    """closed segment pq against closed triangle T [..., 3, 3] with normal n and dropped axis ax"""
    a, b, c = T[..., 0, :], T[..., 1, :], T[..., 2, :]
    sp, sq = np.sign(_dot(n, p - a)), np.sign(_dot(n, q - a))
    general = _same_side(_o3(p, q, a, b), _o3(p, q, b, c), _o3(p, q, c, a))
    inside_p = _same_side(_o2(a, b, p, ax), _o2(b, c, p, ax), _o2(c, a, p, ax))
    inside_q = _same_side(_o2(a, b, q, ax), _o2(b, c, q, ax), _o2(c, a, q, ax))
    coplanar = inside_p | inside_q | _seg_seg(p, q, a, b, ax) | _seg_seg(p, q, b, c, ax) | _seg_seg(p, q, c, a, ax)
    return np.where(sp * sq > 0, False, np.where((sp == 0) & (sq == 0), coplanar, general))


def closed_test(A, B, nA, nB, axA, axB):
    hit = np.zeros(A.shape[:-2], bool)
    for e in range(3):
        hit |= seg_tri(A[..., e, :], A[..., (e + 1) % 3, :], B, nB, axB)
        hit |= seg_tri(B[..., e, :], B[..., (e + 1) % 3, :], A, nA, axA)
    return hit


def _corner(T, k):
    return np.take_along_axis(T, (k % 3)[..., None, None], -2)[..., 0, :]


def verdicts(A, B, same_mesh=True):
    """A, B int64 [P, 3, 3] -> bool [P]: the verdict of every pair (A[p], B[p])"""
    A, B = np.asarray(A, I64).reshape(-1, 3, 3), np.asarray(B, I64).reshape(-1, 3, 3)
    nA, nB = normals(A), normals(B)
    live = nA.any(-1) & nB.any(-1)
    axA, axB = drop_axis(nA), drop_axis(nB)
    closed = closed_test(A, B, nA, nB, axA, axB)
    if not same_mesh:
        return live & closed
    eq = (A[:, :, None, :] == B[:, None, :, :]).all(-1)           # [P, corner of A, corner of B]
    inA, inB = eq.any(2), eq.any(1)
    k = inA.sum(1)
    # one shared point: corner i of A is corner j of B
    i, j = np.argmax(inA, 1), np.argmax(inB, 1)
    one = seg_tri(_corner(A, i + 1), _corner(A, i + 2), B, nB, axB) | seg_tri(_corner(B, j + 1), _corner(B, j + 2), A, nA, axA)
    # a shared edge: corner i of A and corner j of B are the ones left over
    i, j = np.argmin(inA, 1), np.argmin(inB, 1)
    u, w, c, d = _corner(A, i + 1), _corner(A, i + 2), _corner(A, i), _corner(B, j)
    fold = (_o3(u, w, c, d) == 0) & (np.sign(_o2(u, w, c, axA)) == np.sign(_o2(u, w, d, axA)))
    return live & np.where(k == 0, closed, np.where(k == 1, one, np.where(k == 2, fold, True)))


# ---- pairs of a mesh ----------------------------------------------------------------------------------------------------------------
def boxes(tri):
    return tri.min(1), tri.max(1)


def candidates(loA, hiA, loB, hiB):
    """all (i, j) whose closed integer boxes overlap on all three axes: a sweep along x, then y and z.  Two triangles with a
    common point have overlapping boxes, so nothing that a verdict could accept is lost."""
    order = np.argsort(loB[:, 0], kind="stable")
    lx = loB[order, 0]
    out_i, out_j = [], []
    stop = np.searchsorted(lx, hiA[:, 0], side="right")            # B boxes that begin at or before A's end ...
    start = np.searchsorted(lx, loA[:, 0] - (hiB[:, 0] - loB[:, 0]).max(), side="left")    # ... and are wide enough to reach its start
    for a0 in range(0, len(loA), 1024):
        a1 = min(len(loA), a0 + 1024)
        n = np.maximum(stop[a0:a1] - start[a0:a1], 0)
        i = np.repeat(np.arange(a0, a1), n)
        j = order[np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n) + np.repeat(start[a0:a1], n)]   # sorted boxes start[i] .. stop[i]
        keep = ((loA[i] <= hiB[j]) & (loB[j] <= hiA[i])).all(1)
        out_i.append(i[keep])
        out_j.append(j[keep])
    return np.concatenate(out_i), np.concatenate(out_j)


def _verdict_blocks(A, B, same_mesh, step=200_000):
    out = np.zeros(len(A), bool)
    for a in range(0, len(A), step):
        out[a:a + step] = verdicts(A[a:a + step], B[a:a + step], same_mesh)
    return out


def self_pairs(tri, cull=True):
    """snapped triangles [F, 3, 3] -> int64 [P, 2], i < j, in lexicographic order"""
    F = len(tri)
    if cull:
        lo, hi = boxes(tri)
        i, j = candidates(lo, hi, lo, hi)
        keep = i < j
        i, j = i[keep], j[keep]
    else:
        i, j = np.triu_indices(F, 1)
    hit = _verdict_blocks(tri[i], tri[j], True)
    p = np.stack([i[hit], j[hit]], 1).astype(I64)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def between_pairs(triA, triB, cull=True):
    if cull:
        i, j = candidates(*boxes(triA), *boxes(triB))
    else:
        i, j = (g.ravel() for g in np.meshgrid(np.arange(len(triA)), np.arange(len(triB)), indexing="ij"))
    hit = _verdict_blocks(triA[i], triB[j], False)
    p = np.stack([i[hit], j[hit]], 1).astype(I64)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def result(vertices, faces, L, cull=True):
    """what surfd_isect_self must give: dict(pairs int64 [P, 2], count, hits int32 [F], degenerate bool [F])"""
    tri = snap_mesh(vertices, faces, L)
    p = self_pairs(tri, cull)
    hits = (np.bincount(p[:, 0], minlength=len(tri)) + np.bincount(p[:, 1], minlength=len(tri))).astype(np.int32)
    return dict(pairs=p, count=len(p), hits=hits, degenerate=~normals(tri).any(-1))


def result_between(va, fa, vb, fb, L, cull=True):
    ta, tb = snap_mesh(va, fa, L), snap_mesh(vb, fb, L)
    p = between_pairs(ta, tb, cull)
    return dict(pairs=p, count=len(p), hits_a=np.bincount(p[:, 0], minlength=len(ta)).astype(np.int32),
                hits_b=np.bincount(p[:, 1], minlength=len(tb)).astype(np.int32))


# ---- the second form: one pair in Python integers ---------------------------------------------------------------------------------
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross_big(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _o3_big(a, b, c, d):
    n, e = _cross_big(_sub(b, a), _sub(c, a)), _sub(d, a)
    return n[0] * e[0] + n[1] * e[1] + n[2] * e[2]


def _sgn(x):
    return (x > 0) - (x < 0)


def _axis_big(T):
    n = _cross_big(_sub(T[1], T[0]), _sub(T[2], T[0]))
    m = max(abs(x) for x in n)
    return None if m == 0 else [abs(x) for x in n].index(m)


def _flat(p, ax):
    return (p[(ax + 1) % 3], p[(ax + 2) % 3])


def _o2_big(p, q, r):
    return (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])


def _on_segment_big(x, p, q):
    return _o2_big(p, q, x) == 0 and min(p[0], q[0]) <= x[0] <= max(p[0], q[0]) and min(p[1], q[1]) <= x[1] <= max(p[1], q[1])


def _seg_seg_big(p, q, a, b):
    if _on_segment_big(a, p, q) or _on_segment_big(b, p, q) or _on_segment_big(p, a, b) or _on_segment_big(q, a, b):
        return True
    return _sgn(_o2_big(p, q, a)) != _sgn(_o2_big(p, q, b)) and _sgn(_o2_big(a, b, p)) != _sgn(_o2_big(a, b, q))


def _in_tri_big(x, a, b, c):
    s = [_sgn(_o2_big(a, b, x)), _sgn(_o2_big(b, c, x)), _sgn(_o2_big(c, a, x))]
    return min(s) >= 0 or max(s) <= 0


def seg_tri_big(p, q, T):
    a, b, c = T
    sp, sq = _sgn(_o3_big(a, b, c, p)), _sgn(_o3_big(a, b, c, q))
    if sp * sq > 0:
        return False
    if sp == 0 and sq == 0:
        ax = _axis_big(T)
        p, q, a, b, c = (_flat(x, ax) for x in (p, q, a, b, c))
        return _in_tri_big(p, a, b, c) or _in_tri_big(q, a, b, c) or _seg_seg_big(p, q, a, b) or _seg_seg_big(p, q, b, c) \
            or _seg_seg_big(p, q, c, a)
    s = [_sgn(_o3_big(p, q, a, b)), _sgn(_o3_big(p, q, b, c)), _sgn(_o3_big(p, q, c, a))]
    return min(s) >= 0 or max(s) <= 0


def closed_big(A, B):
    return any(seg_tri_big(A[e], A[(e + 1) % 3], B) for e in range(3)) or any(seg_tri_big(B[e], B[(e + 1) % 3], A) for e in range(3))


def verdict_big(A, B, same_mesh=True):
    A = tuple(tuple(int(x) for x in p) for p in A)
    B = tuple(tuple(int(x) for x in p) for p in B)
    if _axis_big(A) is None or _axis_big(B) is None:
        return False
    if not same_mesh:
        return closed_big(A, B)
    shared = [(i, j) for i in range(3) for j in range(3) if A[i] == B[j]]
    if len(shared) == 0:
        return closed_big(A, B)
    if len(shared) == 1:
        i, j = shared[0]
        return seg_tri_big(A[(i + 1) % 3], A[(i + 2) % 3], B) or seg_tri_big(B[(j + 1) % 3], B[(j + 2) % 3], A)
    if len(shared) == 2:
        (i,), (j,) = set(range(3)) - {s[0] for s in shared}, set(range(3)) - {s[1] for s in shared}
        u, w, c, d = A[(i + 1) % 3], A[(i + 2) % 3], A[i], B[j]
        if _o3_big(u, w, c, d) != 0:
            return False
        ax = _axis_big(A)
        u, w, c, d = (_flat(x, ax) for x in (u, w, c, d))
        return _sgn(_o2_big(u, w, c)) == _sgn(_o2_big(u, w, d))
    return True


# ---- case makers ------------------------------------------------------------------------------------------------------------------
LATTICE = 18


def concatenated(a, b):
    (va, fa), (vb, fb) = a, b
    return np.concatenate([va, vb]).astype(F32), np.concatenate([fa, fb + len(va)]).astype(I64)


def shifted(mesh, shift):
    v, f = mesh
    return (v + np.asarray(shift, F32)).astype(F32), f


def two_spheres():
    s = rr.icosphere(2, 0.75)
    return concatenated(s, shifted(s, (0.5, 0.0625, 0.03125)))


def two_cubes():
    c = rr.cube()
    return concatenated(c, shifted(c, (1.0, 0.0, 0.0)))


def interleaved_spheres():
    """the two-spheres mesh with the faces of the two spheres taken in turn (0, 320, 1, 321, ...): intersecting pairs then fall
    inside one tile of 32, across tiles and across chunks of 256"""
    v, f = two_spheres()
    return v, f.reshape(2, -1, 3).transpose(1, 0, 2).reshape(-1, 3)


def torus_with_patch():
    """the 16 896-face torus and a shifted copy of its first 257 faces: 67 chunks of 256"""
    t = rr.torus(96, 88)
    return concatenated(t, shifted((t[0], t[1][:257]), (0.03125, 0.015625, 0.0078125)))


TABLE = {                                                    # name -> (mesh maker, pairs, degenerate faces) at L = 18
    "icosphere2": (lambda: rr.icosphere(2), 0, 0),
    "icosphere3": (lambda: rr.icosphere(3), 0, 0),
    "torus": (rr.torus, 0, 0),
    "cube": (rr.cube, 0, 0),
    "cube_flipped": (rr.cube_flipped, 0, 0),
    "octahedron": (rr.octahedron, 0, 0),
    "wavy_sheet": (rr.wavy_sheet, 0, 0),
    "spliced_sheet": (rr.spliced_sheet, 2, 36),
    "two_spheres": (two_spheres, 88, 0),
    "two_cubes": (two_cubes, 2, 0),
}
