"""Yardstick of the mesh simplification (surfd_amd/meshsimplify.py, csrc/meshsimplify.hip).  Neither the code under test nor its
output: a sequential numpy restatement of vertex clustering with one representative per occupied cell, every elementwise numpy
operation being one IEEE rounding, every sum taken in a stated order.  tests/test_meshsimplify_cpu.py pins it; the device equals
it bit for bit and in the same order.

  simplify          (vertices float64 [V', 3], faces int64 [F', 3], vertex_map int64 [V], counts dict)
  quadric_system    the per-cluster A (six numbers), b, mean and centre that the quadric representative solves: for the checks against
                    numpy.linalg.eigh
  solve_jacobi / solve_eigh     the point of a quadric system through jacobi_f64ops (the contract) / numpy.linalg.eigh (the truth)
  cube_mesh, sphere_mesh, cube_distance         the test meshes of the issue and the distance to the cube's surface
  hand_mesh, order_mesh, edge_triangle, flat_and_parallel_meshes     the hand-made shapes of the CPU tests, shared with the GPU tests

The contract (csrc/meshsimplify.hip carries the same text):
  kept faces   a face that names a vertex with a NaN or an Inf goes; a vertex is REFERENCED when a kept face names it.
  cells        origin = the minimum per axis over the referenced vertices, + 0.0, unless given; k = floor((x - origin) / cell);
               every k in [0, 2^21), else ValueError; key = kx << 42 | ky << 21 | kz.
  clusters     distinct keys ascending, members in ascending vertex index.
  mean         s = 0; s = s + x member by member; mean = s / count.
  quadric      c = origin + (k + 0.5) cell; every (kept face, corner) record in ascending 3 f + corner adds to the cluster of that
               corner: q_i = p_i - c, e1 = q1 - q0, e2 = q2 - q0, n = e1 x e2, l = sqrt((nx nx + ny ny) + nz nz); skipped where
               l == 0; A_ab += (n_a n_b) / l, d = -((nx q0x + ny q0y) + nz q0z), b_a += (n_a d) / l.  Jacobi (six sweeps), lmax by
               strict compares in index order, eigenpairs with lmax > 0 and lambda_j > rank_tol lmax; m = mean - c,
               r_a = -(b_a + ((A_a0 m0 + A_a1 m1) + A_a2 m2)), t_j = ((u_0j r0 + u_1j r1) + u_2j r2) / lambda_j,
               acc_a = acc_a + u_aj t_j in index order, x = m + acc; accepted when finite and |x_a - m_a| <= cell for every a:
               the representative is c + x; otherwise the mean itself, and one fall-back is counted.
  faces        renamed; two equal names: collapsed, dropped; then meshproc.drop_duplicate_faces.
  compaction   clusters no output face names go; the rest keep their order; faces are renumbered.
"""
import numpy as np

from normals_ref import jacobi_f64ops
from surfd_amd import meshproc

KBITS = 21
COUNT_NAMES = ("vertices", "faces", "clusters", "collapsed_faces", "duplicate_faces", "fallbacks")


def _sequential_sums(values, start, count):
    """values [n, d] grouped in runs (start[c], count[c]) -> [C, d]: each run added one by one in its order, from 0.0.  The loop
    runs over the rank within the run and is vectorised across the runs that are that long."""
    C = len(start)
    out = np.zeros((C, values.shape[1]), np.float64)
    if C == 0:
        return out
    order = np.argsort(-count, kind="stable")                  # the longest runs first: the runs still active at a rank are a prefix
    desc = count[order]
    with np.errstate(all="ignore"):
        for r in range(int(desc[0])):
            act = order[:np.searchsorted(-desc, -r, side="left")]      # runs with count > r
            out[act] = out[act] + values[start[act] + r]
    return out


def _clusters(vertices, faces, cell, origin):
    """the part both representatives share: (keep mask of faces, referenced vertices sorted by (key, index), key of each of them,
    run starts, run lengths, cluster of every vertex or -1, origin)"""
    V = len(vertices)
    finite = np.isfinite(vertices).all(axis=1)
    keep = finite[faces].all(axis=1) if len(faces) else np.zeros(0, bool)
    used = np.zeros(V, bool)
    used[faces[keep].ravel()] = True
    ref = np.nonzero(used)[0]
    if origin is None:
        origin = (vertices[ref].min(axis=0) + 0.0) if len(ref) else np.zeros(3)
    origin = np.asarray(origin, np.float64).reshape(3)
    if not np.isfinite(origin).all():
        raise ValueError("the origin must be finite")
    with np.errstate(all="ignore"):
        k = np.floor((vertices[ref] - origin) / cell)
    if len(ref) and not ((k >= 0) & (k < float(1 << KBITS))).all():
        raise ValueError("a cell index falls outside [0, 2^21)")
    ki = k.astype(np.uint64)
    key = (ki[:, 0] << np.uint64(2 * KBITS)) | (ki[:, 1] << np.uint64(KBITS)) | ki[:, 2]
    order = np.argsort(key, kind="stable")                     # ref is ascending: equal keys stay in ascending vertex index
    skey, members = key[order], ref[order]
    head = np.ones(len(skey), bool)
    head[1:] = skey[1:] != skey[:-1]
    start = np.nonzero(head)[0]
    count = np.diff(np.append(start, len(skey)))
    cluster_of = np.full(V, -1, np.int64)
    cluster_of[members] = np.cumsum(head) - 1
    return keep, members, skey[start], k[order][start], start, count, cluster_of, origin


def quadric_system(vertices, faces, cell, origin=None):
    """(A [C, 6] as 00 01 02 11 12 22, b [C, 3], mean [C, 3] absolute, centre [C, 3]) of every cluster, in the contract's order"""
    vertices = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    keep, members, _, kcell, start, count, cluster_of, origin = _clusters(vertices, faces, float(cell), origin)
    return _quadric_system(vertices, faces, float(cell), keep, members, kcell, start, count, cluster_of, origin)


def _quadric_system(vertices, faces, cell, keep, members, kcell, start, count, cluster_of, origin):
    C = len(start)
    with np.errstate(all="ignore"):
        mean = _sequential_sums(vertices[members], start, count) / count[:, None].astype(np.float64)
        centre = origin + (kcell + 0.5) * cell
        kf = np.nonzero(keep)[0]
        rec_face = np.repeat(kf, 3)                                # ascending 3 f + corner
        rec_cluster = cluster_of[faces[kf].ravel()]
        order = np.argsort(rec_cluster, kind="stable")
        rec_face, rec_cluster = rec_face[order], rec_cluster[order]
        c = centre[rec_cluster]
        q0, q1, q2 = vertices[faces[rec_face, 0]] - c, vertices[faces[rec_face, 1]] - c, vertices[faces[rec_face, 2]] - c
        e1, e2 = q1 - q0, q2 - q0
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        l = np.sqrt((nx * nx + ny * ny) + nz * nz)
        d = -((nx * q0[:, 0] + ny * q0[:, 1]) + nz * q0[:, 2])
        terms = np.stack(((nx * nx) / l, (nx * ny) / l, (nx * nz) / l, (ny * ny) / l, (ny * nz) / l, (nz * nz) / l,
                          (nx * d) / l, (ny * d) / l, (nz * d) / l), 1)
        adds = ~(l == 0.0)                                         # nothing is added where l == 0 (a NaN is added)
        terms, rec_cluster = terms[adds], rec_cluster[adds]
        rcount = np.bincount(rec_cluster, minlength=C).astype(np.int64)
        rstart = np.concatenate(([0], np.cumsum(rcount)[:-1])).astype(np.int64) if C else np.zeros(0, np.int64)
        sums = _sequential_sums(terms, rstart, rcount)
    return sums[:, :6], sums[:, 6:], mean, centre


def _matrix(A6):
    M = np.zeros((len(A6), 3, 3), np.float64)
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2] = A6.T
    M[:, 1, 0], M[:, 2, 0], M[:, 2, 1] = M[:, 0, 1], M[:, 0, 2], M[:, 1, 2]
    return M


def solve_jacobi(A6, b, mean, centre, cell, rank_tol=1e-3):
    """the contract's solve: (representative [C, 3], fall-back mask [C])"""
    with np.errstate(all="ignore"):
        m = mean - centre
        a00, a01, a02, a11, a12, a22 = A6.T
        r = np.stack((-(b[:, 0] + ((a00 * m[:, 0] + a01 * m[:, 1]) + a02 * m[:, 2])),
                      -(b[:, 1] + ((a01 * m[:, 0] + a11 * m[:, 1]) + a12 * m[:, 2])),
                      -(b[:, 2] + ((a02 * m[:, 0] + a12 * m[:, 1]) + a22 * m[:, 2]))), 1)
        lam, U, _ = jacobi_f64ops(_matrix(A6))
        lmax = lam[:, 0].copy()
        lmax = np.where(lam[:, 1] > lmax, lam[:, 1], lmax)
        lmax = np.where(lam[:, 2] > lmax, lam[:, 2], lmax)
        cut = rank_tol * lmax
        acc = np.zeros_like(m)
        for j in range(3):
            on = (lmax > 0.0) & (lam[:, j] > cut)
            t = ((U[:, 0, j] * r[:, 0] + U[:, 1, j] * r[:, 1]) + U[:, 2, j] * r[:, 2]) / lam[:, j]
            acc = np.where(on[:, None], acc + U[:, :, j] * t[:, None], acc)
        x = m + acc
        ok = np.isfinite(x).all(axis=1) & (np.abs(x - m) <= cell).all(axis=1)
        rep = np.where(ok[:, None], centre + x, mean)
    return rep, ~ok


def solve_eigh(A6, b, mean, centre, cell, rank_tol=1e-3):
    """the same point through numpy.linalg.eigh: the truth solve_jacobi is measured against (no bit-level claim)"""
    m = mean - centre
    M = _matrix(A6)
    r = -(b + np.einsum("nab,nb->na", M, m))
    lam, U = np.linalg.eigh(M)
    lmax = lam.max(axis=1)
    on = (lmax[:, None] > 0) & (lam > rank_tol * lmax[:, None])
    t = np.where(on, np.einsum("naj,na->nj", U, r) / np.where(on, lam, 1.0), 0.0)
    x = m + np.einsum("naj,nj->na", U, t)
    ok = np.isfinite(x).all(axis=1) & (np.abs(x - m) <= cell).all(axis=1)
    return np.where(ok[:, None], centre + x, mean), ~ok


def simplify(vertices, faces, cell, origin=None, representative="quadric", rank_tol=1e-3):
    vertices = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cell, rank_tol = float(cell), float(rank_tol)
    if not (cell > 0 and np.isfinite(cell)):
        raise ValueError("cell must be positive and finite")
    if not (rank_tol > 0 and np.isfinite(rank_tol)):
        raise ValueError("rank_tol must be positive and finite")
    if representative not in ("mean", "quadric"):
        raise ValueError(representative)
    V = len(vertices)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    if V == 0 or len(faces) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64), np.full(V, -1, np.int64), counts
    if faces.min() < 0 or faces.max() >= V:
        raise ValueError("a face names a vertex outside [0, V)")
    keep, members, _, kcell, start, count, cluster_of, origin = _clusters(vertices, faces, cell, origin)
    C = len(start)
    counts["clusters"] = C
    if representative == "mean":
        with np.errstate(all="ignore"):
            rep = _sequential_sums(vertices[members], start, count) / count[:, None].astype(np.float64)
    else:
        A6, b, mean, centre = _quadric_system(vertices, faces, cell, keep, members, kcell, start, count, cluster_of, origin)
        rep, fell = solve_jacobi(A6, b, mean, centre, cell, rank_tol)
        counts["fallbacks"] = int(fell.sum())
    named = cluster_of[faces[keep]]
    live = (named[:, 0] != named[:, 1]) & (named[:, 1] != named[:, 2]) & (named[:, 0] != named[:, 2])
    counts["collapsed_faces"] = int((~live).sum())
    named = named[live]
    out_faces = meshproc.drop_duplicate_faces(named)
    counts["duplicate_faces"] = len(named) - len(out_faces)
    stays = np.zeros(C, bool)
    stays[out_faces.ravel()] = True
    newid = np.cumsum(stays) - 1
    out_faces = newid[out_faces].reshape(-1, 3)
    vertex_map = np.where((cluster_of >= 0) & stays[np.maximum(cluster_of, 0)], newid[np.maximum(cluster_of, 0)], -1) if C else np.full(V, -1, np.int64)
    out_vertices = rep[stays].reshape(-1, 3)
    counts["vertices"], counts["faces"] = len(out_vertices), len(out_faces)
    return out_vertices, out_faces.astype(np.int64), vertex_map.astype(np.int64), counts


# ---- test meshes ------------------------------------------------------------------------------------------------------------------
def cube_mesh(n=24, side=1.0):
    """the cube [0, side]^3 with n x n quads per face, each split into two triangles, outward winding, shared vertices welded"""
    g = np.arange(n + 1, dtype=np.float64) * (side / n)
    g[-1] = side
    idx = {}
    verts, faces = [], []

    def vid(p):
        if p not in idx:
            idx[p] = len(verts)
            verts.append((g[p[0]], g[p[1]], g[p[2]]))
        return idx[p]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side_i, flip in ((0, True), (n, False)):
            for i in range(n):
                for j in range(n):
                    def at(a, b):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side_i, a, b
                        return vid(tuple(p))
                    q = (at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1))
                    tris = ((q[0], q[1], q[2]), (q[0], q[2], q[3]))
                    for t in tris:
                        faces.append(t[::-1] if flip else t)
    return np.array(verts, np.float64), np.array(faces, np.int64)


def hand_mesh():
    """cell 1, origin 0: cells a = (0,0,0), b = (1,0,0), c = (0,1,0), d = (2,0,0); keys a < c < b < d"""
    nan = float("nan")
    v = np.array([[0.25, 0.25, 0.25], [1.25, 0.25, 0.25], [0.25, 1.25, 0.25],          # 0 a, 1 b, 2 c
                  [0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5],                   # 3 a, 4 b, 5 c
                  [nan, 0.5, 0.5], [5.5, 5.5, 5.5], [-3.0, -3.0, -3.0],                # 6 non-finite, 7 and 8 unreferenced
                  [2.5, 0.5, 0.5], [2.75, 0.5, 0.5]])                                  # 9 d, 10 d
    f = np.array([[0, 1, 2],            # (a, b, c)
                  [5, 4, 3],            # (c, b, a): the same three cells, wound the other way
                  [0, 3, 1],            # two corners in a: collapsed
                  [0, 1, 6],            # names the NaN vertex: not kept
                  [9, 10, 0]])          # two corners in d: collapsed, and d is named by nothing else
    return v, f


def order_mesh(xs):
    """three vertices with the x coordinates xs in the cell (0, 0, 0) of a grid of 4e16 from (-2e16, 0, 0), the other corners of
    their three faces in the cells (0, 1, 0) and (0, 0, 1)"""
    v = np.array([[x, 0.25, 0.25] for x in xs] + [[0.25, 5e16, 0.25], [0.25, 0.25, 5e16]])
    return v, np.array([[0, 3, 4], [1, 3, 4], [2, 3, 4]])


def edge_triangle(x):
    return np.array([[0.5, 0.5, 0.5], [x, 0.5, 0.5], [0.5, 3.5, 0.5]]), np.array([[0, 1, 2]])


def flat_and_parallel_meshes():
    """(a cell whose only own face has no area, two nearly parallel planes whose common line lies far outside the cell)"""
    flat = (np.array([[0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [0.75, 0.75, 0.75], [3.5, 0.5, 0.5], [0.5, 3.5, 0.5]]), np.array([[0, 1, 2], [0, 3, 4]]))
    par = (np.array([[0.5, 0.5, 0.5], [3.5, 0.5, 0.5], [0.5, 3.5, 0.5], [3.5, 0.5, 0.5 + 1e-3], [0.5, 3.5, 0.5 + 2e-3], [0.6, 0.6, 0.9]]),
           np.array([[0, 1, 2], [5, 3, 4]]))
    return flat, par


def cube_distance(points, side=1.0):
    """distance of points to the surface of the cube [0, side]^3"""
    p = np.asarray(points, np.float64)
    outside = np.maximum(np.maximum(-p, p - side), 0.0)
    dout = np.sqrt((outside ** 2).sum(axis=1))
    din = np.minimum(p, side - p).min(axis=1)
    return np.where(dout > 0, dout, np.maximum(din, 0.0))


def sphere_mesh(n_lat=48, n_lon=96, radius=1.0):
    """UV sphere: 2 poles + (n_lat - 1) rings of n_lon vertices (48 x 96: 4 514 vertices, 9 024 faces), outward winding"""
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack((np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n_lon))), 2).reshape(-1, 3)
    verts = np.concatenate(([[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]])) * radius
    faces = []
    south = len(verts) - 1
    for j in range(n_lon):
        faces.append((0, 1 + j, 1 + (j + 1) % n_lon))
    for i in range(n_lat - 2):
        a, b = 1 + i * n_lon, 1 + (i + 1) * n_lon
        for j in range(n_lon):
            j1 = (j + 1) % n_lon
            faces.append((a + j, b + j, b + j1))
            faces.append((a + j, b + j1, a + j1))
    a = 1 + (n_lat - 2) * n_lon
    for j in range(n_lon):
        faces.append((a + j, south, a + (j + 1) % n_lon))
    return verts, np.array(faces, np.int64)


def reference_check():
    """what the restatement reaches on the issue's meshes: the content of profiles/meshsimplify_ref_check.json
    (python tests/meshsimplify_ref.py rewrites the file; tests/test_meshsimplify_cpu.py compares it with a fresh run)"""
    cube, sphere = cube_mesh(24), sphere_mesh()
    corners = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    out = {"what": "tests/meshsimplify_ref.py on the cube of side 1 with 24 x 24 quads per face and the 48 x 96 UV sphere of radius 1: largest "
                   "distance of an output vertex to the surface, per cell size and representative; the largest difference between the "
                   "points of the Jacobi solve of the contract and of numpy.linalg.eigh on the same A, b",
           "cube": {}, "sphere": {}, "jacobi_vs_eigh": {}}
    for cell in (0.071, 0.1, 0.13, 0.21):
        oq, _, _, c = simplify(*cube, cell, representative="quadric")
        om, _, _, _ = simplify(*cube, cell, representative="mean")
        out["cube"][str(cell)] = {"quadric_max_distance": float(cube_distance(oq).max()), "mean_max_distance": float(cube_distance(om).max()),
                                  "quadric_corner_distance": max(float(np.sqrt(((oq - k) ** 2).sum(axis=1)).min()) for k in corners), "counts": c}
    oq, _, _, _ = simplify(*sphere, 0.1, representative="quadric")
    om, _, _, _ = simplify(*sphere, 0.1, representative="mean")
    out["sphere"] = {"cell": 0.1, "quadric_radial_error": float(np.abs(np.sqrt((oq ** 2).sum(axis=1)) - 1.0).max()),
                     "mean_radial_error": float(np.abs(np.sqrt((om ** 2).sum(axis=1)) - 1.0).max())}
    for name, mesh, cells in (("cube", cube, (0.071, 0.1, 0.13, 0.21)), ("sphere", sphere, (0.1, 0.2))):
        worst = 0.0
        for cell in cells:
            A, b, m, c = quadric_system(*mesh, cell)
            worst = max(worst, float(np.abs(solve_jacobi(A, b, m, c, cell)[0] - solve_eigh(A, b, m, c, cell)[0]).max()))
        out["jacobi_vs_eigh"][name] = worst
    return out


if __name__ == "__main__":
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "meshsimplify_ref_check.json")
    with open(path, "w") as fh:
        json.dump(reference_check(), fh, indent=1)
        fh.write("\n")
    print(path)
