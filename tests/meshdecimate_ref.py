"""Yardstick of the edge-collapse decimation (surfd_amd/meshsimplify.py: simplify_quadric_decimation, csrc/meshdecimate.hip).
Neither the code under test nor its output: a sequential numpy restatement of quadric decimation to a target face count by ROUNDS
OF INDEPENDENT COLLAPSES, every elementwise numpy operation being one IEEE rounding, every sum taken in a stated order.
tests/test_meshdecimate_cpu.py pins it; the device equals it bit for bit and in the same order.

  decimate          (vertices float64 [V', 3], faces int64 [F', 3], vertex_map int64 [V], counts dict)
  mix64             the integer finaliser behind the tie order and the priorities
  icosphere, sheet_mesh, torus_mesh, tetrahedron, octahedron, cube12, two_spheres      the test meshes
  reference_check   what the restatement reaches: the content of profiles/meshdecimate_ref_check.json

The contract (csrc/meshdecimate.hip carries the same text).  Input: vertices fp64 [V, 3], faces [F, 3], target_faces >= 0 and the
knobs border_weight >= 0, 0 <= flip_cos < 1, rank_tol > 0 (all finite), spread >= 1, max_rounds >= 1, seed (64 bits).
  kept faces   a face goes if it names a vertex with a NaN or an Inf or names one vertex twice.  An index outside [0, V) is an error.
               A vertex TAKES PART when a kept face names it.  Faces keep their order; a vertex keeps its index until the end.
  centre       lo, hi = the minimum and maximum per axis over the vertices that take part, each + 0.0; c0 = 0.5 lo + 0.5 hi
               (0 without such a vertex).  P_v = x_v - c0 for every vertex; all arithmetic below is on P.
  quadrics     per vertex (A as 00 01 02 11 12 22, b 3, c 1), from 0.0, one addition per term:
               face terms, for the faces at the vertex in ascending 3 f + corner: q_i = P of the corners (corner 0 first),
                 e1 = q1 - q0, e2 = q2 - q0, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x),
                 l = sqrt((nx nx + ny ny) + nz nz); nothing where l == 0; d = -((nx q0x + ny q0y) + nz q0z);
                 A_ab += (n_a n_b) / l, b_a += (n_a d) / l, c += (d d) / l.
               then border terms, for the border half-edges h = 3 f + k (from corner k to corner (k + 1) % 3, the unordered pair
                 occurring once among the kept faces) that end at the vertex, in ascending h: t = P_to - P_from, n and l of the
                 face as above, m = (ty nz - tz ny, tz nx - tx nz, tx ny - ty nx), mm = (mx mx + my my) + mz mz; nothing where
                 mm == 0; s = (border_weight l) / mm; d = -((mx qx + my qy) + mz qz) with q = P_from;
                 A_ab += (m_a m_b) s, b_a += (m_a d) s, c += (d d) s.  (The unit plane through the edge, perpendicular to the face,
                 weighted by twice the face's area and border_weight: the customary form.)
  ROUND r = 0, 1, ... while F_now > target and r < max_rounds, from the current faces:
  1 edges      half-edge h = 3 f + k names (min, max) of its two corners; the unique pairs (lo < hi) ascending are the edges, the
               number of half-edges of a pair is its valence.  deg(v): the edges at v; N(v): its neighbours; a vertex is a BORDER
               vertex when a valence-1 edge meets it.
  2 placement  Q = Q_lo + Q_hi (lo first, entry by entry).  m = (P_lo + P_hi) 0.5.  r_a = -(b_a + ((A_a0 m0 + A_a1 m1) + A_a2 m2)).
               A is decomposed by the six cyclic Jacobi sweeps of tests/normals_ref.py: jacobi_f64ops; lmax = l0, then l1 and l2
               each taken where greater; acc = 0; for j = 0, 1, 2 with lmax > 0 and lambda_j > rank_tol lmax:
               t = ((u_0j r0 + u_1j r1) + u_2j r2) / lambda_j, acc_a = acc_a + u_aj t.  x = m + acc.
               box: mn_a = min(P_lo a, P_hi a), mx_a likewise, ext = the largest mx_a - mn_a.  x is accepted when it is finite
               and mn_a - ext <= x_a <= mx_a + ext for every a.  Otherwise the point is m, then P_lo where its cost is strictly
               smaller, then P_hi where its cost is strictly smaller than the best so far.
               cost(p): g_a = (A_a0 p0 + A_a1 p1) + A_a2 p2; k = ((p0 g0 + p1 g1) + p2 g2 + 2.0 ((b0 p0 + b1 p1) + b2 p2)) + c;
               cost = k where k > 0 or k is a NaN, else 0.0.
  3 validity   the FIRST rule that refuses an edge is counted for it:
               (a) valence 1 or 2;  (b) |N(lo) & N(hi)| == valence;  (c) not (valence 2 and lo and hi both border vertices);
               (d) every opposite vertex o (the third corner of a face at the edge): deg(o) >= 4 where o is no border vertex,
                   deg(o) >= 3 where it is one (a lone triangle does not vanish);
               (n) the cost is no NaN;
               (e) for every face at lo or at hi that does not hold both, with corners q0 q1 q2 and the moved corner replaced
                   by the point in q': n = (q1 - q0) x (q2 - q0), n' likewise (components as above), g = (nx n'x + ny n'y) + nz n'z,
                   nn = (nx nx + ny ny) + nz nz, n'n' likewise: g > 0 and g g > flip_cos2 (nn n'n'), flip_cos2 = flip_cos flip_cos;
                     and the same two comparisons with n0 in the place of n, the normal the face had in the input (over P; a face
                     of a round is one input face renamed, so n0 travels with it): the turns of many rounds do not add up, and a
                     sliver does not come to lie on its side.
  4 candidates key = bits(fp32(cost)) << 32 | (mix64(seed, r, lo, hi) & 0xffffffff) for a valid edge (an fp32 below the smallest
               normal number counts as 0), all ones for an invalid one.  Stable sort by key (ties to the lower edge).
               remaining = ceil((F_now - target) / 2).  The candidates are the first min(valid, spread remaining) edges.
  5 selection  priority of a candidate = (mix64(seed, r, lo, hi), edge), compared in that order: independent of the cost.
               m(v) = the least priority of the candidates at v; M(v) = the least m over v and N(v).  A candidate is selected iff
               its priority is M(lo) and M(hi).  If e = (a, b) and e' = (c, d) are selected and a is c or a neighbour of c, then
               M(a) <= m(c) <= prio(e') and M(c) <= m(a) <= prio(e), so e = e': the end points of two selected edges are distinct
               and not adjacent.  No face then holds an end point of each, so their face fans are disjoint; N(a) & N(b), the
               valence, the border flags at a and b and every face of e's fan are what they were after e' is applied, so
               rules (a), (b), (c), (e) still hold; an opposite vertex of k selected edges has them in its link cycle, pairwise
               non-adjacent, so its degree n >= 3 k leaves n - k >= 3 (rule (d) covers k = 1).  Applying the selected edges in
               any order is applying them at once.  If more than `remaining` are selected, those of lowest sort rank stay.
  6 apply      hi is renamed lo, P_lo = the point, Q_lo = Q_lo + Q_hi.  Faces are renamed; one with two equal names goes; the
               rest keep their order.  vertex_map is composed one hop (a survivor of a round was not collapsed in it).
  end          stop: 0 F_now <= target, 1 a round selected nothing (stalled), 2 max_rounds rounds were made.
               Output vertices: those the final faces name, in ascending input index; one that never moved is the input vertex
               itself, a moved one is c0 + P.  vertex_map: the output vertex that an input vertex ended in, -1 where it took no
               part (or its survivor is named by no face).  counts: COUNT_NAMES; the refusals are those of the last round made.
"""
import numpy as np

from meshsimplify_ref import _matrix, _sequential_sums
from normals_ref import jacobi_f64ops

COUNT_NAMES = ("vertices", "faces", "rounds", "collapses", "border_collapses", "stop", "refused_valence", "refused_link",
               "refused_border", "refused_opposite", "refused_flip", "refused_nan")
STOP_NAMES = ("target", "stalled", "max_rounds")
M64 = (1 << 64) - 1
_FLT_MIN = np.float32(1.17549435e-38)


def _fin(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xbf58476d1ce4e5b9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def mix64(seed, rnd, lo, hi):
    """fin(fin(seed + 0x9e3779b97f4a7c15 (round + 1)) ^ (lo << 32 | hi)) in 64-bit wrapping arithmetic, fin = splitmix64's finaliser
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31"""
    with np.errstate(over="ignore"):
        a = _fin(np.uint64((int(seed) + 0x9e3779b97f4a7c15 * (int(rnd) + 1)) & M64))
        return _fin(a ^ ((np.asarray(lo).astype(np.uint64) << np.uint64(32)) | np.asarray(hi).astype(np.uint64)))


def _expand(start, count):
    """(owner, flat index) of every item of the runs (start[i], count[i]), owners ascending, items in run order"""
    owner = np.repeat(np.arange(len(start)), count)
    first = np.cumsum(count) - count
    return owner, start[owner] + (np.arange(len(owner)) - first[owner])


def _normal(q0, q1, q2):
    e1, e2 = q1 - q0, q2 - q0
    return np.stack((e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), 1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cost(Q, p):
    a00, a01, a02, a11, a12, a22, b0, b1, b2, c = Q.T
    g0 = (a00 * p[:, 0] + a01 * p[:, 1]) + a02 * p[:, 2]
    g1 = (a01 * p[:, 0] + a11 * p[:, 1]) + a12 * p[:, 2]
    g2 = (a02 * p[:, 0] + a12 * p[:, 1]) + a22 * p[:, 2]
    k = (((p[:, 0] * g0 + p[:, 1] * g1) + p[:, 2] * g2) + 2.0 * ((b0 * p[:, 0] + b1 * p[:, 1]) + b2 * p[:, 2])) + c
    return np.where((k > 0.0) | np.isnan(k), k, 0.0)


def _edges(fa):
    """(elo, ehi, valence, edge of every half-edge)"""
    a, b = fa.ravel(), fa[:, [1, 2, 0]].ravel()
    key = (np.minimum(a, b).astype(np.uint64) << np.uint64(32)) | np.maximum(a, b).astype(np.uint64)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    head = np.ones(len(skey), bool)
    head[1:] = skey[1:] != skey[:-1]
    start = np.nonzero(head)[0]
    eoh = np.empty(len(key), np.int64)
    eoh[order] = np.cumsum(head) - 1
    return (skey[start] >> np.uint64(32)).astype(np.int64), (skey[start] & np.uint64(0xffffffff)).astype(np.int64), \
        np.diff(np.append(start, len(skey))), eoh


def initial_quadrics(P, fa, border_weight):
    """[V, 10] from the kept faces fa (int64 [F, 3]) over the centred vertices P"""
    V, F = len(P), len(fa)
    q0, q1, q2 = P[fa[:, 0]], P[fa[:, 1]], P[fa[:, 2]]
    n = _normal(q0, q1, q2)
    l = np.sqrt(_dot(n, n))
    d = -_dot(n, q0)
    ft = np.stack([(n[:, a] * n[:, b]) / l for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))] +
                  [(n[:, a] * d) / l for a in range(3)] + [(d * d) / l], 1)
    fon = ~(l == 0.0)
    rec_v = [fa[fon].ravel()]
    rec_cls = [np.zeros(3 * int(fon.sum()), np.int64)]
    rec_idx = [(3 * np.nonzero(fon)[0][:, None] + np.arange(3)).ravel()]
    rec_t = [np.repeat(ft[fon], 3, axis=0)]
    _, _, val, eoh = _edges(fa)
    hb = np.nonzero(val[eoh] == 1)[0]                           # border half-edges, ascending
    f, k = hb // 3, hb % 3
    frm, to = fa[f, k], fa[f, (k + 1) % 3]
    t = P[to] - P[frm]
    nf, lf = n[f], l[f]
    m = np.stack((t[:, 1] * nf[:, 2] - t[:, 2] * nf[:, 1], t[:, 2] * nf[:, 0] - t[:, 0] * nf[:, 2], t[:, 0] * nf[:, 1] - t[:, 1] * nf[:, 0]), 1)
    mm = _dot(m, m)
    s = (border_weight * lf) / mm
    db = -_dot(m, P[frm])
    bt = np.stack([(m[:, a] * m[:, b]) * s for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))] +
                  [(m[:, a] * db) * s for a in range(3)] + [(db * db) * s], 1)
    bon = ~(mm == 0.0)
    for end in (frm, to):
        rec_v.append(end[bon]); rec_cls.append(np.ones(int(bon.sum()), np.int64)); rec_idx.append(hb[bon]); rec_t.append(bt[bon])
    rec_v, rec_cls, rec_idx, rec_t = np.concatenate(rec_v), np.concatenate(rec_cls), np.concatenate(rec_idx), np.concatenate(rec_t)
    order = np.lexsort((rec_idx, rec_cls, rec_v))
    cnt = np.bincount(rec_v, minlength=V).astype(np.int64)
    return _sequential_sums(rec_t[order], np.cumsum(cnt) - cnt, cnt)


def placement(Q, Plo, Phi, rank_tol):
    """(point [E, 3], cost [E]) of rule 2"""
    a00, a01, a02, a11, a12, a22, b0, b1, b2, _ = Q.T
    m = (Plo + Phi) * 0.5
    r = np.stack((-(b0 + ((a00 * m[:, 0] + a01 * m[:, 1]) + a02 * m[:, 2])), -(b1 + ((a01 * m[:, 0] + a11 * m[:, 1]) + a12 * m[:, 2])),
                  -(b2 + ((a02 * m[:, 0] + a12 * m[:, 1]) + a22 * m[:, 2]))), 1)
    lam, U, _ = jacobi_f64ops(_matrix(Q[:, :6]))
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
    mn, mx = np.minimum(Plo, Phi), np.maximum(Plo, Phi)
    ext = (mx - mn).max(axis=1)[:, None]
    ok = np.isfinite(x).all(axis=1) & ((x >= mn - ext) & (x <= mx + ext)).all(axis=1)
    p, cost = m.copy(), _cost(Q, m)
    for q in (Plo, Phi):
        c = _cost(Q, q)
        better = c < cost
        p, cost = np.where(better[:, None], q, p), np.where(better, c, cost)
    cx = _cost(Q, x)
    return np.where(ok[:, None], x, p), np.where(ok, cx, cost)


def decimate(vertices, faces, target_faces, border_weight=1000.0, flip_cos=0.2, rank_tol=1e-3, spread=4, max_rounds=512, seed=0, trace=None):
    vertices = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    target, spread, max_rounds = int(target_faces), int(spread), int(max_rounds)
    border_weight, flip_cos, rank_tol = float(border_weight), float(flip_cos), float(rank_tol)
    if target < 0 or spread < 1 or max_rounds < 1:
        raise ValueError("target_faces >= 0, spread >= 1 and max_rounds >= 1 are required")
    if not (np.isfinite(border_weight) and border_weight >= 0 and 0 <= flip_cos < 1 and np.isfinite(rank_tol) and rank_tol > 0):
        raise ValueError("border_weight >= 0, 0 <= flip_cos < 1 and rank_tol > 0, all finite, are required")
    V = len(vertices)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    if V == 0 or len(faces) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64), np.full(V, -1, np.int64), counts
    if faces.min() < 0 or faces.max() >= V:
        raise ValueError("a face names a vertex outside [0, V)")
    finite = np.isfinite(vertices).all(axis=1)
    keep = finite[faces].all(axis=1) & (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    fa = faces[keep]
    part = np.zeros(V, bool)
    part[fa.ravel()] = True
    flip2 = flip_cos * flip_cos
    with np.errstate(all="ignore"):
        if part.any():
            c0 = 0.5 * (vertices[part].min(axis=0) + 0.0) + 0.5 * (vertices[part].max(axis=0) + 0.0)
        else:
            c0 = np.zeros(3)
        P = vertices - c0
        Q = initial_quadrics(P, fa, border_weight) if len(fa) else np.zeros((V, 10))
        Nref = _normal(P[fa[:, 0]], P[fa[:, 1]], P[fa[:, 2]])
    moved = np.zeros(V, bool)
    vmap = np.arange(V)
    rnd, stop = 0, 0
    while len(fa) > target:
        if rnd >= max_rounds:
            stop = 2
            break
        Fn = len(fa)
        with np.errstate(all="ignore"):
            elo, ehi, val, eoh = _edges(fa)
            E = len(elo)
            deg = np.bincount(elo, minlength=V) + np.bincount(ehi, minlength=V)
            border = np.zeros(V, bool)
            border[elo[val == 1]] = True
            border[ehi[val == 1]] = True
            Qe = Q[elo] + Q[ehi]
            p, cost = placement(Qe, P[elo], P[ehi], rank_tol)
            # (b) the neighbours of lo that are neighbours of hi
            du, dw = np.concatenate((elo, ehi)), np.concatenate((ehi, elo))
            adj = np.sort(du * V + dw)
            order = np.argsort(du, kind="stable")
            nstart = np.cumsum(deg) - deg
            own, at = _expand(nstart[elo], deg[elo])
            probe = dw[order][at] * V + ehi[own]
            pos = np.minimum(np.searchsorted(adj, probe), len(adj) - 1)
            common = np.bincount(own[adj[pos] == probe], minlength=E)
            # (d) opposite vertices
            opp = fa[:, [2, 0, 1]].ravel()
            bad_d = np.bincount(eoh[np.where(border[opp], deg[opp] < 3, deg[opp] < 4)], minlength=E) > 0
            # (e) flips: the corners of every vertex, ascending
            corner = np.argsort(fa.ravel(), kind="stable")
            ccount = np.bincount(fa.ravel(), minlength=V)
            cstart = np.cumsum(ccount) - ccount
            bad_e = np.zeros(E, bool)
            for end, other in ((elo, ehi), (ehi, elo)):
                own, at = _expand(cstart[end], ccount[end])
                h = corner[at]
                f, k = h // 3, h % 3
                sel = ~(fa[f] == other[own][:, None]).any(axis=1)
                own, f, k = own[sel], f[sel], k[sel]
                q = P[fa[f]]                                    # [n, 3 corners, 3]
                qn = q.copy()
                qn[np.arange(len(f)), k] = p[own]
                n0, n1 = _normal(q[:, 0], q[:, 1], q[:, 2]), _normal(qn[:, 0], qn[:, 1], qn[:, 2])
                g, w1 = _dot(n0, n1), _dot(n1, n1)
                fine = (g > 0.0) & (g * g > flip2 * (_dot(n0, n0) * w1))
                nr = Nref[f]
                g = _dot(nr, n1)
                fine &= (g > 0.0) & (g * g > flip2 * (_dot(nr, nr) * w1))
                bad_e |= np.bincount(own[~fine], minlength=E) > 0
            rules = np.stack((~((val == 1) | (val == 2)), common != val, (val == 2) & border[elo] & border[ehi], bad_d, np.isnan(cost), bad_e), 1)
            valid = ~rules.any(axis=1)
            first = np.argmax(rules, axis=1)[~valid]
            refused = np.bincount(first, minlength=6)
            for name, i in (("refused_valence", 0), ("refused_link", 1), ("refused_border", 2), ("refused_opposite", 3), ("refused_nan", 4),
                            ("refused_flip", 5)):
                counts[name] = int(refused[i])
            # candidates
            hsh = mix64(seed, rnd, elo, ehi)
            c32 = cost.astype(np.float32)
            c32 = np.where(c32 < _FLT_MIN, np.float32(0.0), c32)
            key = (c32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (hsh & np.uint64(0xffffffff))
            key = np.where(valid, key, np.uint64(M64))
            rank_order = np.argsort(key, kind="stable")
            remaining = (Fn - target + 1) // 2
            ncand = min(int(valid.sum()), spread * remaining)
            cand = rank_order[:ncand]
            # selection: prio as one integer rank over (hash, edge)
            pr = np.full(E, E, np.int64)
            pr[cand[np.lexsort((cand, hsh[cand]))]] = np.arange(ncand)
            m = np.full(V, E, np.int64)
            np.minimum.at(m, elo[cand], pr[cand])
            np.minimum.at(m, ehi[cand], pr[cand])
            M = m.copy()
            np.minimum.at(M, elo, m[ehi])
            np.minimum.at(M, ehi, m[elo])
            independent = cand[(pr[cand] == M[elo[cand]]) & (pr[cand] == M[ehi[cand]])]             # cand is in sort rank
            chosen = independent[:remaining]
        rnd += 1
        if trace is not None:
            trace.append(dict(faces=Fn, edges=E, valid=int(valid.sum()), candidates=ncand, selected=len(chosen), chosen=chosen.copy(), independent=independent.copy(), key=key, hash=hsh, valence=val,
                              elo=elo, ehi=ehi, cost=cost, rules=rules, rank_order=rank_order))
        if len(chosen) == 0:
            stop = 1
            break
        lo, hi = elo[chosen], ehi[chosen]
        rename = np.arange(V)
        rename[hi] = lo
        P[lo] = p[chosen]
        moved[lo] = True
        Q[lo] = Qe[chosen]
        counts["collapses"] += len(chosen)
        counts["border_collapses"] += int((val[chosen] == 1).sum())
        fa = rename[fa]
        live = (fa[:, 0] != fa[:, 1]) & (fa[:, 1] != fa[:, 2]) & (fa[:, 0] != fa[:, 2])
        fa, Nref = fa[live], Nref[live]
        vmap = rename[vmap]
    stays = np.zeros(V, bool)
    stays[fa.ravel()] = True
    newid = np.cumsum(stays) - 1
    with np.errstate(all="ignore"):
        out_v = np.where(moved[:, None], c0 + P, vertices)[stays].reshape(-1, 3)
    vertex_map = np.where(part & stays[vmap], newid[vmap], -1)
    counts.update(vertices=len(out_v), faces=len(fa), rounds=rnd, stop=stop)
    return out_v, newid[fa].reshape(-1, 3).astype(np.int64), vertex_map.astype(np.int64), counts


# ---- test meshes ------------------------------------------------------------------------------------------------------------------
def tetrahedron():
    return np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]), np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def octahedron():
    v = np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    return v, f


def cube12():
    v = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    return v, f


def icosphere(level=3, radius=1.0):
    """20 4^level faces (level 3: 1 280 faces, 642 vertices), outward winding"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.sqrt(1 + t * t) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.sqrt((p * p).sum()))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius, np.array(f, np.int64)


def sheet_mesh(nx=17, ny=17, dx=1.0, dy=1.0, bump=0.0):
    """nx x ny quads in the plane z = bump sin(x) sin(y), two triangles each, normals along +z: 2 nx ny faces"""
    x, y = np.meshgrid(np.arange(nx + 1) * dx, np.arange(ny + 1) * dy, indexing="ij")
    v = np.stack((x, y, bump * np.sin(x) * np.sin(y)), 2).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a = (i * (ny + 1) + j).ravel()
    b, c, d = a + (ny + 1), a + (ny + 1) + 1, a + 1
    return v, np.stack((np.stack((a, b, c), 1), np.stack((a, c, d), 1)), 1).reshape(-1, 3)


def torus_mesh(nu=24, nv=12, R=1.0, r=0.35):
    u, w = np.meshgrid(2 * np.pi * np.arange(nu) / nu, 2 * np.pi * np.arange(nv) / nv, indexing="ij")
    v = np.stack(((R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)), 2).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a = (i * nv + j).ravel()
    b, c, d = (((i + 1) % nu) * nv + j).ravel(), (((i + 1) % nu) * nv + (j + 1) % nv).ravel(), (i * nv + (j + 1) % nv).ravel()
    return v, np.stack((np.stack((a, b, c), 1), np.stack((a, c, d), 1)), 1).reshape(-1, 3)


def two_spheres(level=1):
    v, f = icosphere(level)
    return np.concatenate((v, v + [3.0, 0, 0])), np.concatenate((f, f + len(v)))


def rule_meshes():
    """name -> (vertices, faces, the edge (lo, hi) that the rule of that name refuses first), each of at most 12 faces"""
    ang = np.arange(6) * np.pi / 3
    rad = np.array([2, .5, 2, .5, 2, .5])
    star = np.concatenate((np.stack((rad * np.cos(ang), rad * np.sin(ang), 0 * ang), 1), [[0, 0, 0.]]))
    return {
        # three faces on one edge
        "refused_valence": (np.array([[0, 0, 0], [1, 0, 0], [.5, 1, 0], [.5, -1, 0], [.5, 0, 1.]]), np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]]), (0, 1)),
        # a ring of six faces around a triangular hole: 0, 1, 2 are pairwise neighbours and (0, 1, 2) is no face
        "refused_link": (np.array([[0, 0, 0], [1, 0, 0], [.5, 1, 0], [.5, -1, 0], [2, 1, 0], [-1, 1, 0.]]),
                         np.array([[0, 3, 1], [1, 4, 2], [2, 5, 0], [1, 3, 4], [2, 4, 5], [0, 5, 3]]), (0, 1)),
        # two faces: the inner edge joins two border vertices
        "refused_border": (np.array([[0, 0, 0], [1, 0, 0], [.5, 1, 0], [.5, -1, 0.]]), np.array([[0, 1, 2], [1, 0, 3]]), (0, 1)),
        "refused_opposite": tetrahedron() + ((0, 1),),
        # a star of six faces around vertex 6: moved to a tip, the faces across turn over
        "refused_flip": (star, np.array([(6, i, (i + 1) % 6) for i in range(6)]), (0, 6)),
    }


def sheet_border_distance(points, nx, ny):
    """distance of points (taken as border vertices of the flat nx x ny sheet) from the four lines of the rectangle"""
    p = np.asarray(points, np.float64)
    d = np.minimum(np.minimum(np.abs(p[:, 0]), np.abs(p[:, 0] - nx)), np.minimum(np.abs(p[:, 1]), np.abs(p[:, 1] - ny)))
    return np.sqrt(d * d + p[:, 2] * p[:, 2])


def border_vertices(faces):
    elo, ehi, val, _ = _edges(np.asarray(faces, np.int64))
    return np.unique(np.concatenate((elo[val == 1], ehi[val == 1])))


def reference_check():
    """what the restatement reaches on the issue's meshes: the content of profiles/meshdecimate_ref_check.json
    (python tests/meshdecimate_ref.py rewrites the file; tests/test_meshdecimate_cpu.py compares it with a fresh run)"""
    import meshsimplify_ref as MS
    out = {"what": "tests/meshdecimate_ref.py with its default knobs: the cube of side 1 with 24 x 24 quads per face to 10 % of its faces "
                   "(largest distance of an output vertex from the surface), the flat 17 x 17 sheet to 25 % (largest distance of an output "
                   "border vertex from the rectangle's four lines), the 48 x 96 UV sphere to the face count that clustering with cell 0.1 "
                   "gives (largest radial error of both; recorded, not asserted)"}
    cv, cf = MS.cube_mesh(24)
    ov, of, _, c = decimate(cv, cf, len(cf) // 10)
    out["cube"] = {"target": len(cf) // 10, "max_distance": float(MS.cube_distance(ov).max()), "counts": c}
    sv, sf = sheet_mesh(17, 17)
    ov, of, _, c = decimate(sv, sf, len(sf) // 4)
    out["sheet"] = {"target": len(sf) // 4, "border_max_distance": float(sheet_border_distance(ov[border_vertices(of)], 17, 17).max()), "counts": c}
    pv, pf = MS.sphere_mesh()
    kv, kf, _, _ = MS.simplify(pv, pf, 0.1)
    ov, of, _, c = decimate(pv, pf, len(kf))
    out["sphere"] = {"target": len(kf), "decimation_radial_error": float(np.abs(np.sqrt((ov ** 2).sum(axis=1)) - 1.0).max()),
                     "clustering_radial_error": float(np.abs(np.sqrt((kv ** 2).sum(axis=1)) - 1.0).max()), "counts": c}
    return out


if __name__ == "__main__":
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "meshdecimate_ref_check.json")
    with open(path, "w") as fh:
        json.dump(reference_check(), fh, indent=1)
        fh.write("\n")
    print(path)
