"""Yardstick of the isotropic remeshing (surfd_amd/meshremesh.py: remesh_isotropic, csrc/meshremesh.hip).
Neither the code under test nor its output: a sequential numpy restatement of incremental isotropic remeshing (Botsch and Kobbelt
2004) to a target edge length as ROUNDS OF INDEPENDENT OPERATIONS, every elementwise numpy operation being one IEEE rounding, every
sum taken in a stated order.  tests/test_meshremesh_cpu.py pins it; the device equals it bit for bit and in the same order.

  Remesher          the state and one iteration (the handle of the library)
  remesh            (vertices float64 [V', 3], faces int64 [F', 3], origin int64 [V'], list of per-iteration counts)
  reference_check   what the restatement reaches: the content of profiles/meshremesh_ref_check.json
  triangle_quality  numpy twin of surfd_amd.meshremesh.triangle_quality (outside the contract)

The contract (csrc/meshremesh.hip carries the same text).  Input: vertices fp64 [V, 3], faces [F, 3], low2 = (low L)^2 and
high2 = (high L)^2 made once by the caller in fp64 (0 < low2 < high2, finite), 0 <= flip_cos < 1, seed (64 bits).
len2(p, q): d = q - p, (dx dx + dy dy) + dz dz.  normal(q0, q1, q2) and dot: e1 = q1 - q0, e2 = q2 - q0,
n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x); (ax bx + ay by) + az bz.
  kept faces   a face goes if it names a vertex with a NaN or an Inf or names one vertex twice.  An index outside [0, V) is an error.
  state        X (a vertex keeps its index for the life of the handle; new vertices are appended), the faces, n0 per face (the
               normal of the input face, which children and flipped pairs inherit), origin per vertex (its input index while it is
               an input vertex at its input position, else -1), tick (numbers every collapse and flip round made: mix64's round).
  structure    rebuilt at the start of every round: half-edge h = 3 f + k names (min, max) of corners k and (k + 1) % 3; the unique
               pairs (lo < hi) ascending are the edges, the half-edges of an edge in ascending h, their number its valence.
               deg(v): the edges at v; N(v): its neighbours ascending; corners of v: the h that name v, ascending; a vertex is
               a BORDER vertex when a valence-1 edge meets it; it TAKES PART when a face names it.
  ITERATION = A, B, C, D.  A round that is looked at counts as made, the one that finds nothing included; a stage ends with it.
  A split      up to split_rounds rounds.  An edge is marked iff len2(x_lo, x_hi) > high2.  The marked edges in ascending edge
               order get the vertices V_now, V_now + 1, ... at (x_lo + x_hi) 0.5, origin -1.  A face with k marked half-edges is
               replaced by 1 + k faces at the exclusive sum of 1 + k, each with the parent's n0; c_i its corners, m_i the new
               vertex of half-edge i:  k = 0 the face;  k = 1 (i marked): (c_i, m_i, c_i+2), (m_i, c_i+1, c_i+2);
               k = 3: (c0, m0, m2), (m0, c1, m1), (m2, m1, c2), (m0, m1, m2);  k = 2 (j unmarked; a = c_j, b = c_j+1, c = c_j+2,
               m1 = m_j+1, m2 = m_j+2): (m1, c, m2), then where len2(x_a, x_m1) < len2(x_b, x_m2), or they are equal and a < b:
               (a, b, m1), (a, m1, m2); else (a, b, m2), (b, m1, m2).  3 F' >= 2^31 or V' >= 2^31: refused, the state unchanged.
  B collapse   up to collapse_rounds rounds, rnd = tick, tick += 1.  Only edges with len2(x_lo, x_hi) < low2 are looked at; the
               FIRST rule that refuses one is counted:
               (a) valence 1 or 2;  (b) |N(lo) & N(hi)| == valence;  (c) not (valence 2 and lo and hi both border vertices);
               (d) every opposite vertex o: deg(o) >= 4, or >= 3 at a border vertex;
               the point: (x_lo + x_hi) 0.5 where both or neither end is a border vertex, else the border end's own bits;
               (f) for every w of N(lo), then of N(hi), other than lo and hi: len2(x_w, point) <= high2;
               (e) for every face at lo or at hi that does not hold both, the moved corner replaced by the point: with n the
                   standing normal, n' the new one: g = dot(n, n'), g > 0 and g g > flip_cos2 (dot(n, n) dot(n', n')); and the
                   same with the face's n0 in the place of n.
               priority = (mix64(seed, rnd, lo, hi), edge); m(v) = the least priority of the valid edges at v; M(v) = the least m
               over v and N(v); an edge is selected iff its priority is M(lo) and M(hi).  (tests/meshdecimate_ref.py gives the
               argument: selected edges have distinct, non-adjacent end points, so they are applied at once.  Rule (f) looks at
               positions of N(lo) | N(hi) only, none of which another selected collapse moves: its end points are no neighbours.)
               apply: hi is renamed lo, x_lo = the point, origin[lo] = -1 unless the point has x_lo's bits; faces with two equal
               names go, the rest keep their order and n0.
  C flip       up to flip_rounds rounds, rnd = tick, tick += 1.  Only valence-2 edges are looked at; a = lo, b = hi.  With its
               two half-edges in ascending h: one whose two half-edges both leave a or both leave b is refused (orient).  f1
               holds a -> b, c its third corner; f2 holds b -> a, d its third corner.  t(v) = 4 at a border vertex, else 6;
               an edge goes on iff the sum of (deg - t)^2 over a, b, c, d gets strictly smaller with deg(a) - 1, deg(b) - 1,
               deg(c) + 1, deg(d) + 1 (c and d as they are, equal or not).  Then the first refusing rule is counted:
               (same) c != d;  (edge) d not in N(c);  (degree) deg(a) and deg(b) >= 4, or >= 3 at a border vertex;
               (long) len2(x_c, x_d) <= high2;  (fold) w = normal(c, a, d), then normal(d, b, c): against n = the standing normal
               of f1, then of f2, then n0' = n0_f1 + n0_f2: g = dot(n, w), g > 0 and g g > flip_cos2 (dot(n, n) dot(w, w))
               (a zero w fails g > 0).
               key = (mix64(seed, rnd, lo, hi) & 0xffffffff) << 32 | edge; m(v) = the least key over the valid flips that have v
               among a, b, c, d; a flip is selected iff its key is m at all four.  Two selected flips then share no vertex (a
               shared v would have m(v) equal to both keys, and keys are distinct by their edge).  So they share no face
               (a face of a flip has its three corners among the flip's four), each one's f1, f2, degrees, N(c) and positions
               are what the rules saw after the others are applied (the others change edges and degrees at their own four
               vertices only), and no new edge c-d is made twice.  Applying them in any order is applying them at once.
               apply: slot f1 = (c, a, d), slot f2 = (d, b, c), both with n0'.
  D relax      relax_sweeps Jacobi sweeps over the structure of the stage's start; every vertex reads the old positions.  A
               vertex is looked at iff it takes part, is no border vertex and meets no edge of valence >= 3.  s = the sum of x_w
               over N(v) ascending from 0.0, q = s / deg; n = the sum from 0.0 of normal(face) over the corners of v ascending;
               nn = dot(n, n), the vertex stays unless nn > 0 and finite; d = q - p, t = dot(d, n) / nn,
               p'_a = p_a + relax (d_a - n_a t).  Refused (counted, the vertex stays) where a face at v with p' at v's corner
               fails rule (e) against its standing normal or its n0.  A vertex whose p' differs from p in any bit is RELAXED:
               it moves and gets origin -1; one whose p' has p's bits stays what it is (not counted).
  output       the vertices the faces name in ascending index, the faces renamed, origin per output vertex; counts: COUNT_NAMES,
               the refusals those of the last collapse and flip round made, split_marked the marks of the last split round made.
"""
import numpy as np

from meshdecimate_ref import (_dot, _edges, _expand, _normal, border_vertices, cube12, icosphere, mix64, octahedron, sheet_mesh, tetrahedron,  # noqa: F401
                              torus_mesh, two_spheres)
from meshsimplify_ref import _sequential_sums

COUNT_NAMES = ("vertices", "faces", "splits", "collapses", "border_collapses", "flips", "relaxed", "relax_refused", "split_rounds",
               "collapse_rounds", "flip_rounds", "split_marked", "collapse_refused_valence", "collapse_refused_link",
               "collapse_refused_border", "collapse_refused_opposite", "collapse_refused_long", "collapse_refused_flip",
               "flip_refused_orient", "flip_refused_same", "flip_refused_edge", "flip_refused_degree", "flip_refused_long",
               "flip_refused_fold")
M64 = (1 << 64) - 1


def _len2(p, q):
    d = q - p
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def bounds2(L, low=0.8, high=4.0 / 3.0):
    """(low2, high2) as the caller makes them, once, in fp64"""
    L, low, high = float(L), float(low), float(high)
    if not (np.isfinite(L) and L > 0 and 0 < low < high and np.isfinite(high)):
        raise ValueError("target_edge_length > 0 and 0 < low < high, all finite, are required")
    return (low * L) * (low * L), (high * L) * (high * L)


def _keeps_side(n, w, flip2):
    g = _dot(n, w)
    return (g > 0.0) & (g * g > flip2 * (_dot(n, n) * _dot(w, w)))


class Remesher:
    def __init__(self, vertices, faces, low2, high2, flip_cos=0.2, seed=0):
        self.X = np.array(vertices, np.float64).reshape(-1, 3)
        faces = np.asarray(faces, np.int64).reshape(-1, 3)
        self.low2, self.high2, self.flip_cos, self.seed = float(low2), float(high2), float(flip_cos), int(seed) & M64
        if not (0 < self.low2 < self.high2 < np.inf and 0 <= self.flip_cos < 1):
            raise ValueError("0 < low2 < high2, finite, and 0 <= flip_cos < 1 are required")
        self.flip2 = self.flip_cos * self.flip_cos
        V = len(self.X)
        if len(faces) and (V == 0 or faces.min() < 0 or faces.max() >= V):
            raise ValueError("a face names a vertex outside [0, V)")
        finite = np.isfinite(self.X).all(axis=1)
        keep = finite[faces].all(axis=1) & (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2]) \
            if len(faces) else np.zeros(0, bool)
        self.fa = faces[keep]
        with np.errstate(all="ignore"):
            self.n0 = _normal(self.X[self.fa[:, 0]], self.X[self.fa[:, 1]], self.X[self.fa[:, 2]])
        self.origin = np.arange(V, dtype=np.int64)
        self.tick = 0
        self.trace = None

    # ---- structure -----------------------------------------------------------------------------------------------------------
    def structure(self):
        fa, V = self.fa, len(self.X)
        elo, ehi, val, eoh = _edges(fa)
        E = len(elo)
        s = dict(elo=elo, ehi=ehi, val=val, eoh=eoh, E=E)
        s["deg"] = np.bincount(elo, minlength=V) + np.bincount(ehi, minlength=V)
        border = np.zeros(V, bool)
        border[elo[val == 1]] = True
        border[ehi[val == 1]] = True
        s["border"] = border
        du, dw = np.concatenate((elo, ehi)), np.concatenate((ehi, elo))
        order = np.lexsort((dw, du))
        s["nbr"], s["nedge"] = dw[order], np.concatenate((np.arange(E), np.arange(E)))[order]
        s["nstart"] = np.cumsum(s["deg"]) - s["deg"]
        s["adj"] = np.sort(du * V + dw)
        s["corner"] = np.argsort(fa.ravel(), kind="stable")
        s["ccount"] = np.bincount(fa.ravel(), minlength=V)
        s["cstart"] = np.cumsum(s["ccount"]) - s["ccount"]
        s["hord"] = np.argsort(eoh, kind="stable")
        s["estart"] = np.cumsum(val) - val
        return s

    def _adjacent(self, s, u, w):
        adj, V = s["adj"], len(self.X)
        if len(adj) == 0:
            return np.zeros(len(u), bool)
        probe = u * V + w
        pos = np.minimum(np.searchsorted(adj, probe), len(adj) - 1)
        return adj[pos] == probe

    # ---- A ---------------------------------------------------------------------------------------------------------------------
    def split_round(self):
        """the number of edges split (0: nothing was marked)"""
        X, fa = self.X, self.fa
        V, F = len(X), len(fa)
        elo, ehi, _, eoh = _edges(fa)
        with np.errstate(all="ignore"):
            mark = _len2(X[elo], X[ehi]) > self.high2
        M = int(mark.sum())
        if M == 0:
            return 0
        mid = np.full(len(elo), -1, np.int64)
        mid[mark] = V + np.arange(M)
        m = mid[eoh].reshape(F, 3)
        k = (m >= 0).sum(axis=1)
        Fn = int((1 + k).sum())
        if 3 * Fn >= 2 ** 31 or V + M >= 2 ** 31:
            raise OverflowError("3 F must stay below 2^31")
        with np.errstate(all="ignore"):
            Xn = np.concatenate((X, (X[elo[mark]] + X[ehi[mark]]) * 0.5))
        pos = np.cumsum(1 + k) - (1 + k)
        out = np.empty((Fn, 3), np.int64)
        sel = k == 0
        out[pos[sel]] = fa[sel]
        for i in range(3):
            sel = (k == 1) & (m[:, i] >= 0)
            ci, ci1, ci2, mi, p = fa[sel, i], fa[sel, (i + 1) % 3], fa[sel, (i + 2) % 3], m[sel, i], pos[sel]
            out[p] = np.stack((ci, mi, ci2), 1)
            out[p + 1] = np.stack((mi, ci1, ci2), 1)
        sel = k == 3
        p, c, mm = pos[sel], fa[sel], m[sel]
        out[p] = np.stack((c[:, 0], mm[:, 0], mm[:, 2]), 1)
        out[p + 1] = np.stack((mm[:, 0], c[:, 1], mm[:, 1]), 1)
        out[p + 2] = np.stack((mm[:, 2], mm[:, 1], c[:, 2]), 1)
        out[p + 3] = mm
        for j in range(3):
            sel = (k == 2) & (m[:, j] < 0)
            a, b, c, m1, m2, p = fa[sel, j], fa[sel, (j + 1) % 3], fa[sel, (j + 2) % 3], m[sel, (j + 1) % 3], m[sel, (j + 2) % 3], pos[sel]
            with np.errstate(all="ignore"):
                la, lb = _len2(Xn[a], Xn[m1]), _len2(Xn[b], Xn[m2])
            first = ((la < lb) | ((la == lb) & (a < b)))[:, None]
            out[p] = np.stack((m1, c, m2), 1)
            out[p + 1] = np.where(first, np.stack((a, b, m1), 1), np.stack((a, b, m2), 1))
            out[p + 2] = np.where(first, np.stack((a, m1, m2), 1), np.stack((b, m1, m2), 1))
        self.X, self.fa, self.n0 = Xn, out, np.repeat(self.n0, 1 + k, axis=0)
        self.origin = np.concatenate((self.origin, np.full(M, -1, np.int64)))
        return M

    # ---- B ---------------------------------------------------------------------------------------------------------------------
    def collapse_point(self, s, e):
        X, lo, hi, border = self.X, s["elo"][e], s["ehi"][e], s["border"]
        with np.errstate(all="ignore"):
            mid = (X[lo] + X[hi]) * 0.5
        return np.where((border[lo] == border[hi])[:, None], mid, np.where(border[lo][:, None], X[lo], X[hi]))

    def collapse_round(self, counts):
        """the number of edges collapsed"""
        X, fa, V = self.X, self.fa, len(self.X)
        rnd = self.tick
        self.tick += 1
        s = self.structure()
        elo, ehi, val, eoh, E, deg, border = s["elo"], s["ehi"], s["val"], s["eoh"], s["E"], s["deg"], s["border"]
        with np.errstate(all="ignore"):
            short = _len2(X[elo], X[ehi]) < self.low2
            own, at = _expand(s["nstart"][elo], deg[elo])
            common = np.bincount(own[self._adjacent(s, s["nbr"][at], ehi[own])], minlength=E)
            opp = fa[:, [2, 0, 1]].ravel()
            bad_d = np.bincount(eoh[np.where(border[opp], deg[opp] < 3, deg[opp] < 4)], minlength=E) > 0
            p = self.collapse_point(s, np.arange(E))
            bad_f, bad_e = np.zeros(E, bool), np.zeros(E, bool)
            for end, other in ((elo, ehi), (ehi, elo)):
                own, at = _expand(s["nstart"][end], deg[end])
                w = s["nbr"][at]
                far = ~(_len2(X[w], p[own]) <= self.high2) & (w != other[own])
                bad_f |= np.bincount(own[far], minlength=E) > 0
                own, at = _expand(s["cstart"][end], s["ccount"][end])
                h = s["corner"][at]
                f, k = h // 3, h % 3
                sel = ~(fa[f] == other[own][:, None]).any(axis=1)
                own, f, k = own[sel], f[sel], k[sel]
                q = X[fa[f]]
                qn = q.copy()
                qn[np.arange(len(f)), k] = p[own]
                n, w = _normal(q[:, 0], q[:, 1], q[:, 2]), _normal(qn[:, 0], qn[:, 1], qn[:, 2])
                fine = _keeps_side(n, w, self.flip2) & _keeps_side(self.n0[f], w, self.flip2)
                bad_e |= np.bincount(own[~fine], minlength=E) > 0
        rules = np.stack((~((val == 1) | (val == 2)), common != val, (val == 2) & border[elo] & border[ehi], bad_d, bad_f, bad_e), 1)
        valid = short & ~rules.any(axis=1)
        refused = np.bincount(np.argmax(rules, axis=1)[short & ~valid], minlength=6)
        for i, name in enumerate(COUNT_NAMES[12:18]):
            counts[name] = int(refused[i])
        cand = np.nonzero(valid)[0]
        hsh = mix64(self.seed, rnd, elo, ehi)
        pr = np.full(E, E, np.int64)
        pr[cand[np.lexsort((cand, hsh[cand]))]] = np.arange(len(cand))
        m = np.full(V, E, np.int64)
        np.minimum.at(m, elo[cand], pr[cand])
        np.minimum.at(m, ehi[cand], pr[cand])
        M = m.copy()
        np.minimum.at(M, elo, m[ehi])
        np.minimum.at(M, ehi, m[elo])
        chosen = cand[(pr[cand] == M[elo[cand]]) & (pr[cand] == M[ehi[cand]])]
        if self.trace is not None:
            self.trace.append(dict(stage="collapse", rnd=rnd, elo=elo, ehi=ehi, valid=valid, chosen=chosen.copy(), rules=rules, short=short,
                                   nbr=s["nbr"], nstart=s["nstart"], deg=deg))
        if len(chosen) == 0:
            return 0
        lo, hi = elo[chosen], ehi[chosen]
        pt = p[chosen]
        same = (pt.view(np.int64) == np.ascontiguousarray(X[lo]).view(np.int64)).all(axis=1)
        self.origin[lo[~same]] = -1
        X[lo] = pt
        rename = np.arange(V)
        rename[hi] = lo
        counts["collapses"] += len(chosen)
        counts["border_collapses"] += int((val[chosen] == 1).sum())
        fa = rename[fa]
        live = (fa[:, 0] != fa[:, 1]) & (fa[:, 1] != fa[:, 2]) & (fa[:, 0] != fa[:, 2])
        self.fa, self.n0 = fa[live], self.n0[live]
        return len(chosen)

    # ---- C ---------------------------------------------------------------------------------------------------------------------
    def flip_round(self, counts):
        """the number of edges flipped"""
        X, fa, V = self.X, self.fa, len(self.X)
        rnd = self.tick
        self.tick += 1
        s = self.structure()
        deg, border = s["deg"], s["border"]
        e = np.nonzero(s["val"] == 2)[0]
        a, b = s["elo"][e], s["ehi"][e]
        h1, h2 = s["hord"][s["estart"][e]], s["hord"][s["estart"][e] + 1]
        flat = fa.ravel()
        orient = flat[h1] == flat[h2]
        first = flat[h1] == a
        hA, hB = np.where(first, h1, h2), np.where(first, h2, h1)
        f1, f2 = hA // 3, hB // 3
        c, d = fa[f1, (hA % 3 + 2) % 3], fa[f2, (hB % 3 + 2) % 3]
        t = np.where(border, 4, 6)

        def dev(v, by):
            x = deg[v] + by - t[v]
            return x * x
        gain = dev(a, -1) + dev(b, -1) + dev(c, 1) + dev(d, 1) < dev(a, 0) + dev(b, 0) + dev(c, 0) + dev(d, 0)
        with np.errstate(all="ignore"):
            n0p = self.n0[f1] + self.n0[f2]
            fine = np.ones(len(e), bool)
            for w in (_normal(X[c], X[a], X[d]), _normal(X[d], X[b], X[c])):
                for f in (f1, f2):
                    fine &= _keeps_side(_normal(X[fa[f, 0]], X[fa[f, 1]], X[fa[f, 2]]), w, self.flip2)
                fine &= _keeps_side(n0p, w, self.flip2)
            rules = np.stack((c == d, self._adjacent(s, c, d), (deg[a] < np.where(border[a], 3, 4)) | (deg[b] < np.where(border[b], 3, 4)),
                              ~(_len2(X[c], X[d]) <= self.high2), ~fine), 1)
        looked = ~orient & gain
        valid = looked & ~rules.any(axis=1)
        refused = np.bincount(np.argmax(rules, axis=1)[looked & ~valid], minlength=5)
        counts["flip_refused_orient"] = int(orient.sum())
        for i, name in enumerate(COUNT_NAMES[19:24]):
            counts[name] = int(refused[i])
        key = ((mix64(self.seed, rnd, a, b) & np.uint64(0xffffffff)) << np.uint64(32)) | e.astype(np.uint64)
        m = np.full(V, M64, np.uint64)
        for v in (a, b, c, d):
            np.minimum.at(m, v[valid], key[valid])
        chosen = valid & (m[a] == key) & (m[b] == key) & (m[c] == key) & (m[d] == key)
        if self.trace is not None:
            self.trace.append(dict(stage="flip", rnd=rnd, a=a, b=b, c=c, d=d, edge=e, valid=valid, chosen=chosen.copy(), rules=rules, looked=looked,
                                   orient=orient))
        n = int(chosen.sum())
        if n == 0:
            return 0
        a, b, c, d, f1, f2 = a[chosen], b[chosen], c[chosen], d[chosen], f1[chosen], f2[chosen]
        fa[f1] = np.stack((c, a, d), 1)
        fa[f2] = np.stack((d, b, c), 1)
        self.n0[f1] = n0p[chosen]
        self.n0[f2] = n0p[chosen]
        counts["flips"] += n
        return n

    # ---- D ---------------------------------------------------------------------------------------------------------------------
    def relax_stage(self, sweeps, relax, counts):
        if sweeps <= 0:
            return
        fa, V = self.fa, len(self.X)
        s = self.structure()
        deg, ccount = s["deg"], s["ccount"]
        heavy = np.zeros(V, bool)
        heavy[s["elo"][s["val"] >= 3]] = True
        heavy[s["ehi"][s["val"] >= 3]] = True
        on = np.nonzero((ccount > 0) & ~s["border"] & ~heavy)[0]
        cown, cat = _expand(s["cstart"][on], ccount[on])
        ch = s["corner"][cat]
        cf, ck = ch // 3, ch % 3
        ccnt = ccount[on]
        for _ in range(sweeps):
            X = self.X
            with np.errstate(all="ignore"):
                own, at = _expand(s["nstart"][on], deg[on])
                q = _sequential_sums(X[s["nbr"][at]], np.cumsum(deg[on]) - deg[on], deg[on]) / deg[on][:, None].astype(np.float64)
                fq = X[fa[cf]]
                fn = _normal(fq[:, 0], fq[:, 1], fq[:, 2])
                n = _sequential_sums(fn, np.cumsum(ccnt) - ccnt, ccnt)
                nn = _dot(n, n)
                p = X[on]
                d = q - p
                t = _dot(d, n) / nn
                pn = p + relax * (d - n * t[:, None])
                ok = (nn > 0.0) & np.isfinite(nn)
                moved = fq.copy()
                moved[np.arange(len(cf)), ck] = pn[cown]
                w = _normal(moved[:, 0], moved[:, 1], moved[:, 2])
                fine = _keeps_side(fn, w, self.flip2) & _keeps_side(self.n0[cf], w, self.flip2)
                folded = np.bincount(cown[~fine], minlength=len(on)) > 0
            refused = ok & folded
            differs = (np.ascontiguousarray(pn).view(np.int64) != np.ascontiguousarray(p).view(np.int64)).any(axis=1)
            go = ok & ~folded & differs
            counts["relax_refused"] += int(refused.sum())
            counts["relaxed"] += int(go.sum())
            Xn = X.copy()
            Xn[on[go]] = pn[go]
            self.origin[on[go]] = -1
            self.X = Xn

    # ---- one iteration ---------------------------------------------------------------------------------------------------------
    def iterate(self, split_rounds=4, collapse_rounds=16, flip_rounds=4, relax_sweeps=1, relax=1.0):
        counts = dict.fromkeys(COUNT_NAMES, 0)
        for _ in range(split_rounds):
            counts["split_rounds"] += 1
            counts["split_marked"] = self.split_round()
            counts["splits"] += counts["split_marked"]
            if counts["split_marked"] == 0:
                break
        for _ in range(collapse_rounds):
            counts["collapse_rounds"] += 1
            if self.collapse_round(counts) == 0:
                break
        for _ in range(flip_rounds):
            counts["flip_rounds"] += 1
            if self.flip_round(counts) == 0:
                break
        self.relax_stage(relax_sweeps, float(relax), counts)
        counts["vertices"], counts["faces"] = len(np.unique(self.fa)), len(self.fa)
        return counts

    def emit(self):
        stays = np.zeros(len(self.X), bool)
        stays[self.fa.ravel()] = True
        newid = np.cumsum(stays) - 1
        return self.X[stays].reshape(-1, 3), newid[self.fa].reshape(-1, 3).astype(np.int64), self.origin[stays]


def remesh(vertices, faces, target_edge_length, iterations=5, low=0.8, high=4.0 / 3.0, split_rounds=4, collapse_rounds=16, flip_rounds=4,
           relax_sweeps=1, relax=1.0, flip_cos=0.2, seed=0, project=None, trace=None, each=None):
    """project: None or a callable points [n, 3] -> points [n, 3] (the closest points of the input mesh), applied after every
    iteration to the vertices of origin -1; each: a callable (iteration, Remesher) called after every iteration"""
    if not 0 < float(relax) <= 1:
        raise ValueError("relax must lie in (0, 1]")
    low2, high2 = bounds2(target_edge_length, low, high)
    r = Remesher(vertices, faces, low2, high2, flip_cos, seed)
    r.trace = trace
    stats = []
    for it in range(int(iterations)):
        c = r.iterate(split_rounds, collapse_rounds, flip_rounds, relax_sweeps, relax)
        stats.append(c)
        if project is not None:
            idx = np.nonzero(r.origin < 0)[0]
            if len(idx):
                r.X[idx] = np.asarray(project(r.X[idx]), np.float64)
        if each is not None:
            each(it, r)
        if c["splits"] == 0 and c["collapses"] == 0 and c["flips"] == 0 and c["relaxed"] == 0:
            break
    return r.emit() + (stats,)


# ---- measures (outside the contract) -----------------------------------------------------------------------------------------------
def mean_edge_length(vertices, faces):
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    elo, ehi, _, _ = _edges(f)
    return float(np.sqrt(_len2(v[elo], v[ehi])).mean())


def triangle_quality(vertices, faces, L=None, low=0.8, high=4.0 / 3.0):
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    elo, ehi, val, _ = _edges(f)
    l = np.sqrt(_len2(v[elo], v[ehi]))
    out = {"edge_min": float(l.min()), "edge_mean": float(l.mean()), "edge_max": float(l.max())}
    if L is not None:
        out["edges_in_range"] = float(((l >= low * L) & (l <= high * L)).mean())
    ang = []
    for k in range(3):
        p, q, r = v[f[:, k]], v[f[:, (k + 1) % 3]], v[f[:, (k + 2) % 3]]
        u, w = q - p, r - p
        with np.errstate(all="ignore"):
            cs = (u * w).sum(1) / np.sqrt((u * u).sum(1) * (w * w).sum(1))
        ang.append(np.degrees(np.arccos(np.clip(cs, -1.0, 1.0))))
    small = np.nan_to_num(np.min(ang, axis=0))
    out["min_angle_min"], out["min_angle_mean"] = float(small.min()), float(small.mean())
    V = len(v)
    deg = np.bincount(elo, minlength=V) + np.bincount(ehi, minlength=V)
    border = np.zeros(V, bool)
    border[elo[val == 1]] = True
    border[ehi[val == 1]] = True
    part = deg > 0
    out["valence_deviation_mean"] = float(np.abs(deg - np.where(border, 4, 6))[part].mean())
    return out


def bumped_sheet():
    return sheet_mesh(17, 17, bump=0.3)


def cube24():
    from meshsimplify_ref import cube_mesh
    return cube_mesh(24)


def named_meshes():
    return {"icosphere": icosphere(3), "torus": torus_mesh(), "bumped_sheet": bumped_sheet(), "two_spheres": two_spheres(), "cube24": cube24()}


def mc_shell(n=48):
    """a marching-cubes sphere shell (the spheres of radius 0.5 and 0.7 as the zero set of ||x| - 0.6| - 0.1 on the grid of
    tests/mc_fields.py) through the library's host marching cubes (surfd_mc_iso), welded by position"""
    from mc_fields import _grid
    from surfd_amd import mcubes
    x, y, z = _grid(n)
    vol = np.ascontiguousarray(np.abs(np.sqrt(x * x + y * y + z * z) - np.float32(0.6)) - np.float32(0.1), np.float32)
    v, f = mcubes.marching_cubes(vol, 0.0)
    v, inv = np.unique(np.asarray(v, np.float64), axis=0, return_inverse=True)
    f = inv.reshape(-1)[np.asarray(f, np.int64)]
    return v, f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]


def reference_check(shell=None):
    """triangle_quality before and after the restatement at L = the input's mean edge length, default knobs: the content of
    profiles/meshremesh_ref_check.json (python tests/meshremesh_ref.py rewrites the file)"""
    out = {"what": "tests/meshremesh_ref.py with its default knobs (5 iterations) at L = the mean edge length of the input: "
                   "triangle_quality before and after (recorded; on the shell the direction is asserted)"}
    meshes = named_meshes()
    if shell is not None:
        meshes["mc_shell"] = shell
    for name, (v, f) in meshes.items():
        L = mean_edge_length(v, f)
        ov, of, _, stats = remesh(v, f, L)
        out[name] = {"L": L, "faces_before": int(len(f)), "faces_after": int(len(of)), "iterations": len(stats),
                     "before": triangle_quality(v, f, L), "after": triangle_quality(ov, of, L)}
    return out


if __name__ == "__main__":
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "meshremesh_ref_check.json")
    with open(path, "w") as fh:
        json.dump(reference_check(mc_shell()), fh, indent=1)
        fh.write("\n")
    print(path)
