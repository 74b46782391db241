// Incremental isotropic remeshing of a mesh to a target edge length on the device (Botsch and Kobbelt 2004: split, collapse, flip,
// relax), as ROUNDS OF INDEPENDENT OPERATIONS: every round is keys, stable sorts, scans and one lane per item, and the result does
// not depend on launch geometry.  tests/meshremesh_ref.py restates the contract sequentially in numpy and IS the contract:
// vertices (every double), faces, origin and every count equal its output bit for bit and in the same order.  The mesh grows, and
// the caller steps between iterations (the projection onto the input surface is surfd_amd/meshremesh.py's), so this is a handle.
//
// Contract.  Input: vertices fp64 [V, 3], faces int32 [F, 3], on the device; low2 = (low L)^2 and high2 = (high L)^2 made once by
// the caller in fp64 (0 < low2 < high2, finite), 0 <= flip_cos < 1, seed (64 bits).
// len2(p, q): d = q - p, (dx dx + dy dy) + dz dz.  normal(q0, q1, q2) and dot: e1 = q1 - q0, e2 = q2 - q0,
// n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x); (ax bx + ay by) + az bz.
//   kept faces   a face goes if it names a vertex with a NaN or an Inf or names one vertex twice.  An index outside [0, V) is
//                SURFD_ERR_ARG.
//   state        X (a vertex keeps its index for the life of the handle; new vertices are appended), the faces, n0 per face (the
//                normal of the input face, which children and flipped pairs inherit), origin per vertex (its input index while it is
//                an input vertex at its input position, else -1), tick (numbers every collapse and flip round made: mix64's round).
//   structure    rebuilt at the start of every round: half-edge h = 3 f + k names (min, max) of corners k and (k + 1) % 3; the unique
//                pairs (lo < hi) ascending are the edges, the half-edges of an edge in ascending h, their number its valence.
//                deg(v): the edges at v; N(v): its neighbours ascending; corners of v: the h that name v, ascending; a vertex is
//                a BORDER vertex when a valence-1 edge meets it; it TAKES PART when a face names it.
//   ITERATION = A, B, C, D.  A round that is looked at counts as made, the one that finds nothing included; a stage ends with it.
//   A split      up to split_rounds rounds.  An edge is marked iff len2(x_lo, x_hi) > high2.  The marked edges in ascending edge
//                order get the vertices V_now, V_now + 1, ... at (x_lo + x_hi) 0.5, origin -1.  A face with k marked half-edges is
//                replaced by 1 + k faces at the exclusive sum of 1 + k, each with the parent's n0; c_i its corners, m_i the new
//                vertex of half-edge i:  k = 0 the face;  k = 1 (i marked): (c_i, m_i, c_i+2), (m_i, c_i+1, c_i+2);
//                k = 3: (c0, m0, m2), (m0, c1, m1), (m2, m1, c2), (m0, m1, m2);  k = 2 (j unmarked; a = c_j, b = c_j+1, c = c_j+2,
//                m1 = m_j+1, m2 = m_j+2): (m1, c, m2), then where len2(x_a, x_m1) < len2(x_b, x_m2), or they are equal and a < b:
//                (a, b, m1), (a, m1, m2); else (a, b, m2), (b, m1, m2).  3 F' >= 2^31 or V' >= 2^31: refused, the state unchanged.
//   B collapse   up to collapse_rounds rounds, rnd = tick, tick += 1.  Only edges with len2(x_lo, x_hi) < low2 are looked at; the
//                FIRST rule that refuses one is counted:
//                (a) valence 1 or 2;  (b) |N(lo) & N(hi)| == valence;  (c) not (valence 2 and lo and hi both border vertices);
//                (d) every opposite vertex o: deg(o) >= 4, or >= 3 at a border vertex;
//                the point: (x_lo + x_hi) 0.5 where both or neither end is a border vertex, else the border end's own bits;
//                (f) for every w of N(lo), then of N(hi), other than lo and hi: len2(x_w, point) <= high2;
//                (e) for every face at lo or at hi that does not hold both, the moved corner replaced by the point: with n the
//                    standing normal, n' the new one: g = dot(n, n'), g > 0 and g g > flip_cos2 (dot(n, n) dot(n', n')); and the
//                    same with the face's n0 in the place of n.
//                priority = (mix64(seed, rnd, lo, hi), edge); m(v) = the least priority of the valid edges at v; M(v) = the least m
//                over v and N(v); an edge is selected iff its priority is M(lo) and M(hi): selected edges have distinct,
//                non-adjacent end points (csrc/meshdecimate.hip, step 5), and rule (f) looks at positions of N(lo) | N(hi) only,
//                none of which another selected collapse moves.
//                apply: hi is renamed lo, x_lo = the point, origin[lo] = -1 unless the point has x_lo's bits; faces with two equal
//                names go, the rest keep their order and n0.
//   C flip       up to flip_rounds rounds, rnd = tick, tick += 1.  Only valence-2 edges are looked at; a = lo, b = hi.  With its
//                two half-edges in ascending h: one whose two half-edges both leave a or both leave b is refused (orient).  f1
//                holds a -> b, c its third corner; f2 holds b -> a, d its third corner.  t(v) = 4 at a border vertex, else 6;
//                an edge goes on iff the sum of (deg - t)^2 over a, b, c, d gets strictly smaller with deg(a) - 1, deg(b) - 1,
//                deg(c) + 1, deg(d) + 1 (c and d as they are, equal or not).  Then the first refusing rule is counted:
//                (same) c != d;  (edge) d not in N(c);  (degree) deg(a) and deg(b) >= 4, or >= 3 at a border vertex;
//                (long) len2(x_c, x_d) <= high2;  (fold) w = normal(c, a, d), then normal(d, b, c): against n = the standing normal
//                of f1, then of f2, then n0' = n0_f1 + n0_f2: g = dot(n, w), g > 0 and g g > flip_cos2 (dot(n, n) dot(w, w))
//                (a zero w fails g > 0).
//                key = (mix64(seed, rnd, lo, hi) & 0xffffffff) << 32 | edge; m(v) = the least key over the valid flips that have v
//                among a, b, c, d; a flip is selected iff its key is m at all four.  Two selected flips then share no vertex, so
//                no face, and each one's faces, degrees, N(c) and positions are what the rules saw (the restatement has the
//                argument).  apply: slot f1 = (c, a, d), slot f2 = (d, b, c), both with n0'.
//   D relax      relax_sweeps Jacobi sweeps over the structure of the stage's start; every vertex reads the old positions.  A
//                vertex is looked at iff it takes part, is no border vertex and meets no edge of valence >= 3.  s = the sum of x_w
//                over N(v) ascending from 0.0, q = s / deg; n = the sum from 0.0 of normal(face) over the corners of v ascending;
//                nn = dot(n, n), the vertex stays unless nn > 0 and finite; d = q - p, t = dot(d, n) / nn,
//                p'_a = p_a + relax (d_a - n_a t).  Refused (counted, the vertex stays) where a face at v with p' at v's corner
//                fails rule (e) against its standing normal or its n0.  A vertex whose p' differs from p in any bit is RELAXED:
//                it moves and gets origin -1; one whose p' has p's bits stays what it is (not counted).
//   output       the vertices the faces name in ascending index, the faces renamed, origin per output vertex; counts[24]:
//                vertices, faces, splits, collapses, border collapses, flips, relaxed, relax refusals, split / collapse / flip
//                rounds made, the marks of the last split round made, the refusals of the last collapse round by (a) (b) (c) (d)
//                (f) (e) and of the last flip round by orient, same, edge, degree, long, fold.
//
// Passes (256-wide grids, one item per lane; sorts and scans are hipcub's through the handle's CubWorkspace; the er_ pieces are
// meshrounds.h's, shared with csrc/meshdecimate.hip).  Create: rm_vertex_flags -> er_kept_faces (er_face_mark, the only kernel that
// sees caller indices unchecked -> exclusive sum -> er_compact_kept) -> HOST READ (bad index, kept faces) -> er_face_normals (n0).
// The structure of a round (er_structure): er_half_keys -> stable sort of (lo << 32 | hi, h) -> run_heads -> exclusive sum ->
// er_edge_fill -> HOST READ (E) -> er_edge_info; with rings also: stable sort of (vertex, corner) -> er_run_bounds, er_run_bounds
// over lo, stable sort of (hi, edge) -> er_run_bounds.  Split: rm_split_mark -> two exclusive sums (the
// marks, their half-edges) -> HOST READ (marks, F' = F + the marked half-edges, taken in 64 bits) -> growth if the arrays are short (the stream is drained, one new block is
// carved, the state copied, the round's structure made again) -> rm_split_count -> exclusive sum -> rm_split_vertices -> rm_split_faces.  Collapse: rm_collapse_valid
// (er_refused_abcd, rule (f), er_fans_keep_side) -> er_vertex_min -> er_ring_min -> rm_collapse_select -> rm_collapse_apply ->
// er_rename_faces -> exclusive sum -> er_compact_live -> HOST READ (selected, faces, refusals).  Flip: rm_flip_valid (64-bit atomicMin of the key at a, b, c, d: a minimum has no
// order) -> rm_flip_apply -> HOST READ.  Relax: rm_relax per sweep (X -> X2, swapped), one HOST READ at the end of the iteration
// with the count of named vertices (er_count_named: er_mark_named -> sum).  rm_relax and rm_flip_valid are kernels of their own so that neither
// spills (profiles/meshremesh_regs.txt has the compiler's numbers).
// No float atomics, no lane waits on another: every sum is one lane's loop in a fixed order, every device loop runs over a CSR
// run (the corners, edges or neighbours of one vertex, the half-edges of one edge of valence <= 2).
// Memory: ONE block per handle, carved by a ScratchArena (meshremesh_layout.h, checked on the host by tools/meshremesh_layout_check.cpp) for capacities (Vcap, Fcap) >= the input: 112 Vcap + 344 Fcap bytes and the
// slots' rounding, plus hipcub's workspace sized for the largest sort.  Both grow geometrically (at least twofold) in a split round
// whose result does not fit; nothing is allocated in a round that does not grow.
// Limits: F >= 0, V >= 0; 3 F < 2^31 at any time, beyond: SURFD_ERR_UNSUPPORTED.  ONE STREAM AT A TIME PER HANDLE.
// Bounds: every kernel guards its 64-bit thread index; arrays of Vcap entries are indexed by caller indices only behind the
// comparison in er_face_mark or by names of current faces (< V_now <= Vcap; new names are V_now + position < V' <= Vcap, checked on
// the host before they are written); arrays of 3 Fcap entries by corners of current faces, by sorted positions below 3 F_now, or by
// edges below E <= 3 F_now; split children go to positions below F' <= Fcap.
#include "common.h"
#include "devscratch.h"
#include "meshedit.h"
#include "meshrounds.h"
#include "meshscene.h"
#include "meshremesh_layout.h"
#include <cmath>

namespace surfd {

enum { RM_BAD = 0, RM_KEPT, RM_E, RM_SEL, RM_FNEW, RM_BORDER, RM_VOUT, RM_RELAXED, RM_RELAX_REF, RM_HALF, RM_REF = 12 };      // of the RM_WORDS counter words
// RM_REF + 0..5: collapse refusals (a) (b) (c) (d) (f) (e); RM_REF + 6..11: flip refusals orient, same, edge, degree, long, fold
enum { RM_COUNTS = 24 };

__device__ __forceinline__ double rm_len2(const er_v3 &p, const er_v3 &q) {
    const double dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ er_v3 rm_mid(const er_v3 &a, const er_v3 &b) { return {(a.x + b.x) * 0.5, (a.y + b.y) * 0.5, (a.z + b.z) * 0.5}; }
__device__ __forceinline__ bool rm_same_bits(const er_v3 &a, const er_v3 &b) {
    return __double_as_longlong(a.x) == __double_as_longlong(b.x) && __double_as_longlong(a.y) == __double_as_longlong(b.y) &&
           __double_as_longlong(a.z) == __double_as_longlong(b.z);
}

__global__ void rm_vertex_flags_kernel(const double *__restrict__ vertices, int V, int *__restrict__ nonfinite, double *__restrict__ X, int *__restrict__ origin) {
    if (dev_tid() >= V) return;
    const long v = dev_tid();
    nonfinite[v] = vertex_nonfinite(vertices, v);
#pragma unroll
    for (int j = 0; j < 3; ++j) X[3 * v + j] = vertices[3 * v + j];
    origin[v] = (int)v;
}

// ---- A: split ---------------------------------------------------------------------------------------------------------------------
// mark[e]; mval[e]: the half-edges of a marked edge, the faces it adds
__global__ void rm_split_mark_kernel(const double *__restrict__ X, const int *__restrict__ elo, const int *__restrict__ ehi, const int *__restrict__ eval, int E,
                                     double high2, int *__restrict__ mark, int *__restrict__ mval) {
    if (dev_tid() >= E) return;
    const long e = dev_tid();
    const int on = rm_len2(er_load(X, elo[e]), er_load(X, ehi[e])) > high2 ? 1 : 0;
    mark[e] = on;
    mval[e] = on ? eval[e] : 0;
}

__global__ void rm_split_count_kernel(const int *__restrict__ eoh, const int *__restrict__ mark, int F, int *__restrict__ fcnt) {
    if (dev_tid() >= F) return;
    const long f = dev_tid();
    fcnt[f] = 1 + mark[eoh[3 * f]] + mark[eoh[3 * f + 1]] + mark[eoh[3 * f + 2]];
}

// the caller has made room for V_now + marks vertices
__global__ void rm_split_vertices_kernel(double *__restrict__ X, int *__restrict__ origin, const int *__restrict__ elo, const int *__restrict__ ehi, int E,
                                         const int *__restrict__ mark, const int *__restrict__ mpos, int Vn) {
    if (dev_tid() >= E || !mark[dev_tid()]) return;
    const long e = dev_tid(), v = (long)Vn + mpos[e];
    const er_v3 m = rm_mid(er_load(X, elo[e]), er_load(X, ehi[e]));
    X[3 * v] = m.x; X[3 * v + 1] = m.y; X[3 * v + 2] = m.z;
    origin[v] = -1;
}

__device__ __forceinline__ void rm_put(int32_t *__restrict__ out, double *__restrict__ nout, long p, int a, int b, int c, const er_v3 &n) {
    out[3 * p] = a; out[3 * p + 1] = b; out[3 * p + 2] = c;
    nout[3 * p] = n.x; nout[3 * p + 1] = n.y; nout[3 * p + 2] = n.z;
}

// one lane per face: its 1 + k children at fpos[f] (the new vertices are in X already)
__global__ void rm_split_faces_kernel(const double *__restrict__ X, const int32_t *__restrict__ fa, const double *__restrict__ nref, int F,
                                      const int *__restrict__ eoh, const int *__restrict__ mark, const int *__restrict__ mpos, int Vn,
                                      const int *__restrict__ fpos, int32_t *__restrict__ out, double *__restrict__ nout) {
    if (dev_tid() >= F) return;
    const long f = dev_tid(), p = fpos[f];
    const int c[3] = {fa[3 * f], fa[3 * f + 1], fa[3 * f + 2]};
    int m[3], k = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int e = eoh[3 * f + i];
        m[i] = mark[e] ? Vn + mpos[e] : -1;
        k += mark[e];
    }
    const er_v3 n = {nref[3 * f], nref[3 * f + 1], nref[3 * f + 2]};
    if (k == 0) {
        rm_put(out, nout, p, c[0], c[1], c[2], n);
    } else if (k == 1) {
        const int i = m[0] >= 0 ? 0 : (m[1] >= 0 ? 1 : 2);
        rm_put(out, nout, p, c[i], m[i], c[(i + 2) % 3], n);
        rm_put(out, nout, p + 1, m[i], c[(i + 1) % 3], c[(i + 2) % 3], n);
    } else if (k == 3) {
        rm_put(out, nout, p, c[0], m[0], m[2], n);
        rm_put(out, nout, p + 1, m[0], c[1], m[1], n);
        rm_put(out, nout, p + 2, m[2], m[1], c[2], n);
        rm_put(out, nout, p + 3, m[0], m[1], m[2], n);
    } else {
        const int j = m[0] < 0 ? 0 : (m[1] < 0 ? 1 : 2);
        const int a = c[j], b = c[(j + 1) % 3], cc = c[(j + 2) % 3], m1 = m[(j + 1) % 3], m2 = m[(j + 2) % 3];
        const double la = rm_len2(er_load(X, a), er_load(X, m1)), lb = rm_len2(er_load(X, b), er_load(X, m2));
        const bool first = la < lb || (la == lb && a < b);
        rm_put(out, nout, p, m1, cc, m2, n);
        rm_put(out, nout, p + 1, a, b, first ? m1 : m2, n);
        rm_put(out, nout, p + 2, first ? a : b, m1, m2, n);
    }
}

// ---- B: collapse ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ er_v3 rm_collapse_point(const double *__restrict__ X, const int *__restrict__ vborder, int lo, int hi) {
    const er_v3 a = er_load(X, lo), b = er_load(X, hi);
    const int ba = vborder[lo], bb = vborder[hi];
    return ba == bb ? rm_mid(a, b) : (ba ? a : b);
}

// one lane per edge: short edges through rules (a) (b) (c) (d) (f) (e), the first refusal counted
__global__ void __launch_bounds__(256) rm_collapse_valid_kernel(const double *__restrict__ X, const int32_t *__restrict__ fa, er_rings rings, const int *__restrict__ estart,
                                                                const int *__restrict__ sh, const int *__restrict__ eval, const int *__restrict__ vborder,
                                                                const int *__restrict__ vfirst, const int *__restrict__ vlast, const int *__restrict__ vf,
                                                                const double *__restrict__ nref, int E, double low2, double high2, double flip2, rm_u64 salt,
                                                                int *__restrict__ cand, rm_u64 *__restrict__ ehash, int *cnt) {
    if (dev_tid() >= E) return;
    const long e = dev_tid();
    const int lo = rings.elo[e], hi = rings.ehi[e], val = eval[e];
    ehash[e] = er_mix(salt, lo, hi);
    cand[e] = 0;
    if (!(rm_len2(er_load(X, lo), er_load(X, hi)) < low2)) return;
    int refused = er_refused_abcd(rings, fa, estart, sh, vborder, e, lo, hi, val);
    if (refused < 0) {
        const er_v3 p = rm_collapse_point(X, vborder, lo, hi);
#pragma unroll 1
        for (int side = 0; side < 2 && refused < 0; ++side) {
            const er_ring r = rings.at(side ? hi : lo);
            for (int j = 0; j < r.n; ++j) {
                const int w = r.other(j);
                if (w == lo || w == hi) continue;
                if (!(rm_len2(er_load(X, w), p) <= high2)) { refused = 4; break; }
            }
        }
        if (refused < 0 && !er_fans_keep_side(X, fa, vfirst, vlast, vf, nref, lo, hi, p, flip2)) refused = 5;
    }
    if (refused >= 0) { atomicAdd(cnt + RM_REF + refused, 1); return; }      // an integer count has no order
    cand[e] = 1;
}

__global__ void rm_collapse_select_kernel(int E, const int *__restrict__ cand, const int *__restrict__ elo, const int *__restrict__ ehi, const int *__restrict__ eval,
                                          const int *__restrict__ Mbest, int *__restrict__ sel, int *cnt) {
    if (dev_tid() >= E) return;
    const int e = (int)dev_tid();
    const int s = (cand[e] && Mbest[elo[e]] == e && Mbest[ehi[e]] == e) ? 1 : 0;
    sel[e] = s;
    if (s) {
        atomicAdd(cnt + RM_SEL, 1);
        if (eval[e] == 1) atomicAdd(cnt + RM_BORDER, 1);
    }
}

// the end points of the selected edges are pairwise distinct and not adjacent: a lane reads and writes its own two vertices
__global__ void rm_collapse_apply_kernel(int E, const int *__restrict__ sel, const int *__restrict__ elo, const int *__restrict__ ehi,
                                         const int *__restrict__ vborder, double *__restrict__ X, int *__restrict__ origin, int *__restrict__ rename) {
    if (dev_tid() >= E || !sel[dev_tid()]) return;
    const long e = dev_tid();
    const int lo = elo[e], hi = ehi[e];
    const er_v3 p = rm_collapse_point(X, vborder, lo, hi);
    if (!rm_same_bits(p, er_load(X, lo))) origin[lo] = -1;
    X[3L * lo] = p.x; X[3L * lo + 1] = p.y; X[3L * lo + 2] = p.z;
    rename[hi] = lo;
}

// ---- C: flip ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int rm_dev2(int deg, int border) { const int x = deg - (border ? 4 : 6); return x * x; }

// one lane per edge of valence 2: orient, the gain, rules same, edge, degree, long, fold; a valid flip lowers m at a, b, c, d
__global__ void __launch_bounds__(256) rm_flip_valid_kernel(const double *__restrict__ X, const int32_t *__restrict__ fa, er_rings rings, const int *__restrict__ estart,
                                                            const int *__restrict__ sh, const int *__restrict__ eval, const int *__restrict__ vborder,
                                                            const double *__restrict__ nref, int E, double high2, double flip2, rm_u64 salt,
                                                            int *__restrict__ cand, int *__restrict__ qc, int *__restrict__ qd, rm_u64 *__restrict__ vmin, int *cnt) {
    if (dev_tid() >= E) return;
    const long e = dev_tid();
    cand[e] = 0;
    if (eval[e] != 2) return;
    const int a = rings.elo[e], b = rings.ehi[e];
    const long h1 = sh[estart[e]], h2 = sh[estart[e] + 1];
    if (fa[h1] == fa[h2]) { atomicAdd(cnt + RM_REF + 6, 1); return; }
    const long hA = fa[h1] == a ? h1 : h2, hB = fa[h1] == a ? h2 : h1;
    const long f1 = hA / 3, f2 = hB / 3;
    const int c = fa[3 * f1 + ((int)(hA - 3 * f1) + 2) % 3], d = fa[3 * f2 + ((int)(hB - 3 * f2) + 2) % 3];
    const int da = rings.degree(a), db = rings.degree(b), dc = rings.degree(c), dd = rings.degree(d);
    const int ba = vborder[a], bb = vborder[b], bc = vborder[c], bd = vborder[d];
    if (!(rm_dev2(da - 1, ba) + rm_dev2(db - 1, bb) + rm_dev2(dc + 1, bc) + rm_dev2(dd + 1, bd) <
          rm_dev2(da, ba) + rm_dev2(db, bb) + rm_dev2(dc, bc) + rm_dev2(dd, bd)))
        return;
    int refused = -1;
    if (c == d) refused = 7;
    if (refused < 0) {
        const er_ring r = rings.at(c);
        for (int j = 0; j < r.n; ++j)
            if (r.other(j) == d) { refused = 8; break; }
    }
    if (refused < 0 && (da < (ba ? 3 : 4) || db < (bb ? 3 : 4))) refused = 9;
    const er_v3 xa = er_load(X, a), xb = er_load(X, b), xc = er_load(X, c), xd = er_load(X, d);
    if (refused < 0 && !(rm_len2(xc, xd) <= high2)) refused = 10;
    if (refused < 0) {
        const er_v3 n1 = er_normal(er_load(X, fa[3 * f1]), er_load(X, fa[3 * f1 + 1]), er_load(X, fa[3 * f1 + 2]));
        const er_v3 n2 = er_normal(er_load(X, fa[3 * f2]), er_load(X, fa[3 * f2 + 1]), er_load(X, fa[3 * f2 + 2]));
        const er_v3 np = {nref[3 * f1] + nref[3 * f2], nref[3 * f1 + 1] + nref[3 * f2 + 1], nref[3 * f1 + 2] + nref[3 * f2 + 2]};
        const er_v3 w1 = er_normal(xc, xa, xd), w2 = er_normal(xd, xb, xc);
        const double ww1 = er_dot(w1, w1), ww2 = er_dot(w2, w2);
        if (!(er_keeps(n1, w1, ww1, flip2) && er_keeps(n2, w1, ww1, flip2) && er_keeps(np, w1, ww1, flip2) && er_keeps(n1, w2, ww2, flip2) &&
              er_keeps(n2, w2, ww2, flip2) && er_keeps(np, w2, ww2, flip2)))
            refused = 11;
    }
    if (refused >= 0) { atomicAdd(cnt + RM_REF + refused, 1); return; }
    cand[e] = 1; qc[e] = c; qd[e] = d;
    const rm_u64 key = ((er_mix(salt, a, b) & 0xffffffffull) << 32) | (rm_u64)(unsigned)e;
    atomicMin(vmin + a, key); atomicMin(vmin + b, key); atomicMin(vmin + c, key); atomicMin(vmin + d, key);      // a minimum has no order
}

// selected flips share no vertex, so no face: a lane reads and writes its own two faces
__global__ void rm_flip_apply_kernel(int32_t *__restrict__ fa, double *__restrict__ nref, const int *__restrict__ elo, const int *__restrict__ ehi,
                                     const int *__restrict__ estart, const int *__restrict__ sh, int E, rm_u64 salt, const int *__restrict__ cand,
                                     const int *__restrict__ qc, const int *__restrict__ qd, const rm_u64 *__restrict__ vmin, int *cnt) {
    if (dev_tid() >= E || !cand[dev_tid()]) return;
    const long e = dev_tid();
    const int a = elo[e], b = ehi[e], c = qc[e], d = qd[e];
    const rm_u64 key = ((er_mix(salt, a, b) & 0xffffffffull) << 32) | (rm_u64)(unsigned)e;
    if (vmin[a] != key || vmin[b] != key || vmin[c] != key || vmin[d] != key) return;
    const long h1 = sh[estart[e]], h2 = sh[estart[e] + 1];
    const long f1 = (fa[h1] == a ? h1 : h2) / 3, f2 = (fa[h1] == a ? h2 : h1) / 3;
    fa[3 * f1] = c; fa[3 * f1 + 1] = a; fa[3 * f1 + 2] = d;
    fa[3 * f2] = d; fa[3 * f2 + 1] = b; fa[3 * f2 + 2] = c;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double s = nref[3 * f1 + j] + nref[3 * f2 + j];
        nref[3 * f1 + j] = s; nref[3 * f2 + j] = s;
    }
    atomicAdd(cnt + RM_SEL, 1);
}

// ---- D: relax ---------------------------------------------------------------------------------------------------------------------
// one lane per vertex: X -> Xn (every vertex is written: the moved ones their p', the others what they were)
__global__ void __launch_bounds__(256) rm_relax_kernel(const double *__restrict__ X, double *__restrict__ Xn, const int32_t *__restrict__ fa, er_rings rings, int V,
                                                       const int *__restrict__ vborder, const int *__restrict__ vheavy, const int *__restrict__ vfirst,
                                                       const int *__restrict__ vlast, const int *__restrict__ vf, const double *__restrict__ nref, double relax,
                                                       double flip2, int *__restrict__ origin, int *cnt) {
    if (dev_tid() >= V) return;
    const long v = dev_tid();
    const er_v3 p = er_load(X, v);
    er_v3 out = p;
    const int i0 = vfirst[v], i1 = vlast[v];
    if (i1 > i0 && !vborder[v] && !vheavy[v]) {
        const er_ring r = rings.at(v);
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int j = 0; j < r.n; ++j) {
            const er_v3 w = er_load(X, r.other(j));
            sx = sx + w.x; sy = sy + w.y; sz = sz + w.z;
        }
        const double deg = (double)r.n;
        er_v3 n = {0.0, 0.0, 0.0};
        for (int i = i0; i < i1; ++i) {
            const long f = vf[i] / 3;
            const er_v3 m = er_normal(er_load(X, fa[3 * f]), er_load(X, fa[3 * f + 1]), er_load(X, fa[3 * f + 2]));
            n.x = n.x + m.x; n.y = n.y + m.y; n.z = n.z + m.z;
        }
        const double nn = er_dot(n, n);
        if (nn > 0.0 && isfinite(nn)) {
            const er_v3 d = {sx / deg - p.x, sy / deg - p.y, sz / deg - p.z};
            const double t = er_dot(d, n) / nn;
            const er_v3 q = {p.x + relax * (d.x - n.x * t), p.y + relax * (d.y - n.y * t), p.z + relax * (d.z - n.z * t)};
            bool fine = true;
            for (int i = i0; i < i1 && fine; ++i) {
                const long h = vf[i], f = h / 3;
                const int t3[3] = {fa[3 * f], fa[3 * f + 1], fa[3 * f + 2]};
                fine = er_keeps_side(X, t3, (int)(h - 3 * f), q, {nref[3 * f], nref[3 * f + 1], nref[3 * f + 2]}, flip2);
            }
            if (!fine) atomicAdd(cnt + RM_RELAX_REF, 1);
            else if (!rm_same_bits(q, p)) { out = q; origin[v] = -1; atomicAdd(cnt + RM_RELAXED, 1); }
        }
    }
    Xn[3 * v] = out.x; Xn[3 * v + 1] = out.y; Xn[3 * v + 2] = out.z;
}

// ---- output -----------------------------------------------------------------------------------------------------------------------
__global__ void rm_out_vertices_kernel(const double *__restrict__ X, const int *__restrict__ origin, int V, const int *__restrict__ stays,
                                       const int *__restrict__ newid, double *__restrict__ out, int32_t *__restrict__ out_origin) {
    if (dev_tid() >= V || !stays[dev_tid()]) return;
    const long v = dev_tid(), n = newid[v];                    // n <= v
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * n + j] = X[3 * v + j];
    if (out_origin) out_origin[n] = origin[v];
}

}  // namespace surfd

using namespace surfd;

struct surfd_meshremesh {
    int Vn = 0, Fn = 0;                  // vertex slots and faces now
    long Vcap = 0, Fcap = 0;
    double low2 = 0, high2 = 0, flip2 = 0;
    uint64_t seed = 0, tick = 0;
    char *block = nullptr;
    rm_arrays a = {};
    CubWorkspace cub;                    // the handle's own: fixed between growths
};

static const long RM_MAX_F = (long)INT_MAX / 3;

// hipcub's workspace for the capacities (V, F): the largest need of the operations the rounds use, each at its largest size (a
// small scan needs more than a small sort).  Each is asked through a workspace of its own, which its first call sizes; the scans
// have no size-only form and run over temporaries.  The stream has drained.
static int rm_reserve_cub(surfd_meshremesh *m, long V, long F, hipStream_t st) {
    const rm_arrays &a = m->a;
    const int H = (int)(3 * F);
    size_t need = 0;
    for (int op = 0; op < 4; ++op) {
        CubWorkspace probe;
        int rc;
        if (op == 0) rc = probe.sort_pairs(a.hkey, a.hkeys, a.iota, a.sh, H, 64, st, true);
        else if (op == 1) rc = probe.sort_pairs(a.vkey, a.vkeys, a.iota, a.vf, H, 32, st, true);
        else if (op == 2) rc = probe.exclusive_sum(a.sel, a.selpos, H, st);
        else rc = probe.exclusive_sum(a.stays, a.newid, (int)V, st);
        if (rc == SURFD_OK && hipStreamSynchronize(st) != hipSuccess) rc = SURFD_ERR_HIP;
        need = std::max(need, probe.bytes);
        (void)hipFree(probe.ptr);
        SURFD_TRY(rc);
    }
    (void)hipFree(m->cub.ptr);
    m->cub.ptr = nullptr; m->cub.bytes = 0;
    HIP_TRY(hipMalloc((void **)&m->cub.ptr, need));
    m->cub.bytes = need;
    return SURFD_OK;
}

// a new block for (V, F) >= the state; the state is copied, the old block freed once the stream has drained
static int rm_reserve(surfd_meshremesh *m, long V, long F, hipStream_t st) {
    if (F > RM_MAX_F || V > (long)INT_MAX) SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_meshremesh: 3 F must stay below 2^31, F = %ld, V = %ld", F, V);
    HIP_TRY(hipStreamSynchronize(st));                       // the kernels in flight read the old block
    char *block = nullptr;
    HIP_TRY(hipMalloc((void **)&block, rm_block_bytes(V, F)));
    rm_arrays n = {};
    if (const int rc = rm_carve(n, block, V, F); rc != SURFD_OK) { (void)hipFree(block); return rc; }
    hipError_t e = hipSuccess;
    if (m->block) {
        const rm_arrays &o = m->a;
        e = hipMemcpyAsync(n.cnt, o.cnt, RM_WORDS * sizeof(int), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && m->Vn > 0) e = hipMemcpyAsync(n.X, o.X, dev_bytes<double>(3L * m->Vn), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && m->Vn > 0) e = hipMemcpyAsync(n.origin, o.origin, dev_bytes<int>(m->Vn), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && m->Fn > 0) e = hipMemcpyAsync(n.fa, o.fa, dev_bytes<int32_t>(3L * m->Fn), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && m->Fn > 0) e = hipMemcpyAsync(n.nra, o.nra, dev_bytes<double>(3L * m->Fn), hipMemcpyDeviceToDevice, st);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(er_iota_kernel, dim3(dev_grid(3 * F)), dim3(256), 0, st, n.iota, 3 * F);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipFree(block); SURFD_FAIL(SURFD_ERR_HIP, "surfd_meshremesh: growing the handle failed: %s", hipGetErrorString(e)); }
    (void)hipFree(m->block);
    m->block = block; m->a = n; m->Vcap = V; m->Fcap = F;
    return rm_reserve_cub(m, V, F, st);
}

extern "C" void surfd_meshremesh_destroy(surfd_meshremesh *m) {
    if (!m) return;
    (void)hipFree(m->block);
    (void)hipFree(m->cub.ptr);
    delete m;
}

static int rm_read(surfd_meshremesh *m, int *hc, hipStream_t st) { return read_words(m->a.cnt, hc, RM_WORDS, st); }

// the structure of a round over the handle's faces (Fn > 0): the flags zeroed, then er_structure over the arrays as they are now
static int rm_round_structure(surfd_meshremesh *m, bool rings, int *E, hipStream_t st) {
    int hc[RM_WORDS];
    HIP_TRY(hipMemsetAsync(m->a.vborder, 0, rm_round_zero_bytes(m->Vcap), st));      // vborder .. hlast (meshremesh_layout.h)
    return er_structure(m->a, m->cub, m->Vn, m->Fn, rings, m->a.cnt, RM_WORDS, RM_E, hc, E, st);
}

extern "C" int surfd_meshremesh_create(const double *vertices, int V, const int32_t *faces, int F, double low2, double high2, double flip_cos,
                                       uint64_t seed, surfd_stream s, surfd_meshremesh **out) {
    const char *who = "surfd_meshremesh_create";
    if (!out) SURFD_FAIL(SURFD_ERR_ARG, "%s: null out", who);
    *out = nullptr;
    SURFD_TRY(mesh_sizes(who, F, V, SURFD_ERR_UNSUPPORTED));
    if (!(low2 > 0.0 && low2 < high2) || !std::isfinite(high2))
        SURFD_FAIL(SURFD_ERR_ARG, "%s: 0 < low2 = %g < high2 = %g, finite, is required", who, low2, high2);
    if (!(flip_cos >= 0.0 && flip_cos < 1.0)) SURFD_FAIL(SURFD_ERR_ARG, "%s: flip_cos = %g must lie in [0, 1)", who, flip_cos);
    if ((V > 0 && !vertices) || (F > 0 && !faces)) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    hipStream_t st = as_stream(s);
    std::unique_ptr<surfd_meshremesh, void (*)(surfd_meshremesh *)> m(new surfd_meshremesh, surfd_meshremesh_destroy);
    m->low2 = low2; m->high2 = high2; m->flip2 = flip_cos * flip_cos; m->seed = seed;
    SURFD_TRY(rm_reserve(m.get(), std::max(V, 1), std::max(F, 1), st));
    const rm_arrays &a = m->a;
    HIP_TRY(hipMemsetAsync(a.cnt, 0, RM_WORDS * sizeof(int), st));
    m->Vn = V;
    if (F > 0) {                                             // with V == 0 too: every index is then outside [0, V)
        int *nonfinite = a.mbest, *keep = a.live, *kpos = a.lpos;
        DEV_LAUNCH(rm_vertex_flags_kernel, V, vertices, V, nonfinite, a.X, a.origin);
        SURFD_TRY(er_kept_faces(m->cub, faces, F, V, nonfinite, keep, kpos, nullptr, a.cnt + RM_BAD, a.cnt + RM_KEPT, a.fa, st));
        int hc[RM_WORDS];
        SURFD_TRY(rm_read(m.get(), hc, st));
        if (hc[RM_BAD]) return mesh_bad_index(who, V);
        m->Fn = hc[RM_KEPT];
        if (m->Fn > 0) DEV_LAUNCH(er_face_normals_kernel, m->Fn, (const double *)a.X, (const int32_t *)a.fa, m->Fn, a.nra);
    } else if (V > 0) {
        DEV_LAUNCH(rm_vertex_flags_kernel, V, vertices, V, a.mbest, a.X, a.origin);
    }
    HIP_TRY(hipStreamSynchronize(st));
    *out = m.release();
    return SURFD_OK;
}

extern "C" int surfd_meshremesh_sizes(const surfd_meshremesh *m, int64_t *vertices, int64_t *faces) {
    if (!m || !vertices || !faces) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshremesh_sizes: null argument");
    *vertices = m->Vn; *faces = m->Fn;
    return SURFD_OK;
}

static int rm_split_round(surfd_meshremesh *m, int *marked, hipStream_t st) {
    int hc[RM_WORDS], E;
    for (;;) {
        SURFD_TRY(rm_round_structure(m, false, &E, st));
        const rm_arrays &a = m->a;
        int *mark = a.sel, *mpos = a.selpos, *mval = a.cand, *mvpos = a.hie, *fcnt = a.live, *fpos = a.lpos;
        DEV_LAUNCH(rm_split_mark_kernel, E, (const double *)a.X, (const int *)a.elo, (const int *)a.ehi, (const int *)a.eval, E, m->high2, mark, mval);
        SURFD_TRY(m->cub.exclusive_sum(mark, mpos, E, st));
        SURFD_TRY(scan_total(mark, mpos, E, a.cnt + RM_SEL, st));
        SURFD_TRY(m->cub.exclusive_sum(mval, mvpos, E, st));      // the marked half-edges: at most 3 F, an int holds them
        SURFD_TRY(scan_total(mval, mvpos, E, a.cnt + RM_HALF, st));
        SURFD_TRY(rm_read(m, hc, st));
        const long M = hc[RM_SEL];
        *marked = (int)M;
        if (M == 0) return SURFD_OK;
        const long Fn2 = (long)m->Fn + hc[RM_HALF], Vn2 = (long)m->Vn + M;      // F' = F + the marked half-edges, in 64 bits
        if (Fn2 > RM_MAX_F || Vn2 > (long)INT_MAX)
            SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_meshremesh_iterate: 3 F must stay below 2^31, a split round would make F = %ld, V = %ld", Fn2, Vn2);
        if (Fn2 > m->Fcap || Vn2 > m->Vcap) {                 // grow at least twofold, then make the round's structure again
            const long Fc = Fn2 > m->Fcap ? std::min(RM_MAX_F, std::max(2 * m->Fcap, Fn2)) : m->Fcap;
            const long Vc = Vn2 > m->Vcap ? std::min((long)INT_MAX, std::max(2 * m->Vcap, Vn2)) : m->Vcap;
            SURFD_TRY(rm_reserve(m, Vc, Fc, st));
            continue;
        }
        DEV_LAUNCH(rm_split_count_kernel, m->Fn, (const int *)a.eoh, (const int *)mark, m->Fn, fcnt);
        SURFD_TRY(m->cub.exclusive_sum(fcnt, fpos, m->Fn, st));      // ends at F' <= RM_MAX_F, as checked above
        DEV_LAUNCH(rm_split_vertices_kernel, E, a.X, a.origin, (const int *)a.elo, (const int *)a.ehi, E, (const int *)mark, (const int *)mpos, m->Vn);
        DEV_LAUNCH(rm_split_faces_kernel, m->Fn, (const double *)a.X, (const int32_t *)a.fa, (const double *)a.nra, m->Fn, (const int *)a.eoh, (const int *)mark,
                   (const int *)mpos, m->Vn, (const int *)fpos, a.fb, a.nrb);
        std::swap(m->a.fa, m->a.fb);
        std::swap(m->a.nra, m->a.nrb);
        m->Vn = (int)Vn2; m->Fn = (int)Fn2;
        return SURFD_OK;
    }
}

static int rm_collapse_round(surfd_meshremesh *m, int64_t *counts, int *selected, hipStream_t st) {
    int hc[RM_WORDS], E;
    const rm_u64 salt = er_salt(m->seed, m->tick++);
    SURFD_TRY(rm_round_structure(m, true, &E, st));
    const rm_arrays &a = m->a;
    const int V = m->Vn, Fn = m->Fn;
    const er_rings rings = {a.elo, a.ehi, a.hie, a.hfirst, a.hlast, a.lfirst, a.llast};
    HIP_TRY(hipMemsetAsync(a.cnt + RM_SEL, 0, (RM_WORDS - RM_SEL) * sizeof(int), st));
    DEV_LAUNCH(rm_collapse_valid_kernel, E, (const double *)a.X, (const int32_t *)a.fa, rings, (const int *)a.estart, (const int *)a.sh, (const int *)a.eval,
               (const int *)a.vborder, (const int *)a.vfirst, (const int *)a.vlast, (const int *)a.vf, (const double *)a.nra, E, m->low2, m->high2, m->flip2,
               salt, a.cand, a.ehash, a.cnt);
    DEV_LAUNCH(er_vertex_min_kernel, V, rings, V, (const int *)a.cand, (const rm_u64 *)a.ehash, a.mbest);
    DEV_LAUNCH(er_ring_min_kernel, V, rings, V, (const int *)a.mbest, (const rm_u64 *)a.ehash, a.Mbest);
    DEV_LAUNCH(rm_collapse_select_kernel, E, E, (const int *)a.cand, (const int *)a.elo, (const int *)a.ehi, (const int *)a.eval, (const int *)a.Mbest, a.sel, a.cnt);
    DEV_LAUNCH(er_iota_kernel, V, a.rename, (long)V);
    DEV_LAUNCH(rm_collapse_apply_kernel, E, E, (const int *)a.sel, (const int *)a.elo, (const int *)a.ehi, (const int *)a.vborder, a.X, a.origin, a.rename);
    DEV_LAUNCH(er_rename_faces_kernel, Fn, a.fa, Fn, (const int *)a.rename, a.live);
    SURFD_TRY(m->cub.exclusive_sum(a.live, a.lpos, Fn, st));
    SURFD_TRY(scan_total(a.live, a.lpos, Fn, a.cnt + RM_FNEW, st));
    DEV_LAUNCH(er_compact_live_kernel, Fn, (const int32_t *)a.fa, (const double *)a.nra, Fn, (const int *)a.live, (const int *)a.lpos, a.fb, a.nrb);
    SURFD_TRY(rm_read(m, hc, st));
    for (int i = 0; i < 6; ++i) counts[12 + i] = hc[RM_REF + i];
    counts[3] += hc[RM_SEL];
    counts[4] += hc[RM_BORDER];
    *selected = hc[RM_SEL];
    if (hc[RM_SEL] > 0) {                                     // otherwise fa is what it was: nothing was renamed
        std::swap(m->a.fa, m->a.fb);
        std::swap(m->a.nra, m->a.nrb);
        m->Fn = hc[RM_FNEW];
    }
    return SURFD_OK;
}

static int rm_flip_round(surfd_meshremesh *m, int64_t *counts, int *selected, hipStream_t st) {
    int hc[RM_WORDS], E;
    const rm_u64 salt = er_salt(m->seed, m->tick++);
    SURFD_TRY(rm_round_structure(m, true, &E, st));
    const rm_arrays &a = m->a;
    const er_rings rings = {a.elo, a.ehi, a.hie, a.hfirst, a.hlast, a.lfirst, a.llast};
    int *qc = a.head, *qd = a.hpos;                          // the heads of the edge runs are spent
    HIP_TRY(hipMemsetAsync(a.cnt + RM_SEL, 0, (RM_WORDS - RM_SEL) * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(a.vmin, 0xFF, dev_bytes<rm_u64>(m->Vn), st));
    DEV_LAUNCH(rm_flip_valid_kernel, E, (const double *)a.X, (const int32_t *)a.fa, rings, (const int *)a.estart, (const int *)a.sh, (const int *)a.eval,
               (const int *)a.vborder, (const double *)a.nra, E, m->high2, m->flip2, salt, a.cand, qc, qd, a.vmin, a.cnt);
    DEV_LAUNCH(rm_flip_apply_kernel, E, a.fa, a.nra, (const int *)a.elo, (const int *)a.ehi, (const int *)a.estart, (const int *)a.sh, E, salt, (const int *)a.cand,
               (const int *)qc, (const int *)qd, (const rm_u64 *)a.vmin, a.cnt);
    SURFD_TRY(rm_read(m, hc, st));
    for (int i = 0; i < 6; ++i) counts[18 + i] = hc[RM_REF + 6 + i];
    counts[5] += hc[RM_SEL];
    *selected = hc[RM_SEL];
    return SURFD_OK;
}

extern "C" int surfd_meshremesh_iterate(surfd_meshremesh *m, int split_rounds, int collapse_rounds, int flip_rounds, int relax_sweeps, double relax,
                                        int64_t *counts, surfd_stream s) {
    const char *who = "surfd_meshremesh_iterate";
    if (!m || !counts) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    for (int i = 0; i < RM_COUNTS; ++i) counts[i] = 0;
    if (split_rounds < 0 || collapse_rounds < 0 || flip_rounds < 0 || relax_sweeps < 0)
        SURFD_FAIL(SURFD_ERR_ARG, "%s: the rounds (%d, %d, %d) and sweeps (%d) must not be negative", who, split_rounds, collapse_rounds, flip_rounds, relax_sweeps);
    if (!(relax > 0.0 && relax <= 1.0)) SURFD_FAIL(SURFD_ERR_ARG, "%s: relax = %g must lie in (0, 1]", who, relax);
    hipStream_t st = as_stream(s);
    for (int r = 0; r < split_rounds; ++r) {
        int marked = 0;
        ++counts[8];
        if (m->Fn > 0) SURFD_TRY(rm_split_round(m, &marked, st));
        counts[11] = marked;
        counts[2] += marked;
        if (marked == 0) break;
    }
    for (int r = 0; r < collapse_rounds; ++r) {
        int selected = 0;
        ++counts[9];
        if (m->Fn > 0) SURFD_TRY(rm_collapse_round(m, counts, &selected, st));
        else { ++m->tick; for (int i = 0; i < 6; ++i) counts[12 + i] = 0; }
        if (selected == 0) break;
    }
    for (int r = 0; r < flip_rounds; ++r) {
        int selected = 0;
        ++counts[10];
        if (m->Fn > 0) SURFD_TRY(rm_flip_round(m, counts, &selected, st));
        else { ++m->tick; for (int i = 0; i < 6; ++i) counts[18 + i] = 0; }
        if (selected == 0) break;
    }
    HIP_TRY(hipMemsetAsync(m->a.cnt + RM_RELAXED, 0, 2 * sizeof(int), st));
    if (relax_sweeps > 0 && m->Fn > 0) {
        int E;
        SURFD_TRY(rm_round_structure(m, true, &E, st));
        const er_rings rings = {m->a.elo, m->a.ehi, m->a.hie, m->a.hfirst, m->a.hlast, m->a.lfirst, m->a.llast};
        for (int r = 0; r < relax_sweeps; ++r) {
            const rm_arrays &a = m->a;
            DEV_LAUNCH(rm_relax_kernel, m->Vn, (const double *)a.X, a.X2, (const int32_t *)a.fa, rings, m->Vn, (const int *)a.vborder, (const int *)a.vheavy,
                       (const int *)a.vfirst, (const int *)a.vlast, (const int *)a.vf, (const double *)a.nra, relax, m->flip2, a.origin, a.cnt);
            std::swap(m->a.X, m->a.X2);
        }
    }
    SURFD_TRY(er_count_named(m->cub, m->a.fa, m->Fn, m->Vn, m->a.stays, m->a.newid, m->a.cnt + RM_VOUT, st));
    int hc[RM_WORDS];
    SURFD_TRY(rm_read(m, hc, st));
    counts[0] = hc[RM_VOUT];
    counts[1] = m->Fn;
    counts[6] = hc[RM_RELAXED];
    counts[7] = hc[RM_RELAX_REF];
    return SURFD_OK;
}

extern "C" int surfd_meshremesh_get_positions(const surfd_meshremesh *m, double *positions, int32_t *origin, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshremesh_get_positions: null handle");
    hipStream_t st = as_stream(s);
    if (m->Vn == 0) return SURFD_OK;
    if (positions) HIP_TRY(hipMemcpyAsync(positions, m->a.X, dev_bytes<double>(3L * m->Vn), hipMemcpyDeviceToDevice, st));
    if (origin) HIP_TRY(hipMemcpyAsync(origin, m->a.origin, dev_bytes<int>(m->Vn), hipMemcpyDeviceToDevice, st));
    return SURFD_OK;
}

extern "C" int surfd_meshremesh_set_positions(surfd_meshremesh *m, const double *positions, surfd_stream s) {
    if (!m || !positions) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshremesh_set_positions: null argument");
    if (m->Vn == 0) return SURFD_OK;
    HIP_TRY(hipMemcpyAsync(m->a.X, positions, dev_bytes<double>(3L * m->Vn), hipMemcpyDeviceToDevice, as_stream(s)));
    return SURFD_OK;
}

extern "C" int surfd_meshremesh_emit(surfd_meshremesh *m, double *out_vertices, int32_t *out_faces, int32_t *out_origin, int64_t *counts, surfd_stream s) {
    const char *who = "surfd_meshremesh_emit";
    if (!m || !counts) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    counts[0] = counts[1] = 0;
    if (m->Fn == 0) return SURFD_OK;
    if (!out_vertices || !out_faces) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    hipStream_t st = as_stream(s);
    const rm_arrays &a = m->a;
    SURFD_TRY(er_count_named(m->cub, a.fa, m->Fn, m->Vn, a.stays, a.newid, a.cnt + RM_VOUT, st));
    DEV_LAUNCH(rm_out_vertices_kernel, m->Vn, (const double *)a.X, (const int *)a.origin, m->Vn, (const int *)a.stays, (const int *)a.newid, out_vertices, out_origin);
    DEV_LAUNCH(er_out_faces_kernel, 3L * m->Fn, (const int32_t *)a.fa, 3L * m->Fn, (const int *)a.newid, out_faces);
    int hc[RM_WORDS];
    SURFD_TRY(rm_read(m, hc, st));
    counts[0] = hc[RM_VOUT];
    counts[1] = m->Fn;
    return SURFD_OK;
}
