// Edge-collapse decimation of a mesh to a target face count on the device (quadric error metrics, Garland-Heckbert), as ROUNDS OF
// INDEPENDENT COLLAPSES: no priority queue, every round is keys, stable sorts, scans and one lane per item, and the result does not
// depend on launch geometry.  tests/meshdecimate_ref.py restates the contract sequentially in numpy and IS the contract: vertices
// (every double), faces, the map and the counts equal its output bit for bit and in the same order.
//
// Contract.  Vertices fp64 [V, 3], faces int32 [F, 3], on the device; target_faces >= 0; border_weight >= 0, 0 <= flip_cos < 1,
// rank_tol > 0 (all finite), spread >= 1, max_rounds >= 1, seed (64 bits).
//   kept faces   a face goes if it names a vertex with a NaN or an Inf or names one vertex twice.  An index outside [0, V) is
//                SURFD_ERR_ARG.  A vertex TAKES PART when a kept face names it.  Faces keep their order, a vertex its index.
//   centre       lo, hi = the minimum and maximum per axis over the vertices that take part, each + 0.0; c0 = 0.5 lo + 0.5 hi
//                (0 without such a vertex).  P_v = x_v - c0 for every vertex; all arithmetic below is on P.
//   quadrics     per vertex (A as 00 01 02 11 12 22, b 3, c 1), from 0.0, one addition per term:
//                face terms, for the faces at the vertex in ascending 3 f + corner: q_i = P of the corners (corner 0 first),
//                  e1 = q1 - q0, e2 = q2 - q0, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x),
//                  l = sqrt((nx nx + ny ny) + nz nz); nothing where l == 0; d = -((nx q0x + ny q0y) + nz q0z);
//                  A_ab += (n_a n_b) / l, b_a += (n_a d) / l, c += (d d) / l.
//                then border terms, for the border half-edges h = 3 f + k (from corner k to corner (k + 1) % 3, the unordered pair
//                  occurring once among the kept faces) that end at the vertex, in ascending h: t = P_to - P_from, n and l of the
//                  face as above, m = (ty nz - tz ny, tz nx - tx nz, tx ny - ty nx), mm = (mx mx + my my) + mz mz; nothing where
//                  mm == 0; s = (border_weight l) / mm; d = -((mx qx + my qy) + mz qz) with q = P_from;
//                  A_ab += (m_a m_b) s, b_a += (m_a d) s, c += (d d) s.
//   ROUND r = 0, 1, ... while F_now > target and r < max_rounds, from the current faces:
//   1 edges      half-edge h = 3 f + k names (min, max) of its two corners; the unique pairs (lo < hi) ascending are the edges, the
//                number of half-edges of a pair is its valence.  deg(v): the edges at v; N(v): its neighbours; a vertex is a BORDER
//                vertex when a valence-1 edge meets it.
//   2 placement  Q = Q_lo + Q_hi (lo first, entry by entry).  m = (P_lo + P_hi) 0.5.  r_a = -(b_a + ((A_a0 m0 + A_a1 m1) + A_a2 m2)).
//                A is decomposed by six cyclic Jacobi sweeps (the rotation of csrc/cloudnormals.hip, tests/normals_ref.py:
//                jacobi_f64ops); lmax = l0, then l1 and l2 each taken where greater; acc = 0; for j = 0, 1, 2 with lmax > 0 and
//                lambda_j > rank_tol lmax: t = ((u_0j r0 + u_1j r1) + u_2j r2) / lambda_j, acc_a = acc_a + u_aj t.  x = m + acc.
//                box: mn_a = min(P_lo a, P_hi a), mx_a likewise, ext = the largest mx_a - mn_a.  x is accepted when it is finite
//                and mn_a - ext <= x_a <= mx_a + ext for every a.  Otherwise the point is m, then P_lo where its cost is strictly
//                smaller, then P_hi where its cost is strictly smaller than the best so far.
//                cost(p): g_a = (A_a0 p0 + A_a1 p1) + A_a2 p2; k = ((p0 g0 + p1 g1) + p2 g2 + 2.0 ((b0 p0 + b1 p1) + b2 p2)) + c;
//                cost = k where k > 0 or k is a NaN, else 0.0.
//   3 validity   the FIRST rule that refuses an edge is counted for it:
//                (a) valence 1 or 2;  (b) |N(lo) & N(hi)| == valence (a merge of the two ascending neighbour lists);
//                (c) not (valence 2 and lo and hi both border vertices);
//                (d) every opposite vertex o (the third corner of a face at the edge): deg(o) >= 4 where o is no border vertex,
//                    deg(o) >= 3 where it is one (a lone triangle does not vanish);
//                (n) the cost is no NaN;
//                (e) for every face at lo or at hi that does not hold both, with corners q0 q1 q2 and the moved corner replaced
//                    by the point in q': n = (q1 - q0) x (q2 - q0), n' likewise (components as above), g = (nx n'x + ny n'y) + nz n'z,
//                    nn = (nx nx + ny ny) + nz nz, n'n' likewise: g > 0 and g g > flip_cos2 (nn n'n'), flip_cos2 = flip_cos flip_cos;
//                      and the same two comparisons with n0 in the place of n, the normal the face had in the input (over P; a face
//                      of a round is one input face renamed, so n0 travels with it): the turns of many rounds do not add up, and a
//                      sliver does not come to lie on its side.
//   4 candidates key = bits(fp32(cost)) << 32 | (mix64(seed, r, lo, hi) & 0xffffffff) for a valid edge (an fp32 below the smallest
//                normal number counts as 0), all ones for an invalid one.  Stable sort by key (ties to the lower edge).
//                remaining = ceil((F_now - target) / 2).  The candidates are the first min(valid, spread remaining) edges.
//                mix64 = fin(fin(seed + 0x9e3779b97f4a7c15 (r + 1)) ^ (lo << 32 | hi)), fin = splitmix64's finaliser.
//   5 selection  priority of a candidate = (mix64(seed, r, lo, hi), edge), compared in that order: independent of the cost.
//                m(v) = the least priority of the candidates at v; M(v) = the least m over v and N(v).  A candidate is selected iff
//                its priority is M(lo) and M(hi): the end points of two selected edges are distinct and not adjacent, so no face
//                holds an end point of each, their fans are disjoint and neither changes what the other's rules looked at
//                (the restatement gives the argument).  If more than `remaining` are selected, those of lowest sort rank stay.
//   6 apply      hi is renamed lo, P_lo = the point, Q_lo = Q_lo + Q_hi.  Faces are renamed; one with two equal names goes; the
//                rest keep their order.  vertex_map is composed one hop (a survivor of a round was not collapsed in it).
//   end          stop: 0 F_now <= target, 1 a round selected nothing (stalled), 2 max_rounds rounds were made.
//                Output vertices: those the final faces name, in ascending input index; one that never moved is the input vertex
//                itself, a moved one is c0 + P.  vertex_map: the output vertex that an input vertex ended in, -1 where it took no
//                part (or its survivor is named by no face).  counts[12]: output vertices, output faces, rounds, collapses, border
//                collapses, stop, refusals by (a) (b) (c) (d) (e) (n) in the last round made.
//
// Passes (256-wide grids, one item per lane; sorts and scans are hipcub's through CubWorkspace; the er_ pieces are meshrounds.h's,
// shared with csrc/meshremesh.hip).  Once: qd_nonfinite -> er_kept_faces (er_face_mark, the only kernel that sees caller indices
// unchecked -> exclusive sum -> er_compact_kept) -> HOST READ 0 (bad index, kept faces) -> qd_box (block minimum and maximum of an
// order-preserving integer image, then integer atomics: no order) -> qd_centre -> qd_centre_vertices -> er_face_normals (n0).
// Per round: er_structure (er_half_keys -> stable sort of (lo << 32 | hi, h) -> run_heads -> exclusive sum -> er_edge_fill (edge of
// every half-edge, start of every edge) -> stable sort of (vertex, corner) -> er_run_bounds (corners of every vertex) -> HOST READ 1
// (E) -> er_edge_info (valence, border vertices) -> er_run_bounds over lo -> stable sort of (hi, edge) -> er_run_bounds (with the lo
// run: the incident edges and the neighbours of a vertex, ascending)) -> round 0: qd_init_quadrics (one lane per vertex walks its
// corners) -> qd_place (Jacobi, point, cost) -> qd_valid (er_refused_abcd: merge, opposite vertices; rule (n); er_fans_keep_side:
// both fans; the key) -> stable 64-bit sort of (key, edge) -> qd_candidates -> er_vertex_min -> er_ring_min -> qd_select ->
// exclusive sum -> qd_apply -> er_rename_faces -> exclusive sum -> er_compact_live -> qd_map_hop -> HOST READ 2 (selected, faces,
// refusals).  At the end: er_count_named (er_mark_named -> exclusive sum) -> qd_final_vertices, er_out_faces, qd_vertex_map -> one
// read of the output size.
// qd_place is apart from qd_valid so that neither spills (DESIGN.md section 8.18 has the compiler's numbers).
// No float atomics, no lane waits on another: every sum is one lane's loop in a fixed order, every device loop runs over a CSR
// run (the corners, edges or neighbours of one vertex, the half-edges of one edge of valence <= 2) or six sweeps.
// Scratch: ONE arena sized for the input, carved before the first round (sizes only shrink), plus hipcub's workspace, sized by
// the first sort, the largest: 168 V + 452 F bytes (an edge array has 3 F entries: the bound).  Freed when the call returns.
// Limits: F >= 0, V >= 0 (F = 0 or V = 0: empty outputs, the map all -1); 3 F < 2^31, beyond: SURFD_ERR_UNSUPPORTED.
// Bounds: every kernel guards its thread index; arrays of V entries are indexed by caller indices only behind the comparison in
// er_face_mark (a face that fails it is not kept, and only kept faces are read again) or by names of kept faces; arrays of 3 F
// entries by corners 3 f + k of current faces, by sorted positions below 3 F_now, or by edges below E <= 3 F_now.
#include "common.h"
#include "devscratch.h"
#include "meshedit.h"
#include "meshrounds.h"
#include "meshscene.h"
#include <cmath>

namespace surfd {

typedef unsigned long long qd_u64;
enum { QD_BAD = 0, QD_KEPT, QD_E, QD_SEL, QD_FNEW, QD_BORDER, QD_VOUT, QD_VALID, QD_REF_A, QD_REF_B, QD_REF_C, QD_REF_D, QD_REF_E, QD_REF_N, QD_WORDS = 16 };

// an image of the doubles in which unsigned order is numeric order (no NaN comes here)
__device__ __forceinline__ qd_u64 qd_ordered(double x) {
    const qd_u64 b = (qd_u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double qd_unordered(qd_u64 o) {
    const qd_u64 b = (o >> 63) ? (o & ~0x8000000000000000ull) : ~o;
    return __longlong_as_double((long long)b);
}

__global__ void qd_nonfinite_kernel(const double *__restrict__ vertices, int V, int *__restrict__ nonfinite) {
    if (dev_tid() >= V) return;
    nonfinite[dev_tid()] = vertex_nonfinite(vertices, dev_tid());
}

// box[0..2] preset to all ones, box[3..5] to zero: the smallest and the largest image per axis over the vertices that take part
__global__ void __launch_bounds__(256) qd_box_kernel(const double *__restrict__ vertices, int V, const int *__restrict__ part, qd_u64 *box) {
    __shared__ qd_u64 sm[6][256];
    const long v = dev_tid();
    const bool on = v < V && part[v];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const qd_u64 o = on ? qd_ordered(vertices[3 * v + j]) : 0;
        sm[j][threadIdx.x] = on ? o : ~0ull;
        sm[3 + j][threadIdx.x] = o;                          // no image of a finite double is 0
    }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const qd_u64 a = sm[j][threadIdx.x], b = sm[j][threadIdx.x + w];
                sm[j][threadIdx.x] = b < a ? b : a;
                const qd_u64 c = sm[3 + j][threadIdx.x], d = sm[3 + j][threadIdx.x + w];
                sm[3 + j][threadIdx.x] = d > c ? d : c;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 3 && sm[threadIdx.x][0] != ~0ull) {
        atomicMin(box + threadIdx.x, sm[threadIdx.x][0]);
        atomicMax(box + 3 + threadIdx.x, sm[3 + threadIdx.x][0]);
    }
}

__global__ void qd_centre_kernel(const qd_u64 *__restrict__ box, double *__restrict__ c0) {
    if (blockIdx.x != 0 || threadIdx.x >= 3) return;
    const int j = threadIdx.x;
    c0[j] = box[j] == ~0ull ? 0.0 : 0.5 * (qd_unordered(box[j]) + 0.0) + 0.5 * (qd_unordered(box[3 + j]) + 0.0);
}

__global__ void qd_centre_vertices_kernel(const double *__restrict__ vertices, int V, const double *__restrict__ c0, double *__restrict__ P,
                                          int *__restrict__ vmap, int *__restrict__ rename, int *__restrict__ moved) {
    if (dev_tid() >= V) return;
    const long v = dev_tid();
#pragma unroll
    for (int j = 0; j < 3; ++j) P[3 * v + j] = vertices[3 * v + j] - c0[j];
    vmap[v] = (int)v; rename[v] = (int)v; moved[v] = 0;
}

// one lane per vertex: the face terms of its corners in ascending 3 f + corner, then the border terms in ascending half-edge
__global__ void __launch_bounds__(256) qd_init_quadrics_kernel(const double *__restrict__ P, const int32_t *__restrict__ fa, int V, const int *__restrict__ vfirst,
                                                               const int *__restrict__ vlast, const int *__restrict__ vf, const int *__restrict__ eoh,
                                                               const int *__restrict__ eval, double border_weight, double *__restrict__ Q) {
    if (dev_tid() >= V) return;
    const long v = dev_tid();
    double q[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) q[j] = 0.0;
    const int i0 = vfirst[v], i1 = vlast[v];
    for (int i = i0; i < i1; ++i) {
        const long f = vf[i] / 3;
        const er_v3 q0 = er_load(P, fa[3 * f]), q1 = er_load(P, fa[3 * f + 1]), q2 = er_load(P, fa[3 * f + 2]);
        const er_v3 n = er_normal(q0, q1, q2);
        const double l = sqrt(er_dot(n, n));
        if (l == 0.0) continue;
        const double d = -er_dot(n, q0);
        q[0] = q[0] + (n.x * n.x) / l; q[1] = q[1] + (n.x * n.y) / l; q[2] = q[2] + (n.x * n.z) / l;
        q[3] = q[3] + (n.y * n.y) / l; q[4] = q[4] + (n.y * n.z) / l; q[5] = q[5] + (n.z * n.z) / l;
        q[6] = q[6] + (n.x * d) / l; q[7] = q[7] + (n.y * d) / l; q[8] = q[8] + (n.z * d) / l;
        q[9] = q[9] + (d * d) / l;
    }
    for (int i = i0; i < i1; ++i) {
        const long f = vf[i] / 3;
        const int t[3] = {fa[3 * f], fa[3 * f + 1], fa[3 * f + 2]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int from = t[k], to = t[(k + 1) % 3];
            if ((from != (int)v && to != (int)v) || eval[eoh[3 * f + k]] != 1) continue;
            const er_v3 q0 = er_load(P, t[0]), q1 = er_load(P, t[1]), q2 = er_load(P, t[2]);
            const er_v3 n = er_normal(q0, q1, q2);
            const double l = sqrt(er_dot(n, n));
            const er_v3 pf = er_load(P, from), pt = er_load(P, to);
            const double tx = pt.x - pf.x, ty = pt.y - pf.y, tz = pt.z - pf.z;
            const er_v3 m = {ty * n.z - tz * n.y, tz * n.x - tx * n.z, tx * n.y - ty * n.x};
            const double mm = er_dot(m, m);
            if (mm == 0.0) continue;
            const double s = (border_weight * l) / mm;
            const double d = -er_dot(m, pf);
            q[0] = q[0] + (m.x * m.x) * s; q[1] = q[1] + (m.x * m.y) * s; q[2] = q[2] + (m.x * m.z) * s;
            q[3] = q[3] + (m.y * m.y) * s; q[4] = q[4] + (m.y * m.z) * s; q[5] = q[5] + (m.z * m.z) * s;
            q[6] = q[6] + (m.x * d) * s; q[7] = q[7] + (m.y * d) * s; q[8] = q[8] + (m.z * d) * s;
            q[9] = q[9] + (d * d) * s;
        }
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) Q[10 * v + j] = q[j];
}

// one Jacobi rotation of the pair (p, q); r is the third index (csrc/cloudnormals.hip: cnrm_rotate, csrc/meshsimplify.hip: vc_rotate,
// kept as a copy so those files' code stays as their tests pinned it)
__device__ __forceinline__ void qd_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q, double &v1p,
                                          double &v1q, double &v2p, double &v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double root = __builtin_sqrt(theta * theta + 1.0);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(theta) + root);
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
    const double s = t * c;
    const double tapq = t * apq;
    app = app - tapq;
    aqq = aqq + tapq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    const double n0p = c * v0p - s * v0q, n0q = s * v0p + c * v0q;
    const double n1p = c * v1p - s * v1q, n1q = s * v1p + c * v1q;
    const double n2p = c * v2p - s * v2q, n2q = s * v2p + c * v2q;
    v0p = n0p; v0q = n0q; v1p = n1p; v1q = n1q; v2p = n2p; v2q = n2q;
}

__device__ __forceinline__ double qd_cost(const double *q, double p0, double p1, double p2) {
    const double g0 = (q[0] * p0 + q[1] * p1) + q[2] * p2, g1 = (q[1] * p0 + q[3] * p1) + q[4] * p2, g2 = (q[2] * p0 + q[4] * p1) + q[5] * p2;
    const double k = (((p0 * g0 + p1 * g1) + p2 * g2) + 2.0 * ((q[6] * p0 + q[7] * p1) + q[8] * p2)) + q[9];
    return (k > 0.0 || k != k) ? k : 0.0;
}

// one lane per edge: the point and its cost
__global__ void __launch_bounds__(256) qd_place_kernel(const double *__restrict__ P, const double *__restrict__ Q, const int *__restrict__ elo,
                                                       const int *__restrict__ ehi, int E, double rank_tol, double *__restrict__ ept,
                                                       double *__restrict__ ecost) {
    if (dev_tid() >= E) return;
    const long e = dev_tid();
    const long lo = elo[e], hi = ehi[e];
    double q[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) q[j] = Q[10 * lo + j] + Q[10 * hi + j];
    const er_v3 a = er_load(P, lo), b = er_load(P, hi);
    const double m0 = (a.x + b.x) * 0.5, m1 = (a.y + b.y) * 0.5, m2 = (a.z + b.z) * 0.5;
    const double r0 = -(q[6] + ((q[0] * m0 + q[1] * m1) + q[2] * m2)), r1 = -(q[7] + ((q[1] * m0 + q[3] * m1) + q[4] * m2)),
                 r2 = -(q[8] + ((q[2] * m0 + q[4] * m1) + q[5] * m2));
    double a00 = q[0], a01 = q[1], a02 = q[2], a11 = q[3], a12 = q[4], a22 = q[5];
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // v[row][column]
#pragma unroll 1
    for (int sweep = 0; sweep < 6; ++sweep) {
        qd_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (p, q) = (0, 1), r = 2
        qd_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
        qd_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
    }
    double lmax = a00;
    if (a11 > lmax) lmax = a11;
    if (a22 > lmax) lmax = a22;
    const double cut = rank_tol * lmax;
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
    if (lmax > 0.0) {
        if (a00 > cut) { const double t = ((v00 * r0 + v10 * r1) + v20 * r2) / a00; e0 = e0 + v00 * t; e1 = e1 + v10 * t; e2 = e2 + v20 * t; }
        if (a11 > cut) { const double t = ((v01 * r0 + v11 * r1) + v21 * r2) / a11; e0 = e0 + v01 * t; e1 = e1 + v11 * t; e2 = e2 + v21 * t; }
        if (a22 > cut) { const double t = ((v02 * r0 + v12 * r1) + v22 * r2) / a22; e0 = e0 + v02 * t; e1 = e1 + v12 * t; e2 = e2 + v22 * t; }
    }
    const double x0 = m0 + e0, x1 = m1 + e1, x2 = m2 + e2;
    const double mn0 = a.x < b.x ? a.x : b.x, mn1 = a.y < b.y ? a.y : b.y, mn2 = a.z < b.z ? a.z : b.z;
    const double mx0 = a.x < b.x ? b.x : a.x, mx1 = a.y < b.y ? b.y : a.y, mx2 = a.z < b.z ? b.z : a.z;
    double ext = mx0 - mn0;
    if (mx1 - mn1 > ext) ext = mx1 - mn1;
    if (mx2 - mn2 > ext) ext = mx2 - mn2;
    const bool ok = isfinite(x0) && isfinite(x1) && isfinite(x2) && x0 >= mn0 - ext && x0 <= mx0 + ext && x1 >= mn1 - ext && x1 <= mx1 + ext &&
                    x2 >= mn2 - ext && x2 <= mx2 + ext;
    double p0 = x0, p1 = x1, p2 = x2, cost;
    if (ok) {
        cost = qd_cost(q, x0, x1, x2);
    } else {
        p0 = m0; p1 = m1; p2 = m2; cost = qd_cost(q, m0, m1, m2);
        const double ca = qd_cost(q, a.x, a.y, a.z);
        if (ca < cost) { p0 = a.x; p1 = a.y; p2 = a.z; cost = ca; }
        const double cb = qd_cost(q, b.x, b.y, b.z);
        if (cb < cost) { p0 = b.x; p1 = b.y; p2 = b.z; cost = cb; }
    }
    ept[3 * e] = p0; ept[3 * e + 1] = p1; ept[3 * e + 2] = p2;
    ecost[e] = cost;
}

// one lane per edge: rules (a) (b) (c) (d) (n) (e), the first refusal counted; the sort key
__global__ void __launch_bounds__(256) qd_valid_kernel(const double *__restrict__ P, const int32_t *__restrict__ fa, er_rings rings, const int *__restrict__ estart,
                                                       const int *__restrict__ sh, const int *__restrict__ eval, const int *__restrict__ vborder,
                                                       const int *__restrict__ vfirst, const int *__restrict__ vlast, const int *__restrict__ vf,
                                                       const double *__restrict__ nref, const double *__restrict__ ept, const double *__restrict__ ecost, int E, double flip2, qd_u64 salt,
                                                       qd_u64 *__restrict__ ekey, qd_u64 *__restrict__ ehash, int *cnt) {
    if (dev_tid() >= E) return;
    const long e = dev_tid();
    const int lo = rings.elo[e], hi = rings.ehi[e], val = eval[e];
    const qd_u64 hash = er_mix(salt, lo, hi);
    ehash[e] = hash;
    int refused = er_refused_abcd(rings, fa, estart, sh, vborder, e, lo, hi, val);
    if (refused >= 0) refused += QD_REF_A;                   // QD_REF_A .. QD_REF_D are consecutive
    const double cost = ecost[e];
    if (refused < 0 && cost != cost) refused = QD_REF_N;
    if (refused < 0 && !er_fans_keep_side(P, fa, vfirst, vlast, vf, nref, lo, hi, {ept[3 * e], ept[3 * e + 1], ept[3 * e + 2]}, flip2)) refused = QD_REF_E;
    if (refused >= 0) { atomicAdd(cnt + refused, 1); ekey[e] = ~0ull; return; }      // an integer count has no order
    atomicAdd(cnt + QD_VALID, 1);
    float c32 = (float)cost;
    if (c32 < 1.17549435e-38f) c32 = 0.0f;
    ekey[e] = ((qd_u64)__float_as_uint(c32) << 32) | (hash & 0xffffffffull);
}

// sorted position i: cand[edge] = i is among the first min(valid, cap)
__global__ void qd_candidates_kernel(const int *__restrict__ erank, int E, const int *__restrict__ cnt, long cap, int *__restrict__ cand) {
    if (dev_tid() >= E) return;
    const long i = dev_tid();
    const long n = cnt[QD_VALID] < cap ? cnt[QD_VALID] : cap;
    cand[erank[i]] = i < n ? 1 : 0;
}

__global__ void qd_select_kernel(const int *__restrict__ erank, int E, const int *__restrict__ cand, const int *__restrict__ elo, const int *__restrict__ ehi,
                                 const int *__restrict__ Mbest, int *__restrict__ sel) {
    if (dev_tid() >= E) return;
    const int e = erank[dev_tid()];
    sel[dev_tid()] = (cand[e] && Mbest[elo[e]] == e && Mbest[ehi[e]] == e) ? 1 : 0;
}

// one lane per sorted position: the selected edges of the lowest `remaining` ranks collapse.  Their end points are pairwise distinct.
__global__ void qd_apply_kernel(const int *__restrict__ erank, int E, const int *__restrict__ sel, const int *__restrict__ selpos, long remaining,
                                const int *__restrict__ elo, const int *__restrict__ ehi, const int *__restrict__ eval, const double *__restrict__ ept,
                                double *__restrict__ P, double *__restrict__ Q, int *__restrict__ rename, int *__restrict__ moved, int *cnt) {
    if (dev_tid() >= E || !sel[dev_tid()] || selpos[dev_tid()] >= remaining) return;
    const long e = erank[dev_tid()];
    const long lo = elo[e], hi = ehi[e];
    rename[hi] = (int)lo;
    moved[lo] = 1;
#pragma unroll
    for (int j = 0; j < 3; ++j) P[3 * lo + j] = ept[3 * e + j];
#pragma unroll
    for (int j = 0; j < 10; ++j) Q[10 * lo + j] = Q[10 * lo + j] + Q[10 * hi + j];
    if (eval[e] == 1) atomicAdd(cnt + QD_BORDER, 1);
}

__global__ void qd_map_hop_kernel(int *__restrict__ vmap, int V, const int *__restrict__ rename) {
    if (dev_tid() < V) vmap[dev_tid()] = rename[vmap[dev_tid()]];
}

__global__ void qd_final_vertices_kernel(const double *__restrict__ vertices, const double *__restrict__ P, const double *__restrict__ c0,
                                       const int *__restrict__ moved, int V, const int *__restrict__ stays, const int *__restrict__ newid,
                                       double *__restrict__ out) {
    if (dev_tid() >= V || !stays[dev_tid()]) return;
    const long v = dev_tid(), n = newid[v];                    // n <= v
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * n + j] = moved[v] ? c0[j] + P[3 * v + j] : vertices[3 * v + j];
}

__global__ void qd_vertex_map_kernel(const int *__restrict__ vmap, int V, const int *__restrict__ part, const int *__restrict__ stays,
                                     const int *__restrict__ newid, int32_t *__restrict__ map) {
    if (dev_tid() >= V) return;
    const int t = vmap[dev_tid()];
    map[dev_tid()] = (part[dev_tid()] && stays[t]) ? newid[t] : -1;
}

}  // namespace surfd

using namespace surfd;

// the arrays of a call, carved from its arena; er_structure (meshrounds.h) sees those of a round through their names
struct qd_arrays {
    int *cnt, *nonfinite, *part, *moved, *vmap, *rename, *mbest, *Mbest, *stays, *newid;
    int *vborder, *vfirst, *vlast, *lfirst, *llast, *hfirst, *hlast;                  // zeroed together every round
    int *vheavy = nullptr;                                   // no slot: the decimation does not ask for the vertices at heavy edges
    int *keep, *kpos, *iota, *sh, *head, *hpos, *eoh, *vf, *estart, *elo, *ehi, *eval, *hie, *erank, *cand, *sel, *selpos;
    unsigned *vkey, *vkeys;
    qd_u64 *box, *hkey, *hkeys, *ehash;
    double *c0, *P, *Q, *ept, *ecost, *nra, *nrb;
    int32_t *fa, *fb;
};

extern "C" int surfd_meshsimplify_decimate(const double *vertices, int V, const int32_t *faces, int F, int64_t target_faces, double border_weight,
                                           double flip_cos, double rank_tol, int spread, int max_rounds, uint64_t seed, double *out_vertices,
                                           int32_t *out_faces, int32_t *vertex_map, int64_t *counts, surfd_stream s) {
    const char *who = "surfd_meshsimplify_decimate";
    if (!counts) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    for (int i = 0; i < 12; ++i) counts[i] = 0;
    SURFD_TRY(mesh_sizes(who, F, V, SURFD_ERR_UNSUPPORTED));
    if (target_faces < 0) SURFD_FAIL(SURFD_ERR_ARG, "%s: target_faces = %lld must not be negative", who, (long long)target_faces);
    if (!(border_weight >= 0.0) || !std::isfinite(border_weight))
        SURFD_FAIL(SURFD_ERR_ARG, "%s: border_weight = %g must be finite and not negative", who, border_weight);
    if (!(flip_cos >= 0.0 && flip_cos < 1.0)) SURFD_FAIL(SURFD_ERR_ARG, "%s: flip_cos = %g must lie in [0, 1)", who, flip_cos);
    if (!(rank_tol > 0.0) || !std::isfinite(rank_tol)) SURFD_FAIL(SURFD_ERR_ARG, "%s: rank_tol = %g must be positive and finite", who, rank_tol);
    if (spread < 1 || max_rounds < 1) SURFD_FAIL(SURFD_ERR_ARG, "%s: spread = %d and max_rounds = %d must be at least 1", who, spread, max_rounds);
    if (V > 0 && !vertices) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    hipStream_t st = as_stream(s);
    if (V > 0 && vertex_map) HIP_TRY(hipMemsetAsync(vertex_map, 0xFF, dev_bytes<int32_t>(V), st));      // -1 everywhere
    if (F == 0 || V == 0) return SURFD_OK;
    if (!faces || !out_vertices || !out_faces) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);

    const long H = 3L * F;                                   // corners; edges are at most as many
    DeviceScratch scratch;
    CubWorkspace cub{&scratch};
    qd_arrays a;
    ScratchArena arena("meshdecimate");
    SURFD_TRY(arena.open(scratch, dev_slot<int>(QD_WORDS) + dev_slot<qd_u64>(6) + dev_slot<double>(3) + 16 * dev_slot<int>(V) + dev_slot<double>(3L * V) +
                                      dev_slot<double>(10L * V) + 2 * dev_slot<int>(F) + 2 * dev_slot<int32_t>(H) + 14 * dev_slot<int>(H) + dev_slot<int>(H + 1) +
                                      2 * dev_slot<unsigned>(H) + 3 * dev_slot<qd_u64>(H) + dev_slot<double>(3 * H) + dev_slot<double>(H) + 2 * dev_slot<double>(H)));
    SURFD_TRY(zeroed_words(arena, &a.cnt, QD_WORDS, st)); SURFD_TRY(arena.get(&a.box, 6)); SURFD_TRY(arena.get(&a.c0, 3));
    SURFD_TRY(arena.get(&a.nonfinite, V)); SURFD_TRY(arena.get(&a.part, V)); SURFD_TRY(arena.get(&a.moved, V)); SURFD_TRY(arena.get(&a.vmap, V));
    SURFD_TRY(arena.get(&a.rename, V)); SURFD_TRY(arena.get(&a.mbest, V)); SURFD_TRY(arena.get(&a.Mbest, V)); SURFD_TRY(arena.get(&a.stays, V));
    SURFD_TRY(arena.get(&a.newid, V));
    SURFD_TRY(arena.get(&a.vborder, V)); SURFD_TRY(arena.get(&a.vfirst, V)); SURFD_TRY(arena.get(&a.vlast, V)); SURFD_TRY(arena.get(&a.lfirst, V));
    SURFD_TRY(arena.get(&a.llast, V)); SURFD_TRY(arena.get(&a.hfirst, V)); SURFD_TRY(arena.get(&a.hlast, V));
    const size_t round_zero = 7 * dev_slot<int>(V);          // vborder .. hlast are consecutive slots
    SURFD_TRY(arena.get(&a.P, 3L * V)); SURFD_TRY(arena.get(&a.Q, 10L * V));
    SURFD_TRY(arena.get(&a.keep, F)); SURFD_TRY(arena.get(&a.kpos, F)); SURFD_TRY(arena.get(&a.fa, H)); SURFD_TRY(arena.get(&a.fb, H));
    SURFD_TRY(arena.get(&a.iota, H)); SURFD_TRY(arena.get(&a.sh, H)); SURFD_TRY(arena.get(&a.head, H)); SURFD_TRY(arena.get(&a.hpos, H));
    SURFD_TRY(arena.get(&a.eoh, H)); SURFD_TRY(arena.get(&a.vf, H)); SURFD_TRY(arena.get(&a.elo, H)); SURFD_TRY(arena.get(&a.ehi, H));
    SURFD_TRY(arena.get(&a.eval, H)); SURFD_TRY(arena.get(&a.hie, H)); SURFD_TRY(arena.get(&a.erank, H)); SURFD_TRY(arena.get(&a.cand, H));
    SURFD_TRY(arena.get(&a.sel, H)); SURFD_TRY(arena.get(&a.selpos, H)); SURFD_TRY(arena.get(&a.estart, H + 1));
    SURFD_TRY(arena.get(&a.vkey, H)); SURFD_TRY(arena.get(&a.vkeys, H));
    SURFD_TRY(arena.get(&a.hkey, H)); SURFD_TRY(arena.get(&a.hkeys, H)); SURFD_TRY(arena.get(&a.ehash, H));
    SURFD_TRY(arena.get(&a.ept, 3 * H)); SURFD_TRY(arena.get(&a.ecost, H)); SURFD_TRY(arena.get(&a.nra, H)); SURFD_TRY(arena.get(&a.nrb, H));
    int *cnt = a.cnt, *live = a.keep, *lpos = a.kpos;        // the flags of a round's faces, once the kept faces are compacted
    qd_u64 *ekey = a.hkey, *ekeys = a.hkeys;                 // the half-edge keys are spent when the candidate keys are made

    HIP_TRY(hipMemsetAsync(a.part, 0, dev_bytes<int>(V), st));
    DEV_LAUNCH(qd_nonfinite_kernel, V, vertices, V, a.nonfinite);
    SURFD_TRY(cub.sort_pairs(a.hkey, a.hkeys, a.iota, a.sh, (int)H, 64, st, true));      // room for the largest sort of the call, before the first scan
    SURFD_TRY(er_kept_faces(cub, faces, F, V, a.nonfinite, a.keep, a.kpos, a.part, cnt + QD_BAD, cnt + QD_KEPT, a.fa, st));
    int hc[QD_WORDS];
    SURFD_TRY(read_words(cnt, hc, QD_WORDS, st));                         // host read 0
    if (hc[QD_BAD]) return mesh_bad_index(who, V);
    int Fn = hc[QD_KEPT];
    HIP_TRY(hipMemsetAsync(a.box, 0xFF, 3 * sizeof(qd_u64), st));
    HIP_TRY(hipMemsetAsync(a.box + 3, 0, 3 * sizeof(qd_u64), st));
    DEV_LAUNCH(qd_box_kernel, V, vertices, V, (const int *)a.part, a.box);
    hipLaunchKernelGGL(qd_centre_kernel, dim3(1), dim3(64), 0, st, (const qd_u64 *)a.box, a.c0);
    LAUNCH_CHECK();
    DEV_LAUNCH(qd_centre_vertices_kernel, V, vertices, V, (const double *)a.c0, a.P, a.vmap, a.rename, a.moved);
    DEV_LAUNCH(er_iota_kernel, H, a.iota, H);
    if (Fn > 0) DEV_LAUNCH(er_face_normals_kernel, Fn, (const double *)a.P, (const int32_t *)a.fa, Fn, a.nra);

    const double flip2 = flip_cos * flip_cos;
    const er_rings rings = {a.elo, a.ehi, a.hie, a.hfirst, a.hlast, a.lfirst, a.llast};
    int rounds = 0, stop = 0;
    int64_t collapses = 0;
    while (Fn > target_faces) {
        if (rounds >= max_rounds) { stop = 2; break; }
        const long remaining = ((long)Fn - target_faces + 1) / 2;
        const long cap = (long)spread * remaining;
        const qd_u64 salt = er_salt(seed, (uint64_t)rounds);
        int E;
        HIP_TRY(hipMemsetAsync(a.vborder, 0, round_zero, st));
        HIP_TRY(hipMemsetAsync(cnt + QD_VALID, 0, (QD_WORDS - QD_VALID) * sizeof(int), st));
        SURFD_TRY(er_structure(a, cub, V, Fn, true, cnt, QD_WORDS, QD_E, hc, &E, st));      // host read 1
        if (rounds == 0)
            DEV_LAUNCH(qd_init_quadrics_kernel, V, (const double *)a.P, (const int32_t *)a.fa, V, (const int *)a.vfirst, (const int *)a.vlast, (const int *)a.vf,
                       (const int *)a.eoh, (const int *)a.eval, border_weight, a.Q);
        DEV_LAUNCH(qd_place_kernel, E, (const double *)a.P, (const double *)a.Q, (const int *)a.elo, (const int *)a.ehi, E, rank_tol, a.ept, a.ecost);
        DEV_LAUNCH(qd_valid_kernel, E, (const double *)a.P, (const int32_t *)a.fa, rings, (const int *)a.estart, (const int *)a.sh, (const int *)a.eval,
                   (const int *)a.vborder, (const int *)a.vfirst, (const int *)a.vlast, (const int *)a.vf, (const double *)a.nra, (const double *)a.ept,
                   (const double *)a.ecost, E, flip2, salt, ekey, a.ehash, cnt);
        SURFD_TRY(cub.sort_pairs(ekey, ekeys, a.iota, a.erank, E, 64, st));
        DEV_LAUNCH(qd_candidates_kernel, E, (const int *)a.erank, E, (const int *)cnt, cap, a.cand);
        DEV_LAUNCH(er_vertex_min_kernel, V, rings, V, (const int *)a.cand, (const qd_u64 *)a.ehash, a.mbest);
        DEV_LAUNCH(er_ring_min_kernel, V, rings, V, (const int *)a.mbest, (const qd_u64 *)a.ehash, a.Mbest);
        DEV_LAUNCH(qd_select_kernel, E, (const int *)a.erank, E, (const int *)a.cand, (const int *)a.elo, (const int *)a.ehi, (const int *)a.Mbest, a.sel);
        SURFD_TRY(cub.exclusive_sum(a.sel, a.selpos, E, st));
        SURFD_TRY(scan_total(a.sel, a.selpos, E, cnt + QD_SEL, st));
        DEV_LAUNCH(qd_apply_kernel, E, (const int *)a.erank, E, (const int *)a.sel, (const int *)a.selpos, remaining, (const int *)a.elo, (const int *)a.ehi,
                   (const int *)a.eval, (const double *)a.ept, a.P, a.Q, a.rename, a.moved, cnt);
        DEV_LAUNCH(er_rename_faces_kernel, Fn, a.fa, Fn, (const int *)a.rename, live);
        SURFD_TRY(cub.exclusive_sum(live, lpos, Fn, st));
        SURFD_TRY(scan_total(live, lpos, Fn, cnt + QD_FNEW, st));
        DEV_LAUNCH(er_compact_live_kernel, Fn, (const int32_t *)a.fa, (const double *)a.nra, Fn, (const int *)live, (const int *)lpos, a.fb, a.nrb);
        DEV_LAUNCH(qd_map_hop_kernel, V, a.vmap, V, (const int *)a.rename);
        SURFD_TRY(read_words(cnt, hc, QD_WORDS, st));                     // host read 2
        ++rounds;
        for (int i = 0; i < 4; ++i) counts[6 + i] = hc[QD_REF_A + i];
        counts[10] = hc[QD_REF_E];
        counts[11] = hc[QD_REF_N];
        const long chosen = hc[QD_SEL] < remaining ? hc[QD_SEL] : remaining;
        if (chosen == 0) { stop = 1; break; }                // fa is what it was: nothing was renamed
        collapses += chosen;
        std::swap(a.fa, a.fb);
        std::swap(a.nra, a.nrb);
        Fn = hc[QD_FNEW];
    }

    SURFD_TRY(er_count_named(cub, a.fa, Fn, V, a.stays, a.newid, cnt + QD_VOUT, st));
    DEV_LAUNCH(qd_final_vertices_kernel, V, vertices, (const double *)a.P, (const double *)a.c0, (const int *)a.moved, V, (const int *)a.stays, (const int *)a.newid,
               out_vertices);
    if (Fn > 0) DEV_LAUNCH(er_out_faces_kernel, 3L * Fn, (const int32_t *)a.fa, 3L * Fn, (const int *)a.newid, out_faces);
    if (vertex_map) DEV_LAUNCH(qd_vertex_map_kernel, V, (const int *)a.vmap, V, (const int *)a.part, (const int *)a.stays, (const int *)a.newid, vertex_map);
    SURFD_TRY(read_words(cnt, hc, QD_WORDS, st));                         // the output size
    counts[0] = hc[QD_VOUT];
    counts[1] = Fn;
    counts[2] = rounds;
    counts[3] = collapses;
    counts[4] = hc[QD_BORDER];
    counts[5] = stop;
    return SURFD_OK;
}
