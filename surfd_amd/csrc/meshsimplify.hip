// Mesh simplification on the device: vertex clustering on a uniform grid (Rossignac-Borrel) with one representative per occupied
// cell, either the mean of the cell's vertices or the minimiser of the cell's plane quadric (Lindstrom).  A sort plus independent
// work per cell: no priority queue and no dependence on a visiting order.  tests/meshsimplify_ref.py restates the contract
// sequentially in numpy and IS the contract: vertices (every double), faces, the map and the counts equal its output bit for bit
// and in the same order.
//
// Contract.  Vertices fp64 [V, 3], faces int32 [F, 3], on the device; cell > 0; origin (host, 3 doubles) or null.
//   kept faces   a face that names a vertex with a NaN or an Inf goes.  A vertex is REFERENCED when a kept face names it; only those
//                take part.
//   cells        origin defaults to the minimum per axis over the referenced vertices, + 0.0 (so a -0.0 and a 0.0 that tie give
//                0.0 whichever the minimum met first).  k = floor((x - origin) / cell) per axis, each operation rounded once.
//                Every k lies in [0, 2^21): anything else (an overflow or a NaN of the arithmetic included) is SURFD_ERR_ARG,
//                never a wrapped key.  key = kx << 42 | ky << 21 | kz.
//   clusters     the distinct keys in ascending order; the members of one in ascending vertex index (a stable sort of (key, index)).
//   mean         s = 0; s = s + x, member by member; mean = s / count.
//   quadric      centre c = origin + (k + 0.5) cell.  Every (kept face, corner) pair, in ascending 3 f + corner, adds to the cluster
//                of that corner, with q_i = p_i - c for the three corners of the face (corner 0 first, whichever corner the record is
//                for): e1 = q1 - q0, e2 = q2 - q0, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x),
//                l = sqrt((nx nx + ny ny) + nz nz); nothing is added where l == 0; otherwise A_ab += (n_a n_b) / l for the six
//                entries (00, 01, 02, 11, 12, 22), d = -((nx q0x + ny q0y) + nz q0z), b_a += (n_a d) / l.
//                A is decomposed by six cyclic Jacobi sweeps (the rotation of csrc/cloudnormals.hip, tests/normals_ref.py:
//                jacobi_f64ops): lambda_j = the diagonal, u_j = column j.  lmax = l0, then l1 and l2 each taken where greater.
//                m = mean - c.  r_a = -(b_a + ((A_a0 m0 + A_a1 m1) + A_a2 m2)).  acc = 0; for j = 0, 1, 2 with lmax > 0 and
//                lambda_j > rank_tol lmax: t = ((u_0j r0 + u_1j r1) + u_2j r2) / lambda_j, acc_a = acc_a + u_aj t.  x = m + acc.
//                x is accepted when it is finite and |x_a - m_a| <= cell for every a: the representative is c + x.  Otherwise
//                the representative is the mean itself and one fall-back is counted.
//   faces        every kept face is renamed through the clusters of its corners; one with two equal names is COLLAPSED and goes;
//                the rest pass through surfd_meshclean_drop_duplicate_faces (one face per set of three names, the lowest face of the
//                class with its own winding, written in ascending (largest, middle, smallest)).
//   compaction   clusters that no output face names go; the others keep their ascending-key order; faces are renumbered.
//   vertex_map   [V]: the output vertex of every input vertex, -1 for a non-finite, unreferenced or removed one.
//   counts       output vertices, output faces, clusters, collapsed faces, duplicate faces, fall-backs (over all clusters).
//
// Passes (256-wide grids, one item per lane unless said; sorts and scans are hipcub's through CubWorkspace):
//   vc_vertex_flags -> face_mark (keep per face, used per vertex; the only kernel that sees caller indices unchecked) ->
//   vc_origin_min (block minimum of an order-preserving integer image of the doubles, then one integer atomicMin per block and
//   axis: a minimum has no order) -> vc_origin_set -> vc_keys (range check; a vertex that takes no part gets 2^63, which no key
//   has) -> stable 64-bit radix sort of (key, vertex) -> run_heads -> exclusive sum -> vc_cluster_of (cluster of every vertex, start
//   of every run) -> vc_face_live (renamed, not collapsed) -> exclusive sums of keep and live -> vc_compact_live -> HOST READ 1:
//   flags, clusters C, kept faces, live faces.
//   vc_mean (one lane per cluster walks its run) -> for quadric: vc_corner_records (3 per kept face, compacted, in ascending
//   3 f + corner) -> stable sort by cluster over ceil(log2 C) bits (C == 1: ZERO bits, no sort is issued: rocPRIM's onesweep writes
//   nothing to its output for an empty bit range, and the records are in order already) -> vc_record_heads -> vc_quadric (one lane
//   per cluster walks its records, then the Jacobi and the point) -> surfd_meshclean_drop_duplicate_faces on the live faces (HOST
//   READ 2, its own) -> vc_mark_named -> exclusive sum -> vc_out_vertices, vc_out_faces, vc_vertex_map -> HOST READ 3: output
//   vertices, fall-backs.  face_mark, run_heads and the non-finite flag are in meshedit.h.
// No float atomics: every sum is one lane's loop in a fixed order.  The one-lane walks cost what their longest run costs: a
// cluster of n members and r records is n + r dependent iterations on one lane (each record gathers 3 indices and 9 doubles)
// while the other 63 lanes of its wave wait; nothing balances lanes of unequal length.
// Scratch (freed when the call returns): 48 V + 28 F bytes before the first read, then 36 C + 12 F_live + (quadric) 48 F_kept,
// each stage in ONE DeviceScratch block (the ScratchArena of devscratch.h, opened once per stage), plus hipcub's workspace and the
// duplicate pass's own 36 F_live.
// Limits: F >= 0, V >= 0 (F = 0 or V = 0: empty outputs, the map all -1); 3 F < 2^31 and V < 2^31, beyond: SURFD_ERR_UNSUPPORTED.
// Bounds: every kernel guards its thread index; arrays of V entries are indexed by caller indices only behind the comparison in
// face_mark (a face that fails it is not kept, and only kept faces are read again) or by library-made values (permutations of
// [0, V), cluster numbers below C <= V, record values 3 f + corner of kept faces); output rows come from exclusive sums of flags.
#include "common.h"
#include "devscratch.h"
#include "meshedit.h"
#include "meshscene.h"
#include <cmath>

namespace surfd {

typedef unsigned long long vc_u64;
constexpr vc_u64 VC_KEY_NONE = 0x8000000000000000ull;        // every key of a vertex that takes part is below 2^63
constexpr int VC_KBITS = 21;
enum { VC_BAD = 0, VC_RANGE = 1, VC_C = 2, VC_KEPT = 3, VC_LIVE = 4, VC_VOUT = 5, VC_FALLBACK = 6, VC_WORDS = 8 };

// an image of the doubles in which unsigned order is numeric order (-0.0 below 0.0; no NaN comes here)
__device__ __forceinline__ vc_u64 vc_ordered(double x) {
    const vc_u64 b = (vc_u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | VC_KEY_NONE);
}
__device__ __forceinline__ double vc_unordered(vc_u64 o) {
    const vc_u64 b = (o >> 63) ? (o & ~VC_KEY_NONE) : ~o;
    return __longlong_as_double((long long)b);
}

__global__ void vc_vertex_flags_kernel(const double *__restrict__ vertices, int V, int *__restrict__ nonfinite) {
    if (dev_tid() >= V) return;
    const long v = dev_tid();
    nonfinite[v] = vertex_nonfinite(vertices, v);
}

// omin[3], preset to all ones: the smallest image per axis over the referenced vertices
__global__ void __launch_bounds__(256) vc_origin_min_kernel(const double *__restrict__ vertices, int V, const int *__restrict__ used, vc_u64 *omin) {
    __shared__ vc_u64 sm[3][256];
    const long v = dev_tid();
    const bool on = v < V && used[v];
#pragma unroll
    for (int j = 0; j < 3; ++j) sm[j][threadIdx.x] = on ? vc_ordered(vertices[3 * v + j]) : ~0ull;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const vc_u64 a = sm[j][threadIdx.x], b = sm[j][threadIdx.x + w];
                sm[j][threadIdx.x] = b < a ? b : a;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 3 && sm[threadIdx.x][0] != ~0ull) atomicMin(omin + threadIdx.x, sm[threadIdx.x][0]);
}

__global__ void vc_origin_set_kernel(const vc_u64 *__restrict__ omin, int given, double ox, double oy, double oz, double *__restrict__ org) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (given) { org[0] = ox; org[1] = oy; org[2] = oz; return; }
#pragma unroll
    for (int j = 0; j < 3; ++j) org[j] = omin[j] == ~0ull ? 0.0 : vc_unordered(omin[j]) + 0.0;      // no referenced vertex: no key is made
}

__global__ void vc_keys_kernel(const double *__restrict__ vertices, int V, const int *__restrict__ used, const double *__restrict__ org, double cell,
                               vc_u64 *__restrict__ key, int *__restrict__ iota, int *__restrict__ cnt) {
    if (dev_tid() >= V) return;
    const long v = dev_tid();
    iota[v] = (int)v;
    vc_u64 k = VC_KEY_NONE;
    if (used[v]) {
        const double kx = floor((vertices[3 * v] - org[0]) / cell), ky = floor((vertices[3 * v + 1] - org[1]) / cell),
                     kz = floor((vertices[3 * v + 2] - org[2]) / cell);
        const double top = (double)(1 << VC_KBITS);
        if (kx >= 0.0 && kx < top && ky >= 0.0 && ky < top && kz >= 0.0 && kz < top)
            k = ((vc_u64)kx << (2 * VC_KBITS)) | ((vc_u64)ky << VC_KBITS) | (vc_u64)kz;
        else
            cnt[VC_RANGE] = 1;                                  // every writer stores the same 1; the vertex keeps the key of no cell
    }
    key[v] = k;
}

__global__ void vc_cluster_of_kernel(const vc_u64 *__restrict__ skey, const int *__restrict__ sidx, const int *__restrict__ head, const int *__restrict__ hpos,
                                     int V, int *__restrict__ cluster_of, int *__restrict__ cstart) {
    if (dev_tid() >= V) return;
    const long i = dev_tid();
    const int v = sidx[i];
    if (skey[i] == VC_KEY_NONE) { cluster_of[v] = -1; return; }
    const int c = hpos[i] + head[i] - 1;                       // the heads up to and including this position, less one
    cluster_of[v] = c;
    if (head[i]) cstart[c] = (int)i;
}

// a kept face names validated, finite, referenced vertices: each has a cluster
__global__ void vc_face_live_kernel(const int32_t *__restrict__ faces, int F, const int *__restrict__ keep, const int *__restrict__ cluster_of,
                                    int *__restrict__ live) {
    if (dev_tid() >= F) return;
    const long f = dev_tid();
    int l = 0;
    if (keep[f]) {
        const int a = cluster_of[faces[3 * f]], b = cluster_of[faces[3 * f + 1]], c = cluster_of[faces[3 * f + 2]];
        l = (a != b && b != c && a != c) ? 1 : 0;
    }
    live[f] = l;
}

__global__ void vc_compact_live_kernel(const int32_t *__restrict__ faces, int F, const int *__restrict__ live, const int *__restrict__ lpos,
                                       const int *__restrict__ cluster_of, int32_t *__restrict__ out) {
    if (dev_tid() >= F || !live[dev_tid()]) return;
    const long f = dev_tid(), n = lpos[f];                     // n <= f
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * n + c] = cluster_of[faces[3 * f + c]];
}

// one lane per cluster: the sum of its members in ascending vertex index
__global__ void vc_mean_kernel(const double *__restrict__ vertices, const vc_u64 *__restrict__ skey, const int *__restrict__ sidx, int V,
                               const int *__restrict__ cstart, int C, double *__restrict__ mean) {
    if (dev_tid() >= C) return;
    const long c = dev_tid();
    long i = cstart[c];
    const vc_u64 k = skey[i];
    double sx = 0.0, sy = 0.0, sz = 0.0, n = 0.0;
    for (; i < V && skey[i] == k; ++i) {
        const long v = sidx[i];
        sx = sx + vertices[3 * v]; sy = sy + vertices[3 * v + 1]; sz = sz + vertices[3 * v + 2];
        n += 1.0;
    }
    mean[3 * c] = sx / n; mean[3 * c + 1] = sy / n; mean[3 * c + 2] = sz / n;
}

__global__ void vc_corner_records_kernel(const int32_t *__restrict__ faces, int F, const int *__restrict__ keep, const int *__restrict__ kpos,
                                         const int *__restrict__ cluster_of, unsigned *__restrict__ rkey, int *__restrict__ rval) {
    if (dev_tid() >= F || !keep[dev_tid()]) return;
    const long f = dev_tid(), n = kpos[f];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        rkey[3 * n + c] = (unsigned)cluster_of[faces[3 * f + c]];
        rval[3 * n + c] = (int)(3 * f + c);
    }
}

__global__ void vc_record_heads_kernel(const unsigned *__restrict__ rkey, int n, int C, int *__restrict__ rstart) {
    if (dev_tid() >= n) return;
    const long i = dev_tid();
    const unsigned k = rkey[i];
    if (k < (unsigned)C && (i == 0 || rkey[i - 1] != k)) rstart[k] = (int)i;
}

// one Jacobi rotation of the pair (p, q); r is the third index (csrc/cloudnormals.hip: cnrm_rotate, kept as a copy so that file's
// code stays as its tests pinned it)
__device__ __forceinline__ void vc_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q, double &v1p,
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

// one lane per cluster: its records in ascending 3 f + corner, then the solve.  rep holds the mean on entry and the representative
// on return.
__global__ void __launch_bounds__(256) vc_quadric_kernel(const double *__restrict__ vertices, const int32_t *__restrict__ faces, const vc_u64 *__restrict__ skey,
                                                         const int *__restrict__ cstart, const unsigned *__restrict__ rkey, const int *__restrict__ rval, int n,
                                                         const int *__restrict__ rstart, int C, const double *__restrict__ org, double cell, double rank_tol,
                                                         double *__restrict__ rep, int *cnt) {
    if (dev_tid() >= C) return;
    const long c = dev_tid();
    const vc_u64 key = skey[cstart[c]];
    const vc_u64 mask = (1ull << VC_KBITS) - 1;
    const double cx = org[0] + ((double)(key >> (2 * VC_KBITS)) + 0.5) * cell, cy = org[1] + ((double)((key >> VC_KBITS) & mask) + 0.5) * cell,
                 cz = org[2] + ((double)(key & mask) + 0.5) * cell;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    long i = rstart[c];
    if (i >= 0) {
        for (; i < n && rkey[i] == (unsigned)c; ++i) {
            const long f = rval[i] / 3;
            const long t0 = faces[3 * f], t1 = faces[3 * f + 1], t2 = faces[3 * f + 2];
            const double q0x = vertices[3 * t0] - cx, q0y = vertices[3 * t0 + 1] - cy, q0z = vertices[3 * t0 + 2] - cz;
            const double q1x = vertices[3 * t1] - cx, q1y = vertices[3 * t1 + 1] - cy, q1z = vertices[3 * t1 + 2] - cz;
            const double q2x = vertices[3 * t2] - cx, q2y = vertices[3 * t2 + 1] - cy, q2z = vertices[3 * t2 + 2] - cz;
            const double ax = q1x - q0x, ay = q1y - q0y, az = q1z - q0z, bx = q2x - q0x, by = q2y - q0y, bz = q2z - q0z;
            const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
            const double l = sqrt((nx * nx + ny * ny) + nz * nz);
            if (l == 0.0) continue;
            a00 = a00 + (nx * nx) / l; a01 = a01 + (nx * ny) / l; a02 = a02 + (nx * nz) / l;
            a11 = a11 + (ny * ny) / l; a12 = a12 + (ny * nz) / l; a22 = a22 + (nz * nz) / l;
            const double d = -((nx * q0x + ny * q0y) + nz * q0z);
            b0 = b0 + (nx * d) / l; b1 = b1 + (ny * d) / l; b2 = b2 + (nz * d) / l;
        }
    }
    const double meanx = rep[3 * c], meany = rep[3 * c + 1], meanz = rep[3 * c + 2];
    const double m0 = meanx - cx, m1 = meany - cy, m2 = meanz - cz;
    const double r0 = -(b0 + ((a00 * m0 + a01 * m1) + a02 * m2)), r1 = -(b1 + ((a01 * m0 + a11 * m1) + a12 * m2)),
                 r2 = -(b2 + ((a02 * m0 + a12 * m1) + a22 * m2));
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // v[row][column]
#pragma unroll 1
    for (int sweep = 0; sweep < 6; ++sweep) {
        vc_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (p, q) = (0, 1), r = 2
        vc_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
        vc_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
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
    const bool ok = isfinite(x0) && isfinite(x1) && isfinite(x2) && fabs(x0 - m0) <= cell && fabs(x1 - m1) <= cell && fabs(x2 - m2) <= cell;
    if (!ok) { atomicAdd(cnt + VC_FALLBACK, 1); return; }      // an integer count has no order; rep keeps the mean
    rep[3 * c] = cx + x0; rep[3 * c + 1] = cy + x1; rep[3 * c + 2] = cz + x2;
}

// names are cluster numbers the library made, below C
__global__ void vc_mark_named_kernel(const int32_t *__restrict__ names, long n, int *__restrict__ named) {
    if (dev_tid() >= n) return;
    named[names[dev_tid()]] = 1;                               // every writer stores the same 1
}

__global__ void vc_out_vertices_kernel(const double *__restrict__ rep, int C, const int *__restrict__ named, const int *__restrict__ newid,
                                       double *__restrict__ out) {
    if (dev_tid() >= C || !named[dev_tid()]) return;
    const long c = dev_tid(), n = newid[c];                    // n <= c < C <= V
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * n + j] = rep[3 * c + j];
}

__global__ void vc_out_faces_kernel(const int32_t *__restrict__ names, long n, const int *__restrict__ newid, int32_t *__restrict__ out) {
    if (dev_tid() >= n) return;
    out[dev_tid()] = newid[names[dev_tid()]];
}

__global__ void vc_vertex_map_kernel(const int *__restrict__ cluster_of, int V, const int *__restrict__ named, const int *__restrict__ newid,
                                     int32_t *__restrict__ map) {
    if (dev_tid() >= V) return;
    const int c = cluster_of[dev_tid()];
    map[dev_tid()] = (c >= 0 && named[c]) ? newid[c] : -1;
}

}  // namespace surfd

using namespace surfd;

extern "C" int surfd_meshsimplify_cluster(const double *vertices, int V, const int32_t *faces, int F, const double *origin, double cell, int representative,
                                          double rank_tol, double *out_vertices, int32_t *out_faces, int32_t *vertex_map, int64_t *counts, surfd_stream s) {
    const char *who = "surfd_meshsimplify_cluster";
    if (!counts) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    for (int i = 0; i < 6; ++i) counts[i] = 0;
    SURFD_TRY(mesh_sizes(who, F, V, SURFD_ERR_UNSUPPORTED));
    if (!(cell > 0.0) || !std::isfinite(cell)) SURFD_FAIL(SURFD_ERR_ARG, "%s: cell = %g must be positive and finite", who, cell);
    if (!(rank_tol > 0.0) || !std::isfinite(rank_tol)) SURFD_FAIL(SURFD_ERR_ARG, "%s: rank_tol = %g must be positive and finite", who, rank_tol);
    if (representative != SURFD_SIMPLIFY_MEAN && representative != SURFD_SIMPLIFY_QUADRIC)
        SURFD_FAIL(SURFD_ERR_ARG, "%s: representative = %d is neither mean (0) nor quadric (1)", who, representative);
    if (origin && !(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2])))
        SURFD_FAIL(SURFD_ERR_ARG, "%s: the origin must be finite", who);
    if (V > 0 && !vertices) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    hipStream_t st = as_stream(s);
    if (V > 0 && vertex_map) HIP_TRY(hipMemsetAsync(vertex_map, 0xFF, dev_bytes<int32_t>(V), st));      // -1 everywhere
    if (F == 0 || V == 0) return SURFD_OK;
    if (!faces || !out_vertices || !out_faces) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);

    DeviceScratch scratch;
    CubWorkspace cub{&scratch};
    int *cnt, *nonfinite, *used, *idxa, *sidx, *head, *hpos, *cluster_of, *cstart, *keep, *kpos, *live, *lpos;
    vc_u64 *key, *skey, *omin;
    double *org;
    int32_t *fbuf;
    ScratchArena arena("meshsimplify");
    SURFD_TRY(arena.open(scratch, dev_slot<int>(VC_WORDS) + dev_slot<vc_u64>(3) + dev_slot<double>(3) + 8 * dev_slot<int>(V) + 2 * dev_slot<vc_u64>(V) +
                                      4 * dev_slot<int>(F) + dev_slot<int32_t>(3L * F)));
    SURFD_TRY(zeroed_words(arena, &cnt, VC_WORDS, st)); SURFD_TRY(arena.get(&omin, 3)); SURFD_TRY(arena.get(&org, 3));
    SURFD_TRY(arena.get(&nonfinite, V)); SURFD_TRY(arena.get(&used, V)); SURFD_TRY(arena.get(&idxa, V)); SURFD_TRY(arena.get(&sidx, V));
    SURFD_TRY(arena.get(&head, V)); SURFD_TRY(arena.get(&hpos, V)); SURFD_TRY(arena.get(&cluster_of, V)); SURFD_TRY(arena.get(&cstart, V));
    SURFD_TRY(arena.get(&key, V)); SURFD_TRY(arena.get(&skey, V));
    SURFD_TRY(arena.get(&keep, F)); SURFD_TRY(arena.get(&kpos, F)); SURFD_TRY(arena.get(&live, F)); SURFD_TRY(arena.get(&lpos, F));
    SURFD_TRY(arena.get(&fbuf, 3L * F));
    HIP_TRY(hipMemsetAsync(omin, 0xFF, 3 * sizeof(vc_u64), st));
    HIP_TRY(hipMemsetAsync(used, 0, dev_bytes<int>(V), st));
    DEV_LAUNCH(vc_vertex_flags_kernel, V, vertices, V, nonfinite);
    DEV_LAUNCH(face_mark_kernel, F, faces, F, V, (const int *)nonfinite, keep, used, cnt + VC_BAD);
    if (!origin) DEV_LAUNCH(vc_origin_min_kernel, V, vertices, V, (const int *)used, omin);
    hipLaunchKernelGGL(vc_origin_set_kernel, dim3(1), dim3(64), 0, st, (const vc_u64 *)omin, origin ? 1 : 0, origin ? origin[0] : 0.0, origin ? origin[1] : 0.0,
                       origin ? origin[2] : 0.0, org);
    LAUNCH_CHECK();
    DEV_LAUNCH(vc_keys_kernel, V, vertices, V, (const int *)used, (const double *)org, cell, key, idxa, cnt);
    SURFD_TRY(cub.sort_pairs(key, skey, idxa, sidx, V, 64, st));
    DEV_LAUNCH(run_heads_kernel<VC_KEY_NONE>, V, (const vc_u64 *)skey, V, head);
    SURFD_TRY(cub.exclusive_sum(head, hpos, V, st));
    SURFD_TRY(scan_total(head, hpos, V, cnt + VC_C, st));
    DEV_LAUNCH(vc_cluster_of_kernel, V, (const vc_u64 *)skey, (const int *)sidx, (const int *)head, (const int *)hpos, V, cluster_of, cstart);
    DEV_LAUNCH(vc_face_live_kernel, F, faces, F, (const int *)keep, (const int *)cluster_of, live);
    SURFD_TRY(cub.exclusive_sum(keep, kpos, F, st));
    SURFD_TRY(scan_total(keep, kpos, F, cnt + VC_KEPT, st));
    SURFD_TRY(cub.exclusive_sum(live, lpos, F, st));
    SURFD_TRY(scan_total(live, lpos, F, cnt + VC_LIVE, st));
    DEV_LAUNCH(vc_compact_live_kernel, F, faces, F, (const int *)live, (const int *)lpos, (const int *)cluster_of, fbuf);
    int hc[VC_WORDS];
    SURFD_TRY(read_words(cnt, hc, VC_WORDS, st));                         // host read 1
    if (hc[VC_BAD]) return mesh_bad_index(who, V);
    if (hc[VC_RANGE])
        SURFD_FAIL(SURFD_ERR_ARG, "%s: a cell index floor((x - origin) / %g) falls outside [0, 2^21): beyond the range of the keys", who, cell);
    const int Cn = hc[VC_C], kept = hc[VC_KEPT], F1 = hc[VC_LIVE];
    counts[2] = Cn;
    counts[3] = (int64_t)kept - F1;
    if (Cn == 0) return SURFD_OK;                            // every face named a non-finite vertex

    const int R = representative == SURFD_SIMPLIFY_QUADRIC ? 3 * kept : 0;
    double *rep;
    int *named, *newid, *rstart, *rval, *rvals;
    unsigned *rkey, *rkeys;
    int32_t *dbuf;
    ScratchArena stage("meshsimplify");
    SURFD_TRY(stage.open(scratch, dev_slot<double>(3L * Cn) + 3 * dev_slot<int>(Cn) + dev_slot<int32_t>(3L * F1) + 2 * dev_slot<int>(R) + 2 * dev_slot<unsigned>(R)));
    SURFD_TRY(stage.get(&rep, 3L * Cn)); SURFD_TRY(stage.get(&named, Cn)); SURFD_TRY(stage.get(&newid, Cn)); SURFD_TRY(stage.get(&rstart, Cn));
    SURFD_TRY(stage.get(&dbuf, 3L * F1));
    SURFD_TRY(stage.get(&rval, R)); SURFD_TRY(stage.get(&rvals, R)); SURFD_TRY(stage.get(&rkey, R)); SURFD_TRY(stage.get(&rkeys, R));
    DEV_LAUNCH(vc_mean_kernel, Cn, vertices, (const vc_u64 *)skey, (const int *)sidx, V, (const int *)cstart, Cn, rep);
    if (representative == SURFD_SIMPLIFY_QUADRIC) {
        DEV_LAUNCH(vc_corner_records_kernel, F, faces, F, (const int *)keep, (const int *)kpos, (const int *)cluster_of, rkey, rval);
        int bits = 0;                                        // of a cluster number below C
        while ((1L << bits) < Cn) ++bits;
        if (bits > 0) SURFD_TRY(cub.sort_pairs(rkey, rkeys, rval, rvals, R, bits, st));
        else { rkeys = rkey; rvals = rval; }                 // one cluster: the records are in order, and a sort over no bits writes nothing
        HIP_TRY(hipMemsetAsync(rstart, 0xFF, dev_bytes<int>(Cn), st));
        DEV_LAUNCH(vc_record_heads_kernel, R, (const unsigned *)rkeys, R, Cn, rstart);
        DEV_LAUNCH(vc_quadric_kernel, Cn, vertices, faces, (const vc_u64 *)skey, (const int *)cstart, (const unsigned *)rkeys, (const int *)rvals, R,
                  (const int *)rstart, Cn, (const double *)org, cell, rank_tol, rep, cnt);
    }
    int64_t F2 = 0;
    if (F1 > 0) SURFD_TRY(surfd_meshclean_drop_duplicate_faces(fbuf, F1, dbuf, &F2, s));      // host read 2 (its own)
    HIP_TRY(hipMemsetAsync(named, 0, dev_bytes<int>(Cn), st));
    if (F2 > 0) DEV_LAUNCH(vc_mark_named_kernel, 3 * F2, (const int32_t *)dbuf, 3L * F2, named);
    SURFD_TRY(cub.exclusive_sum(named, newid, Cn, st));
    SURFD_TRY(scan_total(named, newid, Cn, cnt + VC_VOUT, st));
    DEV_LAUNCH(vc_out_vertices_kernel, Cn, (const double *)rep, Cn, (const int *)named, (const int *)newid, out_vertices);
    if (F2 > 0) DEV_LAUNCH(vc_out_faces_kernel, 3 * F2, (const int32_t *)dbuf, 3L * F2, (const int *)newid, out_faces);
    if (vertex_map) DEV_LAUNCH(vc_vertex_map_kernel, V, (const int *)cluster_of, V, (const int *)named, (const int *)newid, vertex_map);
    SURFD_TRY(read_words(cnt, hc, VC_WORDS, st));                         // host read 3
    counts[0] = hc[VC_VOUT];
    counts[1] = F2;
    counts[4] = (int64_t)F1 - F2;
    counts[5] = hc[VC_FALLBACK];
    return SURFD_OK;
}
