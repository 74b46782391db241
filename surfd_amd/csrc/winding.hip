// Generalized winding numbers of a triangle mesh (Jacobson, Kavan and Sorkine-Hornung, Robust Inside-Outside Segmentation using
// Generalized Winding Numbers, SIGGRAPH 2013): w(p) = the signed solid angle of the mesh seen from p, divided by 4 pi.  1 inside
// and 0 outside a closed, consistently oriented mesh; a hole costs only its own solid angle, so |w| >= 1/2 still tells inside
// from outside where the parity of ray crossings (raycast.hip, voxel.hip) flips a whole cone or column.  What libigl calls
// winding_number.  No reference counterpart (the reference takes its signs from open3d's crossing parity).  fp32 in, fp64 pair
// arithmetic on the VALU, no MFMA, no atomics except the integer ones of create's checks.
//
// The contract, restated decision for decision in tests/winding_ref.py.  Every operation is ONE fp64
// IEEE rounding (the library is built with -ffp-contract=off; nothing here is an fma).
//   term     query p, triangle (A, B, C) in the caller's corner order:
//            a = A - p, b = B - p, c = C - p, both operands converted to fp64 first;
//            la = sqrt((a.x a.x + a.y a.y) + a.z a.z), lb, lc likewise;
//            det = (a.x (b.y c.z - b.z c.y) + a.y (b.z c.x - b.x c.z)) + a.z (b.x c.y - b.y c.x);
//            ab = (a.x b.x + a.y b.y) + a.z b.z, bc, ca likewise;
//            den = ((la lb) lc + ab lc) + (bc la + ca lb);
//            theta = atan2(det, den), and theta = +0 when det == 0 (a query in the triangle's plane, a triangle without area, a
//            query on a vertex: the principal value; the sign of a zero never chooses between +pi and -pi).
//            This is van Oosterom and Strackee's formula; 2 theta is the signed solid angle.  + - * sqrt are correctly rounded
//            on the device and in numpy, so det and den have the same bits in both; atan2 is the only operation that may differ.
//   sum      a fixed function of F alone, never of Q, the launch geometry, the number of splits or a query's place in its call.
//            Triangles in the caller's order (nothing is sorted: there is nothing to cull).  A chunk is 256 consecutive
//            triangles, s_c = the left-to-right sum of its theta from +0.  A group is 16 consecutive chunks (4 096 triangles),
//            S_g = the left-to-right sum of its s_c from +0.  Theta = the left-to-right sum of the S_g from +0.
//            w = Theta / 6.283185307179586 (0x401921FB54442D18).  A split of the triangle range owns whole groups.
//   special  a query that holds a NaN or an Inf: w = NaN (its coordinates are never used).  An index outside [0, V) or a vertex
//            that is not finite: create fails with SURFD_ERR_ARG, found on the device and read back as a flag.
// w depends on the orientation: reversing every triangle negates it, and a mesh whose faces are not consistently oriented gives
// values that mean nothing.
//
// Kernels:
//   wn_check_kernel    one thread per vertex: counts the vertices that are not finite.
//   wn_gather_kernel   one thread per triangle: nine fp32 (A, B, C) in the order given; an index outside [0, V) raises a flag.
//   wn_kernel          one query per lane (three doubles in registers), 256 lanes per workgroup.  A chunk of 256 triangles is
//                      staged in LDS (9 KiB); all lanes of a wave read the same triangle at the same time (a broadcast).  grid.y
//                      splits the groups, so that a call with few queries and many faces still fills the chip.  The partial S_g
//                      of every (group, query) goes to the handle's workspace.
//   wn_finish_kernel   one thread per query: adds the S_g in ascending order, divides, writes NaN for a query that is not finite.
// The library walks the queries in slabs so that the workspace stays at or below 256 MiB; lanes are independent, so slab
// boundaries cannot change a bit.
//
// Bounds.  Vertex v < V reads vertices[3 v .. 3 v + 2].  Triangle f < F reads triangles[3 f .. 3 f + 2], reads vertices at an
// index clamped into [0, V) and writes rec[9 f .. 9 f + 8].  In wn_kernel lane n >= Q reads query Q - 1 and writes nothing; group
// g < ngroup, chunk c < nchunk = ceil(F / 256) with c < 16 (g + 1); staging reads rec[9 (256 c) + e] for e < 9 cnt with
// 256 c + cnt <= F, so the index is below 9 F <= 3 (2^31 - 1) and is formed in 64 bits; LDS is indexed with 9 u + 8 < 9 cnt <= 2304;
// the workspace with g Q + n < ngroup Q (64 bits), Q the slab's query count, and it holds ngroup * slab doubles with Q <= slab.
// wn_finish_kernel reads the same range and points[3 n .. 3 n + 2], writes w[n], n < Q.  Hazards: the LDS chunk is bracketed by a
// barrier on both sides.  No workgroup waits for another.  Partial results live in the handle's arena (meshscene.h).
//
// ---- The fast path (surfd_winding_build_bvh, surfd_winding_eval_fast) ------------------------------------
// Opt-in, and an APPROXIMATION: a part of the mesh that is far from the query is replaced by one dipole (the first term of
// Barill et al., Fast Winding Numbers for Soups and Clouds, SIGGRAPH 2018).  The cost per query is logarithmic in F.  The exact
// path above is untouched.  The contract, restated decision for decision in tests/winding_fast_ref.py; every operation is one
// fp64 rounding on fp32 input converted first, only + - * / sqrt outside wn_theta:
//   tree     the hierarchy of meshbvh.hip over the handle's triangles: absolute corners, Morton order, leaves of 4, its boxes.
//            bvh_build reads float4 records a, b, c: fwn_rec4_kernel copies the nine floats of every triangle into such records
//            in a scratch buffer that lives for the build only; rec and its order stay as they are.
//   moments  triangle (A, B, C) in the caller's corner order, u = B - A, v = C - A:
//            n = 0.5 (u x v), n.x = 0.5 (u.y v.z - u.z v.y), n.y = 0.5 (u.z v.x - u.x v.z), n.z = 0.5 (u.x v.y - u.y v.x);
//            a = sqrt((n.x n.x + n.y n.y) + n.z n.z);  c = ((A + B) + C) / 3.
//   sums     of an entry (a leaf or a node): (sum a, sum a c [3], sum n [3]), seven doubles.  A leaf adds its triangles in slot
//            order, left to right from +0, empty slots (-1) skipped, the product a c.x formed first.  A node adds the sums of its
//            existing children in ascending order, left to right from +0.  Hierarchical: never recomputed from the triangles.
//   record   of an entry, kept in slot c of its parent: (p.x, p.y, p.z, N.x, N.y, N.z, R2).  p = sum a c / sum a where sum a > 0,
//            else (lo + hi) 0.5 of the entry's fp32 box;  N = sum n;  R2 = (m.x m.x + m.y m.y) + m.z m.z with
//            m.j = (p.j - lo.j) > (hi.j - p.j) ? (p.j - lo.j) : (hi.j - p.j): the squared distance from p to the farthest corner
//            of the box.  A box that meshbvh.hip stores as (-inf, +inf) gives R2 = +inf: never approximated.  An absent child
//            slot (past the end of a level) is (0, 0, 0, 0, 0, 0, -1): no squared radius is negative.  The root has no record.
//   walk     of a finite query p: bvh_next / bvh_enter from the root; all four slots of a node wait when it is entered and are
//            taken in ascending order.  For the slot taken: R2 < 0: nothing.  r = p~ - p, d2 = (r.x r.x + r.y r.y) + r.z r.z.
//            d2 > (beta beta) R2: S = S + (((N.x r.x + N.y r.y) + N.z r.z) / (d2 sqrt(d2))) 0.5, the dipole in units of theta,
//            and no descent.  Otherwise (a NaN compares false) descend; in a leaf S = S + wn_theta of its triangles in slot
//            order.  One running sum per query from +0, w = S / 6.283185307179586.  A query with a NaN or an Inf: w = NaN.
//   beta     a finite double >= 1, or +inf (every triangle exactly, in Morton order); anything else is SURFD_ERR_ARG before any
//            launch.  beta beta is formed on the host.  With beta >= 1 the strict inequality gives d2 > R2 >= 0, so d > 0.
// The bits of w[n] depend on the query, the mesh and beta alone: a lane's walk and sum are its own.  No floating-point atomics.
//
// Kernels of the fast path:
//   fwn_rec4_kernel    one thread per triangle: rec[9 f ..] -> three float4 (the fourth component 0).
//   fwn_leaf_kernel    one thread per leaf: its sums from its triangles, its record into its level-0 node.
//   fwn_level_kernel   one launch per level, bottom-up, one thread per node: its sums from the entries below, and (but for the
//                      root) its record into its parent.  The thread of a level's last entry also writes the absent slots that
//                      follow it in its parent.
//   fwn_walk_kernel    one query per lane (three doubles, the running sum and the walk's 64-bit mask in registers), 256 lanes
//                      per workgroup; lanes diverge, nothing is shared but the 16 level offsets in LDS.
// Bounds.  fwn_rec4: f < F reads rec[9 f .. 9 f + 8], writes rec4[3 f .. 3 f + 2].  fwn_leaf: leaf i < nleaf reads leaf_tri[i],
// rec[9 f ..] for 0 <= f < F only, the box of slot i % 4 of node i / 4 < size[0] (boxes index (i / 4) 6 + j, j < 6), writes
// sums[7 i ..] and recs[8 (4 (i / 4) + i % 4) ..]; the last leaf also the slots i % 4 + 1 .. 3 of the same node.  fwn_level at
// level k: node n < size[k] reads the sums of the entries 4 n .. 4 n + cnt - 1, cnt = bvh_child_count(below, n), writes sums at
// 7 (nleaf + off[k] + n) (the sums array holds nleaf + nodes entries) and, where k < top, slot n % 4 of node
// off[k + 1] + n / 4 < nodes, reading that slot's box.  fwn_walk: lane n >= Q reads query Q - 1 and writes nothing; it takes slot
// child = 4 node + c with node < size[level], so the record index off[level] 4 + child < 4 nodes (recs holds 4 nodes records of
// 8 doubles); a leaf is entered only through a record that exists, so child < nleaf; a triangle index outside [0, F) is not read.
// Hazards: LDS is written once before one barrier.  No workgroup waits for another.
#include "common.h"
#include "meshscene.h"
#include "meshbvh.h"
#include <cmath>
#include <algorithm>

namespace surfd {

constexpr int WN_CHUNK = 256;                     // triangles per LDS chunk, and queries per workgroup
constexpr int WN_GROUP_CHUNKS = 16;               // chunks per group: the unit a split owns (tests/winding_ref.py restates it)
constexpr int WN_REC = 9;                         // fp32 per triangle: A, B, C
constexpr size_t WN_WS_MAX = (size_t)256 << 20;   // bytes of partial sums a call may hold
constexpr double WN_TWO_PI = 6.283185307179586;   // 0x401921FB54442D18

__device__ __forceinline__ bool wn_finite(float x) { return x - x == 0.f; }

// the term of one (query, triangle) pair
__device__ __forceinline__ double wn_theta(double px, double py, double pz, const float *__restrict__ t) {
    const double ax = (double)t[0] - px, ay = (double)t[1] - py, az = (double)t[2] - pz;
    const double bx = (double)t[3] - px, by = (double)t[4] - py, bz = (double)t[5] - pz;
    const double cx = (double)t[6] - px, cy = (double)t[7] - py, cz = (double)t[8] - pz;
    const double la = __builtin_sqrt((ax * ax + ay * ay) + az * az);
    const double lb = __builtin_sqrt((bx * bx + by * by) + bz * bz);
    const double lc = __builtin_sqrt((cx * cx + cy * cy) + cz * cz);
    const double det = (ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz)) + az * (bx * cy - by * cx);
    const double ab = (ax * bx + ay * by) + az * bz;
    const double bc = (bx * cx + by * cy) + bz * cz;
    const double ca = (cx * ax + cy * ay) + cz * az;
    const double den = ((la * lb) * lc + ab * lc) + (bc * la + ca * lb);
    return det == 0.0 ? 0.0 : atan2(det, den);
}

// one thread per vertex
__global__ __launch_bounds__(256) void wn_check_kernel(const float *__restrict__ vtx, int V, int *__restrict__ bad) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    if (!(wn_finite(vtx[(long)v * 3]) && wn_finite(vtx[(long)v * 3 + 1]) && wn_finite(vtx[(long)v * 3 + 2]))) atomicAdd(bad, 1);
}

// one thread per triangle
__global__ __launch_bounds__(256) void wn_gather_kernel(const float *__restrict__ vtx, int V, const int *__restrict__ tri, int F,
                                                        float *__restrict__ rec, int *__restrict__ bad) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int k = tri[(long)f * 3 + c];
        if (k < 0 || k >= V) { atomicOr(bad, 1); k = 0; }
#pragma unroll
        for (int d = 0; d < 3; ++d) rec[(long)f * WN_REC + 3 * c + d] = vtx[(long)k * 3 + d];
    }
}

// points [Q, 3]; split blockIdx.y covers the groups [y * gspan, min(ngroup, (y + 1) * gspan)); partial sums ws [ngroup, Q]
__global__ __launch_bounds__(256) void wn_kernel(const float *__restrict__ rec, int F, int nchunk, int ngroup, int gspan,
                                                 const float *__restrict__ points, int Q, double *__restrict__ ws) {
    __shared__ float lds[WN_CHUNK * WN_REC];
    const int tid = threadIdx.x;
    const int n = blockIdx.x * WN_CHUNK + tid;
    const long nr = n < Q ? n : Q - 1;
    float fx = points[nr * 3], fy = points[nr * 3 + 1], fz = points[nr * 3 + 2];
    if (!(wn_finite(fx) && wn_finite(fy) && wn_finite(fz))) fx = fy = fz = 0.f;      // the finish writes a NaN for this query
    const double px = (double)fx, py = (double)fy, pz = (double)fz;
    const int g0 = blockIdx.y * gspan, g1 = min(ngroup, g0 + gspan);
#pragma unroll 1
    for (int g = g0; g < g1; ++g) {
        double S = 0.0;
        const int c0 = g * WN_GROUP_CHUNKS, c1 = min(nchunk, c0 + WN_GROUP_CHUNKS);
#pragma unroll 1
        for (int c = c0; c < c1; ++c) {
            const int f0 = c * WN_CHUNK;
            const int cnt = min(WN_CHUNK, F - f0);
            __syncthreads();                                 // every lane is done with the previous chunk
#pragma unroll
            for (int i = 0; i < WN_REC; ++i) {
                const int e = tid + 256 * i;
                if (e < cnt * WN_REC) lds[e] = rec[(long)f0 * WN_REC + e];
            }
            __syncthreads();
            double s = 0.0;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int u = 0; u < cnt; ++u) s = s + wn_theta(px, py, pz, &lds[u * WN_REC]);
            S = S + s;
        }
        if (n < Q) ws[(long)g * Q + n] = S;
    }
}

__global__ __launch_bounds__(256) void wn_finish_kernel(const double *__restrict__ ws, int ngroup, const float *__restrict__ points, int Q,
                                                        double *__restrict__ w) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= Q) return;
    double T = 0.0;
    for (int g = 0; g < ngroup; ++g) T = T + ws[(long)g * Q + n];
    const bool ok = wn_finite(points[(long)n * 3]) && wn_finite(points[(long)n * 3 + 1]) && wn_finite(points[(long)n * 3 + 2]);
    w[n] = ok ? T / WN_TWO_PI : __builtin_nan("");
}

// ---- the fast path --------------------------------------------------------------------------------------------------------------
constexpr int FWN_SUMS = 7;                       // doubles per entry: sum a, sum a c [3], sum n [3]
constexpr int FWN_REC = 8;                        // doubles per record: p [3], N [3], R2 and one that is never read (64-byte records)
constexpr int FWN_REC_USED = 7;                   // what surfd_winding_bvh_read hands out

struct FwnSums {
    double v[FWN_SUMS];
};

// one thread per triangle: the float4 records bvh_build reads
__global__ __launch_bounds__(256) void fwn_rec4_kernel(const float *__restrict__ rec, int F, float4 *__restrict__ rec4) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const float *t = rec + (long)f * WN_REC;
#pragma unroll
    for (int k = 0; k < 3; ++k) rec4[(long)f * 3 + k] = make_float4(t[3 * k], t[3 * k + 1], t[3 * k + 2], 0.f);
}

// the record of the entry with sums s in slot c of node `node` (an index into the whole node array), whose box is read there
__device__ __forceinline__ void fwn_store_record(const FwnSums &s, const float4 *__restrict__ boxes, long node, int c, double *__restrict__ recs) {
    double *out = recs + (node * BVH_W + c) * FWN_REC;
    double m2[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double lo = (double)bvh_comp(boxes[node * BVH_BOX4 + j], c), hi = (double)bvh_comp(boxes[node * BVH_BOX4 + 3 + j], c);
        const double p = s.v[0] > 0.0 ? s.v[1 + j] / s.v[0] : (lo + hi) * 0.5;
        const double below = p - lo, above = hi - p;
        const double m = below > above ? below : above;
        m2[j] = m * m;
        out[j] = p;
        out[3 + j] = s.v[4 + j];
    }
    out[6] = (m2[0] + m2[1]) + m2[2];
    out[7] = 0.0;
}

// the slots after c of node `node` hold nothing
__device__ __forceinline__ void fwn_store_absent(long node, int c, double *__restrict__ recs) {
    for (int k = c + 1; k < BVH_W; ++k) {
        double *out = recs + (node * BVH_W + k) * FWN_REC;
#pragma unroll
        for (int e = 0; e < FWN_REC; ++e) out[e] = e == 6 ? -1.0 : 0.0;
    }
}

// one thread per leaf; boxes: level 0
__global__ __launch_bounds__(256) void fwn_leaf_kernel(const float *__restrict__ rec, int F, const int4 *__restrict__ leaf_tri, int nleaf,
                                                       const float4 *__restrict__ boxes, double *__restrict__ sums, double *__restrict__ recs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nleaf) return;
    const int4 ids = leaf_tri[i];
    FwnSums s;
#pragma unroll
    for (int e = 0; e < FWN_SUMS; ++e) s.v[e] = 0.0;
#pragma unroll
    for (int k = 0; k < BVH_L; ++k) {
        const int f = bvh_comp(ids, k);
        if ((unsigned)f >= (unsigned)F) continue;
        const float *t = rec + (long)f * WN_REC;
        const double ax = (double)t[0], ay = (double)t[1], az = (double)t[2];
        const double bx = (double)t[3], by = (double)t[4], bz = (double)t[5];
        const double cx = (double)t[6], cy = (double)t[7], cz = (double)t[8];
        const double ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
        const double nx = 0.5 * (uy * vz - uz * vy), ny = 0.5 * (uz * vx - ux * vz), nz = 0.5 * (ux * vy - uy * vx);
        const double a = __builtin_sqrt((nx * nx + ny * ny) + nz * nz);
        const double gx = ((ax + bx) + cx) / 3.0, gy = ((ay + by) + cy) / 3.0, gz = ((az + bz) + cz) / 3.0;
        s.v[0] = s.v[0] + a;
        s.v[1] = s.v[1] + a * gx; s.v[2] = s.v[2] + a * gy; s.v[3] = s.v[3] + a * gz;
        s.v[4] = s.v[4] + nx; s.v[5] = s.v[5] + ny; s.v[6] = s.v[6] + nz;
    }
#pragma unroll
    for (int e = 0; e < FWN_SUMS; ++e) sums[(long)i * FWN_SUMS + e] = s.v[e];
    fwn_store_record(s, boxes, i / BVH_W, i % BVH_W, recs);
    if (i == nleaf - 1) fwn_store_absent(i / BVH_W, i % BVH_W, recs);
}

// one thread per node of a level: below = the sums of the nbelow entries under the level, out = the sums of its nnode nodes;
// parent (the index of the level above in the node array) < 0 for the root's level
__global__ __launch_bounds__(256) void fwn_level_kernel(const double *__restrict__ below, int nbelow, double *__restrict__ out, int nnode,
                                                        const float4 *__restrict__ boxes, long parent, double *__restrict__ recs) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= nnode) return;
    const int cnt = bvh_child_count(nbelow, n);
    FwnSums s;
#pragma unroll
    for (int e = 0; e < FWN_SUMS; ++e) s.v[e] = 0.0;
    for (int c = 0; c < cnt; ++c) {
#pragma unroll
        for (int e = 0; e < FWN_SUMS; ++e) s.v[e] = s.v[e] + below[((long)n * BVH_W + c) * FWN_SUMS + e];
    }
#pragma unroll
    for (int e = 0; e < FWN_SUMS; ++e) out[(long)n * FWN_SUMS + e] = s.v[e];
    if (parent < 0) return;
    fwn_store_record(s, boxes, parent + n / BVH_W, n % BVH_W, recs);
    if (n == nnode - 1) fwn_store_absent(parent + n / BVH_W, n % BVH_W, recs);
}

// points [Q, 3] -> w [Q]; bb = beta beta; visits: null, or two counters (cluster terms, triangle terms)
__global__ __launch_bounds__(256) void fwn_walk_kernel(const float *__restrict__ rec, int F, const double *__restrict__ recs,
                                                       const int4 *__restrict__ leaf_tri, const int *__restrict__ level_off, int top,
                                                       const float *__restrict__ points, int Q, double bb, double *__restrict__ w,
                                                       unsigned long long *__restrict__ visits) {
    __shared__ int off[BVH_MAX_LEVELS];
    const int tid = threadIdx.x;
    if (tid < BVH_MAX_LEVELS) off[tid] = level_off[tid];
    __syncthreads();
    const int n = blockIdx.x * 256 + tid;
    const long nr = n < Q ? n : Q - 1;
    const float fx = points[nr * 3], fy = points[nr * 3 + 1], fz = points[nr * 3 + 2];
    const bool live = n < Q && wn_finite(fx) && wn_finite(fy) && wn_finite(fz);
    const double px = (double)fx, py = (double)fy, pz = (double)fz;
    double S = 0.0;
    unsigned ncluster = 0, ntri = 0;
    int level = top;
    unsigned node = 0, child = 0;
    unsigned long long mask = live ? bvh_mask_bits(top, 15u) : 0ull;
#pragma unroll 1
    while (bvh_next(top, level, node, mask, child)) {
        const double *e = recs + ((long)off[level] * BVH_W + (long)child) * FWN_REC;
        const double R2 = e[6];
        if (R2 < 0.0) continue;                                    // an absent slot
        const double rx = e[0] - px, ry = e[1] - py, rz = e[2] - pz;
        const double d2 = (rx * rx + ry * ry) + rz * rz;
        if (d2 > bb * R2) {
            S = S + (((e[3] * rx + e[4] * ry) + e[5] * rz) / (d2 * __builtin_sqrt(d2))) * 0.5;
            ncluster += 1;
            continue;
        }
        if (level > 0) {
            bvh_enter(level, node, child);
            mask |= bvh_mask_bits(level, 15u);
            continue;
        }
        const int4 ids = leaf_tri[child];
#pragma unroll 1
        for (int i = 0; i < BVH_L; ++i) {
            const int f = bvh_comp(ids, i);
            if ((unsigned)f >= (unsigned)F) continue;              // -1: the last leaf has fewer than L triangles
            S = S + wn_theta(px, py, pz, rec + (long)f * WN_REC);
            ntri += 1;
        }
    }
    if (n < Q) w[n] = live ? S / WN_TWO_PI : __builtin_nan("");
    if (visits) bvh_count_visits(visits, ncluster, ntri, tid & 63);
}

}  // namespace surfd

using namespace surfd;

struct surfd_winding {
    int F = 0, nchunk = 0, ngroup = 0;
    float *rec = nullptr;             // [F] triangles of 9 fp32
    DeviceArena ws;                   // partial sums [ngroup, slab]
    MeshBvh bvh;                      // the hierarchy of surfd_winding_build_bvh (meshbvh.hip)
    double *recs = nullptr;           // [bvh.lay.nodes][BVH_W] records of FWN_REC doubles; set once the build is complete
};

// queries per slab: as many as keep ngroup * slab doubles within WN_WS_MAX, in whole workgroups where that leaves one (whole waves
// otherwise: ngroup <= 174 763 for 3 F < 2^31, and 174 763 * 64 * 8 bytes is 85 MiB)
static long wn_slab(int ngroup) {
    const long fit = (long)(WN_WS_MAX / (sizeof(double) * (size_t)ngroup));
    return fit >= WN_CHUNK ? fit / WN_CHUNK * WN_CHUNK : std::max<long>(64, fit / 64 * 64);
}

extern "C" {

int surfd_winding_create(const float *vertices, int V, const int32_t *triangles, int F, surfd_stream s, surfd_winding **out) {
    int rc = mesh_create_args("surfd_winding_create", vertices, V, triangles, F, out, INT_MAX);  // the size test below is this file's
    if (rc != SURFD_OK) return rc;
    if ((long long)F * 3 >= (1ll << 31)) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_create: F = %d: 3 F must stay below 2^31", F);
    hipStream_t st = as_stream(s);
    surfd_winding *m = new surfd_winding();
    m->F = F;
    m->nchunk = ceil_div(F, WN_CHUNK);
    m->ngroup = ceil_div(m->nchunk, WN_GROUP_CHUNKS);
    CreateFlags bad(2);                                       // [0] vertices that are not finite, [1] bad indices
    int flag[2] = {0, 0};
    auto run = [&]() -> int {
        HIP_TRY(hipMalloc(&m->rec, (size_t)F * WN_REC * sizeof(float)));
        if (int e = bad.init(st)) return e;
        hipLaunchKernelGGL(wn_check_kernel, dim3((unsigned)ceil_div(V, 256)), dim3(256), 0, st, vertices, V, bad.dev);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(wn_gather_kernel, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, st, vertices, V, triangles, F, m->rec, bad.dev + 1);
        LAUNCH_CHECK();
        return bad.read(flag, st);
    };
    rc = run();
    if (rc == SURFD_OK && flag[0]) {
        set_error("surfd_winding_create: %d of %d vertices hold a NaN or an Inf", flag[0], V);
        rc = SURFD_ERR_ARG;
    } else if (rc == SURFD_OK && flag[1]) {
        rc = mesh_bad_index("surfd_winding_create", V);
    }
    if (rc != SURFD_OK) { surfd_winding_destroy(m); return rc; }
    *out = m;
    return SURFD_OK;
}

void surfd_winding_destroy(surfd_winding *m) {
    if (!m) return;
    (void)hipFree(m->rec);
    (void)hipFree(m->recs);
    bvh_free(&m->bvh);
    m->ws.release();
    delete m;
}

int surfd_winding_num_triangles(const surfd_winding *m) { return m ? m->F : 0; }

int surfd_winding_eval(surfd_winding *m, const float *points, int64_t Q, int flags, double *w, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_eval: null handle");
    if (Q < 0 || Q >= (1ll << 31)) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_eval: Q = %lld must lie in [0, 2^31)", (long long)Q);
    if (flags & ~SURFD_WINDING_ONE_SPLIT) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_eval: unknown flags 0x%x", flags);
    if (Q == 0) return SURFD_OK;
    if (!points || !w) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_eval: null points or output");
    hipStream_t st = as_stream(s);
    const long slab = wn_slab(m->ngroup);
    int rc;
    if ((rc = m->ws.reserve((size_t)m->ngroup * (size_t)std::min<long>(slab, (long)Q) * sizeof(double), st))) return rc;
    for (long q0 = 0; q0 < Q; q0 += slab) {
        const int Qs = (int)std::min<long>(slab, (long)Q - q0);
        // splits of the group range per block of queries; 65535: the most a grid has along y
        const Split sp = split_units(Qs, WN_CHUNK, m->ngroup, 65535, (flags & SURFD_WINDING_ONE_SPLIT) ? 1 : 2048);
        hipLaunchKernelGGL(wn_kernel, dim3((unsigned)ceil_div(Qs, WN_CHUNK), (unsigned)sp.S), dim3(256), 0, st, (const float *)m->rec, m->F,
                           m->nchunk, m->ngroup, sp.span, points + q0 * 3, Qs, (double *)m->ws.ptr);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(wn_finish_kernel, dim3((unsigned)ceil_div(Qs, 256)), dim3(256), 0, st, (const double *)m->ws.ptr, m->ngroup,
                           points + q0 * 3, Qs, w + q0);
        LAUNCH_CHECK();
    }
    return SURFD_OK;
}

int surfd_winding_build_bvh(surfd_winding *m, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_build_bvh: null handle");
    if (m->recs) return SURFD_OK;
    hipStream_t st = as_stream(s);
    int rc;
    if (!m->bvh.built) {
        float4 *rec4 = nullptr;                                   // what bvh_build reads, for the build only
        auto tree = [&]() -> int {
            HIP_TRY(hipMalloc(&rec4, (size_t)m->F * 3 * sizeof(float4)));
            hipLaunchKernelGGL(fwn_rec4_kernel, dim3((unsigned)ceil_div(m->F, 256)), dim3(256), 0, st, (const float *)m->rec, m->F, rec4);
            LAUNCH_CHECK();
            return bvh_build(&m->bvh, rec4, 3, false, m->F, st);   // syncs the stream before it returns
        };
        rc = tree();
        (void)hipFree(rec4);                                      // after a refusal hipFree waits for the device itself
        if (rc != SURFD_OK) return rc;
    }
    const BvhLayout &lay = m->bvh.lay;
    double *sums = nullptr, *recs = nullptr;
    auto run = [&]() -> int {
        HIP_TRY(hipMalloc(&sums, ((size_t)lay.nleaf + (size_t)lay.nodes) * FWN_SUMS * sizeof(double)));
        HIP_TRY(hipMalloc(&recs, (size_t)lay.nodes * BVH_W * FWN_REC * sizeof(double)));
        hipLaunchKernelGGL(fwn_leaf_kernel, dim3((unsigned)ceil_div(lay.nleaf, 256)), dim3(256), 0, st, (const float *)m->rec, m->F,
                           (const int4 *)m->bvh.leaf_tri, lay.nleaf, (const float4 *)m->bvh.boxes, sums, recs);
        LAUNCH_CHECK();
        for (int k = 0; k < lay.levels; ++k) {
            const double *below = k == 0 ? sums : sums + ((size_t)lay.nleaf + (size_t)lay.off[k - 1]) * FWN_SUMS;
            hipLaunchKernelGGL(fwn_level_kernel, dim3((unsigned)ceil_div(lay.size[k], 256)), dim3(256), 0, st, below, bvh_below(lay, k),
                               sums + ((size_t)lay.nleaf + (size_t)lay.off[k]) * FWN_SUMS, lay.size[k], (const float4 *)m->bvh.boxes,
                               k + 1 < lay.levels ? (long)lay.off[k + 1] : -1l, recs);
            LAUNCH_CHECK();
        }
        HIP_TRY(hipStreamSynchronize(st));                        // the sums are freed next
        return SURFD_OK;
    };
    rc = run();
    (void)hipFree(sums);
    if (rc != SURFD_OK) { (void)hipFree(recs); return rc; }
    m->recs = recs;
    return SURFD_OK;
}

int surfd_winding_eval_fast(surfd_winding *m, const float *points, int64_t Q, double beta, int flags, double *w, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_eval_fast: null handle");
    if (Q < 0 || Q >= (1ll << 31)) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_eval_fast: Q = %lld must lie in [0, 2^31)", (long long)Q);
    if (flags & ~SURFD_WINDING_COUNT_VISITS) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_eval_fast: unknown flags 0x%x", flags);
    if (!(beta >= 1.0)) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_eval_fast: beta = %g must be a finite number >= 1 or +inf", beta);
    if (!m->recs) SURFD_FAIL(SURFD_ERR_STATE, "surfd_winding_eval_fast: the hierarchy was not built (surfd_winding_build_bvh)");
    hipStream_t st = as_stream(s);
    int rc;
    if ((flags & SURFD_WINDING_COUNT_VISITS) && (rc = bvh_visits_reset(&m->bvh, st))) return rc;
    if (Q == 0) return SURFD_OK;
    if (!points || !w) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_eval_fast: null points or output");
    hipLaunchKernelGGL(fwn_walk_kernel, dim3((unsigned)ceil_div((long)Q, 256l)), dim3(256), 0, st, (const float *)m->rec, m->F,
                       (const double *)m->recs, (const int4 *)m->bvh.leaf_tri, (const int *)m->bvh.level_off, m->bvh.lay.levels - 1, points,
                       (int)Q, beta * beta, w, (flags & SURFD_WINDING_COUNT_VISITS) ? m->bvh.visits : nullptr);
    LAUNCH_CHECK();
    return SURFD_OK;
}

int surfd_winding_visits(surfd_winding *m, int64_t *cluster_terms, int64_t *triangle_terms, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_visits: null handle");
    if (!m->recs) SURFD_FAIL(SURFD_ERR_STATE, "surfd_winding_visits: the hierarchy was not built");
    return bvh_visits_read("surfd_winding_visits", &m->bvh, cluster_terms, triangle_terms, as_stream(s));
}

int surfd_winding_bvh_info(const surfd_winding *m, int *levels, int *leaves, int *nodes, int32_t *level_sizes, int capacity) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_bvh_info: null handle");
    if (!m->recs) SURFD_FAIL(SURFD_ERR_STATE, "surfd_winding_bvh_info: the hierarchy was not built");
    return bvh_info("surfd_winding_bvh_info", &m->bvh, levels, leaves, nodes, level_sizes, capacity);
}

int surfd_winding_bvh_read(const surfd_winding *m, float *boxes, int32_t *leaf_triangles, double *records, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_winding_bvh_read: null handle");
    if (!m->recs) SURFD_FAIL(SURFD_ERR_STATE, "surfd_winding_bvh_read: the hierarchy was not built");
    if (records)
        HIP_TRY(hipMemcpy2DAsync(records, FWN_REC_USED * sizeof(double), m->recs, FWN_REC * sizeof(double), FWN_REC_USED * sizeof(double),
                                 (size_t)m->bvh.lay.nodes * BVH_W, hipMemcpyDefault, as_stream(s)));
    return bvh_read("surfd_winding_bvh_read", &m->bvh, boxes, leaf_triangles, as_stream(s));
}

}  // extern "C"
