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
#include "common.h"
#include "meshscene.h"
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

}  // namespace surfd

using namespace surfd;

struct surfd_winding {
    int F = 0, nchunk = 0, ngroup = 0;
    float *rec = nullptr;             // [F] triangles of 9 fp32
    DeviceArena ws;                   // partial sums [ngroup, slab]
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

}  // extern "C"
