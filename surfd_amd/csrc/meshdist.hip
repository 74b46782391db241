// Exact closest point of a triangle mesh for many query points: the primitive behind the auto-encoder's data preparation
// (reference AutoEncoder/utils.py:223-314, open3d's RaycastingScene.compute_closest_points) and behind the point-to-mesh
// distance that measures a reconstruction.  Plain fp32, VALU only.
//
//   md_prepare_kernel   — (vertices, triangles) -> one 112-byte record per triangle: a, the edges ab, ac, bc, the inverses of
//                         their squared lengths, the unit normal n and the three in-plane edge normals n x ab, n x bc, n x ca
//                         (they point into the triangle).  n comes from an fp64 cross product of the vertices, so it is good to
//                         fp32 rounding however thin the triangle is; a triangle without area gets n = 0.  Out-of-range vertex
//                         indices raise a device flag (and are clamped).
//   md_bounds_kernel    — one bounding sphere per tile of 32 triangles and one per chunk of 8 tiles.
//   md_closest_kernel   — one query per lane, 256 queries per workgroup.  The triangles of one split of the mesh stream through
//                         LDS in chunks of 256 records; every lane of a wave reads the same record at the same time (a broadcast:
//                         identical addresses do not conflict).  The triangle range is split over S workgroups per query block so
//                         that a small call fills the chip.  With CULL a chunk is not even staged when no lane of the workgroup
//                         can be improved by it, and a tile is skipped when no lane of the wave can (wave-uniform branches).
//   md_finish_kernel    — takes the minimum of the S partial results of a query, evaluates the pair test once more on the
//                         winner and writes distance, closest point and triangle index.
//
// Pair test: md_pair().  The regions of the closest point of a triangle (Ericson, Real-Time Collision Detection, 5.1.5: three
// vertices, three edges, the interior) are classified without the products of dot products that the textbook form takes its signs
// from: va, vb, vc are differences of products of size |ab| |ap| |ac| |bp|, and on a thin triangle their rounding exceeds
// |ab x ac|^2, so the signs become noise and the result is wrong by up to the triangle's length.  Instead:
//   * the three edge SEGMENTS, each from its own start vertex (r = q - a, q - b, q - c): t = clamp(e.r / e.e, 0, 1), difference
//     r - t e.  These cover the three vertex and the three edge regions, and every quantity is a plain dot product;
//   * the plane, h = n.(q - a), taken only where q projects strictly inside all three edges: (n x e).r > 0 for each edge with r
//     from that edge's start vertex.  A sign can be wrong only within the rounding of one dot product, i.e. for a projection
//     within a few u |r| of an edge (u = 2^-24), where the plane and the edge answers differ by no more than that.
// The squared distance is the minimum of the four candidates.  Nothing is divided per pair (the inverses of the squared edge
// lengths are per triangle, 0 for an edge without length), so a degenerate triangle gives the distance to the segment or point
// it is and no input gives a NaN or an Inf: without area n and the edge normals are 0 and the strict test never passes.  Each
// segment starts at its own vertex, so a query on a vertex gets the distance 0 exactly.
//
// Selection: per query the winner is the minimum under the total order (squared distance, triangle index).  THE SQUARED DISTANCE
// OF A GIVEN (QUERY, TRIANGLE) PAIR COMES FROM ONE INSTRUCTION SEQUENCE ONLY, md_pair(): every kernel and both the culled and
// the brute-force path call it, with fmaf written out (the library is built with -ffp-contract=off).  The order does not depend
// on the traversal, so the result has the same bits for any tile order, any split count and any culling.
//
// Culling bound (md_cannot_improve).  c, r: a sphere that holds every point of the tile's triangles; D = |q - c|; d = the
// lane's best distance so far.  Every point p of the tile has |q - p| >= D - r.  In fp32:
//   * r is the largest computed vertex distance, enlarged by 1 + 2^-18 in md_bounds_kernel, which covers the <= 4u relative
//     error of that distance and the <= u |ab| by which a record's a + ab differs from the vertex b;
//   * the computed D^2 (three subtractions, one product, two fmaf) is within a factor 1 +- 6u of the true one, so
//     D >= sqrt(D2) (1 - 3.1u);  t = fl(r + d) >= (r + d)(1 - u), and d = fl(sqrt(best2)) >= sqrt(best2)(1 - u): a d rounded
//     DOWN is what could make the test skip too much, and it is that side the margin has to cover;
//   * md_pair's candidates: r_b = fl(r_a - ab) and a segment's difference vector are each rounded by at most 2u (|r| + |e|) per
//     component, its squared length by 3u more; the plane candidate is accepted up to 5u |r| outside an edge and h is off by 4u |r|.
//     With |r| <= D + r and |e| <= 2r the computed distance of a pair is at least D - r - 10u (D + 5r).
//   A tile can be skipped when that exceeds sqrt(best2): D (1 - 10u) > (r + d)(1 + 52u), i.e. D > (r + d)(1 + 63u).  The test
//   D2 > t^2 (1 + 2^-16) gives D > (r + d)(1 + 2^-17 - 2^-21) = (r + d)(1 + 120u): sufficient, with a factor 1.9 in hand, and
//   strict, so a pair that ties the best distance (and might win on the index) is never skipped.  The margin is derived, not tuned.
// The first bound of a wave comes from the tile whose sphere centre is nearest to the wave's first query, visited before the
// ascending pass (a tile visited twice changes nothing: the order above is a total order on pairs).
//
// Hierarchy (surfd_mesh_closest_bvh, the bvm_ kernel; built by meshbvh.hip, whose header describes the tree and how a leaf's box
// is widened so that it holds the triangle md_pair() sees: a, a + ab, a + ac in real numbers).  bvm_closest_kernel: one query
// per lane, every lane walks the implicit tree on its own (meshbvh_layout.h; no stack, no private array), one split, then
// md_finish_kernel with S = 1.  A leaf's triangles go through md_pair() with the handle's own index: keys and ties as above.
// First bound: the lane descends from the root to one leaf, at every node into the child whose box is nearest (the lowest on
// a tie), and takes that leaf's triangles; then it walks the whole tree with the children in ascending order.  The result
// cannot depend on either choice: the winner is the minimum of a total order over the pairs tested, a pair tested twice
// changes nothing, and the bound below never skips a pair that could be that minimum.
// Box bound (bvm_cannot_improve), from md_cannot_improve's analysis, u = 2^-24.  Dn = the distance from q to the box, Df = the
// distance to its farthest corner, d = sqrt(best2) of the lane.  Every point of a triangle in the box is at least Dn away, its
// vertices at most Df, its edges no longer than 2 Df.  md_pair's roundings as listed above (r_b and a segment's difference
// vector 2u (|r| + |e|) per component, the squared length 3u, the plane accepted 5u |r| outside with h off by 4u |r|), with
// |r| <= Df and |e| <= 2 Df, put the computed distance of a pair at or above Dn - 62u Df (the 10u (D + 5r) of the sphere bound
// with D + r <= Df, r <= Df, and 2u Df for a box edge that the widening moved).  A box can be skipped when Dn > d + 62u Df;
// squared, with d Df <= max(d^2, Df^2), that follows from Dn^2 > d^2 + 125u max(d^2, Df^2).  In fp32 D2 = Dn^2 and F2 = Df^2
// (three subtractions, a max, one product, two fmaf each) are within 6u relative, the right-hand side within 3u:
// the test D2 > fl(best2 + 2^-16 fl(best2 + F2)) has 256u (best2 + F2) where 125u + 6u + 3u of it are needed: a factor 1.9 in
// hand, and strict, so a pair that ties the best distance is never skipped.  best2 = +inf (nothing found yet), a box of
// (-inf, +inf)^3 (D2 = 0) and a NaN anywhere make the compare false: no skip.
//
// Hazards: the only LDS reuse is the record chunk of md_closest_kernel, bracketed by a barrier on both sides (__syncthreads_or
// in front of the staging stores, __syncthreads() behind them); cross-lane values move with __shfl_xor / __all only.  The only
// atomics are integer ones (the skipped-tile count, one per wave that holds a query, and the bad-index flag).  A call's partial
// results live in the handle's arena (meshscene.h).
#include "common.h"
#include "meshbvh.h"
#include "meshscene.h"
#include <cfloat>
#include <climits>
#include <cmath>
#include <algorithm>

namespace surfd {

constexpr int MD_TILE = 32;                      // triangles per bounding sphere
constexpr int MD_CHUNK_TILES = 8;
constexpr int MD_CHUNK = MD_TILE * MD_CHUNK_TILES;   // records per LDS chunk, and queries per workgroup
constexpr int MD_MAX_SPLITS = 64;
constexpr float MD_CULL_MARGIN = 1.52587890625e-05f;    // 2^-16, see the header
constexpr float MD_RADIUS_MARGIN = 3.814697265625e-06f; // 2^-18

constexpr int MD_REC4 = 7;                       // float4 per record

struct MdRec {
    float4 a;        // a.xyz,  1 / ab.ab
    float4 ab;       // ab.xyz, 1 / bc.bc
    float4 ac;       // ac.xyz, 1 / ac.ac     (an inverse is 0 where the edge has no positive normal squared length)
    float4 bc;       // bc.xyz, n.x           n = the unit normal, 0 where the triangle has no area
    float4 mab;      // (n x ab).xyz, n.y     the in-plane normals of the three edges, pointing into the triangle
    float4 mbc;      // (n x bc).xyz, n.z
    float4 mca;      // (n x ca).xyz, 0
};

__device__ __forceinline__ float md_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return fmaf(az, bz, fmaf(ay, by, ax * bx));
}

__device__ __forceinline__ float md_clamp01(float x) { return __builtin_amdgcn_fmed3f(x, 0.f, 1.f); }

__device__ __forceinline__ float md_inv(float x) { return (x >= FLT_MIN && x <= FLT_MAX) ? __fdiv_rn(1.f, x) : 0.f; }

// closest point of the segment p + t e, t in [0, 1], to the query at r = q - p: squared distance, (dx, dy, dz) = q - that point.
// sgn = -1 walks the stored edge backwards (the segment c -> a over the stored ac).
__device__ __forceinline__ float md_segment(float rx, float ry, float rz, float4 e, float inv, float sgn, float &dx, float &dy, float &dz) {
    const float t = md_clamp01(sgn * md_dot(e.x, e.y, e.z, rx, ry, rz) * inv);
    const float u = -sgn * t;
    dx = fmaf(u, e.x, rx);
    dy = fmaf(u, e.y, ry);
    dz = fmaf(u, e.z, rz);
    return md_dot(dx, dy, dz, dx, dy, dz);
}

// The pair test.  Returns the squared distance from q to the triangle of record t; (dx, dy, dz) = q - closest point.
__device__ __forceinline__ float md_pair(const MdRec &t, float qx, float qy, float qz, float &dx, float &dy, float &dz) {
    const float ax = qx - t.a.x, ay = qy - t.a.y, az = qz - t.a.z;               // q - a
    const float bx = ax - t.ab.x, by = ay - t.ab.y, bz = az - t.ab.z;           // q - b
    const float cx = ax - t.ac.x, cy = ay - t.ac.y, cz = az - t.ac.z;           // q - c
    float x1, y1, z1, x2, y2, z2, x3, y3, z3;
    const float d1 = md_segment(ax, ay, az, t.ab, t.a.w, 1.f, x1, y1, z1);      // a -> b
    const float d2 = md_segment(bx, by, bz, t.bc, t.ab.w, 1.f, x2, y2, z2);     // b -> c
    const float d3 = md_segment(cx, cy, cz, t.ac, t.ac.w, -1.f, x3, y3, z3);    // c -> a
    // the plane: taken where q projects strictly inside all three edges (never for a triangle without area: its m are 0)
    const float h = md_dot(t.bc.w, t.mab.w, t.mbc.w, ax, ay, az);
    const float s1 = md_dot(t.mab.x, t.mab.y, t.mab.z, ax, ay, az), s2 = md_dot(t.mbc.x, t.mbc.y, t.mbc.z, bx, by, bz);
    const float s3 = md_dot(t.mca.x, t.mca.y, t.mca.z, cx, cy, cz);
    const bool in = fminf(s1, fminf(s2, s3)) > 0.f;          // one min3 and one compare: no short-circuit branches in the loop
    const float de = fminf(d1, fminf(d2, d3));
    const float dp = in ? h * h : INFINITY;
    const float dd = fminf(de, dp);
    // the difference vector of the candidate that gave dd (dead code where a caller does not use it)
    const bool p = dp == dd, e1 = d1 == dd, e2 = d2 == dd;
    dx = p ? h * t.bc.w : (e1 ? x1 : (e2 ? x2 : x3));
    dy = p ? h * t.mab.w : (e1 ? y1 : (e2 ? y2 : y3));
    dz = p ? h * t.mbc.w : (e1 ? z1 : (e2 ? z2 : z3));
    return dd;
}

// the total order (squared distance, triangle index)
__device__ __forceinline__ void md_take(float dd, int j, float &best, int &idx) {
    const bool better = dd < best || (dd == best && j < idx);
    best = better ? dd : best;
    idx = better ? j : idx;
}

// true where no triangle inside the sphere (c.xyz, c.w) can beat the lane's best distance d (header: culling bound)
__device__ __forceinline__ bool md_cannot_improve(float4 c, float qx, float qy, float qz, float d) {
    const float x = qx - c.x, y = qy - c.y, z = qz - c.z;
    const float D2 = md_dot(x, y, z, x, y, z);
    const float t = c.w + d;
    const float t2 = t * t;
    return D2 > fmaf(t2, MD_CULL_MARGIN, t2);
}

__device__ __forceinline__ MdRec md_load(const float4 *p) { return MdRec{p[0], p[1], p[2], p[3], p[4], p[5], p[6]}; }

// one thread per triangle
__global__ __launch_bounds__(256) void md_prepare_kernel(const float *__restrict__ vtx, int V, const int *__restrict__ tri, int F,
                                                         float4 *__restrict__ rec, int *__restrict__ bad) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    float p[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int k = tri[(long)f * 3 + c];
        if (k < 0 || k >= V) { atomicOr(bad, 1); k = 0; }
#pragma unroll
        for (int e = 0; e < 3; ++e) p[c][e] = vtx[(long)k * 3 + e];
    }
    float ab[3], ac[3], bc[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) { ab[e] = p[1][e] - p[0][e]; ac[e] = p[2][e] - p[0][e]; bc[e] = p[2][e] - p[1][e]; }
    const float abab = md_dot(ab[0], ab[1], ab[2], ab[0], ab[1], ab[2]);
    const float acac = md_dot(ac[0], ac[1], ac[2], ac[0], ac[1], ac[2]);
    const float bcbc = md_dot(bc[0], bc[1], bc[2], bc[0], bc[1], bc[2]);
    // The normal in fp64 from the vertices themselves (the differences of fp32 numbers and the products of two such differences
    // are exact or rounded at 2^-53 there), so that the unit normal and the edge normals are good to fp32 rounding however thin
    // the triangle is.  Once per triangle; the pair test stays fp32.
    double E1[3], E2[3], E3[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) { E1[e] = (double)p[1][e] - (double)p[0][e]; E2[e] = (double)p[2][e] - (double)p[0][e]; E3[e] = (double)p[2][e] - (double)p[1][e]; }
    double n[3] = {E1[1] * E2[2] - E1[2] * E2[1], E1[2] * E2[0] - E1[0] * E2[2], E1[0] * E2[1] - E1[1] * E2[0]};
    const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const bool area = nn >= 1e-290 && nn <= 1e290;
    const double s = area ? 1.0 / sqrt(nn) : 0.0;
#pragma unroll
    for (int e = 0; e < 3; ++e) n[e] *= s;
    auto cross = [&](const double (&e)[3], float (&m)[3]) {       // n x e
        m[0] = (float)(n[1] * e[2] - n[2] * e[1]);
        m[1] = (float)(n[2] * e[0] - n[0] * e[2]);
        m[2] = (float)(n[0] * e[1] - n[1] * e[0]);
    };
    float mab[3], mbc[3], mca[3];
    const double CA[3] = {-E2[0], -E2[1], -E2[2]};
    cross(E1, mab); cross(E3, mbc); cross(CA, mca);
    float4 *r = rec + (long)f * MD_REC4;
    r[0] = make_float4(p[0][0], p[0][1], p[0][2], md_inv(abab));
    r[1] = make_float4(ab[0], ab[1], ab[2], md_inv(bcbc));
    r[2] = make_float4(ac[0], ac[1], ac[2], md_inv(acac));
    r[3] = make_float4(bc[0], bc[1], bc[2], (float)n[0]);
    r[4] = make_float4(mab[0], mab[1], mab[2], (float)n[1]);
    r[5] = make_float4(mbc[0], mbc[1], mbc[2], (float)n[2]);
    r[6] = make_float4(mca[0], mca[1], mca[2], 0.f);
}

// one thread per sphere: sphere s holds the records [s * per, min(F, (s + 1) * per)); centre = the middle of their bounding box
__global__ __launch_bounds__(64) void md_bounds_kernel(const float4 *__restrict__ rec, int F, int per, int count, float4 *__restrict__ sph) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= count) return;
    const int f0 = s * per, f1 = min(F, f0 + per);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int f = f0; f < f1; ++f) {
        const MdRec t = md_load(rec + (long)f * MD_REC4);
        const float a[3] = {t.a.x, t.a.y, t.a.z}, ab[3] = {t.ab.x, t.ab.y, t.ab.z}, ac[3] = {t.ac.x, t.ac.y, t.ac.z};
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const float b = a[e] + ab[e], c = a[e] + ac[e];
            lo[e] = fminf(lo[e], fminf(a[e], fminf(b, c)));
            hi[e] = fmaxf(hi[e], fmaxf(a[e], fmaxf(b, c)));
        }
    }
    const float cx = 0.5f * (lo[0] + hi[0]), cy = 0.5f * (lo[1] + hi[1]), cz = 0.5f * (lo[2] + hi[2]);
    float r2 = 0.f;
    for (int f = f0; f < f1; ++f) {
        const MdRec t = md_load(rec + (long)f * MD_REC4);
        const float ax = t.a.x - cx, ay = t.a.y - cy, az = t.a.z - cz;
        const float bx = ax + t.ab.x, by = ay + t.ab.y, bz = az + t.ab.z;
        const float gx = ax + t.ac.x, gy = ay + t.ac.y, gz = az + t.ac.z;
        r2 = fmaxf(r2, fmaxf(md_dot(ax, ay, az, ax, ay, az), fmaxf(md_dot(bx, by, bz, bx, by, bz), md_dot(gx, gy, gz, gx, gy, gz))));
    }
    const float r = __fsqrt_rn(r2);
    sph[s] = make_float4(cx, cy, cz, fmaf(r, MD_RADIUS_MARGIN, r) + FLT_MIN);
}

// queries [Q, 3]; split s covers the chunks [s * span, min(nchunk, (s + 1) * span)); partial results pd / pi [S, Q]
template <bool CULL>
__global__ __launch_bounds__(256) void md_closest_kernel(const float4 *__restrict__ rec, int F, const float4 *__restrict__ tile_sph,
                                                         const float4 *__restrict__ chunk_sph, int nchunk, int span,
                                                         const float *__restrict__ queries, int Q, float *__restrict__ pd,
                                                         int *__restrict__ pi, unsigned long long *__restrict__ skipped) {
    __shared__ float4 lds[MD_CHUNK * MD_REC4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = blockIdx.x * MD_CHUNK + tid;
    const int nq = n < Q ? n : Q - 1;
    const float qx = queries[(long)nq * 3], qy = queries[(long)nq * 3 + 1], qz = queries[(long)nq * 3 + 2];
    float best = INFINITY, bestd = INFINITY;
    int idx = INT_MAX;
    float dx, dy, dz;
    unsigned nskip = 0;
    const int ntile = (F + MD_TILE - 1) / MD_TILE;
    if constexpr (CULL) {
        // the tile whose sphere centre is nearest to the wave's first query gives every lane of the wave its first bound
        const float fx = __shfl(qx, 0), fy = __shfl(qy, 0), fz = __shfl(qz, 0);
        float sd = INFINITY;
        int st = INT_MAX;
        for (int t = lane; t < ntile; t += 64) {
            const float4 c = tile_sph[t];
            const float x = fx - c.x, y = fy - c.y, z = fz - c.z;
            const float d = md_dot(x, y, z, x, y, z);
            if (d < sd) { sd = d; st = t; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float od = __shfl_xor(sd, o);
            const int ot = __shfl_xor(st, o);
            if (od < sd || (od == sd && ot < st)) { sd = od; st = ot; }
        }
        st = __builtin_amdgcn_readfirstlane(st);
        if (st < ntile) {                                   // false only where every centre distance is a NaN
            const int f0 = st * MD_TILE, f1 = min(F, f0 + MD_TILE);
            for (int f = f0; f < f1; ++f) {
                const MdRec t = md_load(rec + (long)f * MD_REC4);
                md_take(md_pair(t, qx, qy, qz, dx, dy, dz), f, best, idx);
            }
            bestd = __fsqrt_rn(best);
        }
    }
    const int c0 = blockIdx.y * span, c1 = min(nchunk, c0 + span);
    for (int c = c0; c < c1; ++c) {
        const int f0 = c * MD_CHUNK;
        const int cnt = min(MD_CHUNK, F - f0);
        const int tiles = (cnt + MD_TILE - 1) / MD_TILE;
        if constexpr (CULL) {
            // a barrier (every lane is done with the previous chunk) that also tells whether any lane needs this chunk
            const int need = __syncthreads_or(!md_cannot_improve(chunk_sph[c], qx, qy, qz, bestd));
            if (!need) { nskip += tiles; continue; }        // the same in every lane of the workgroup
        } else {
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < MD_REC4; ++i) {
            const int e = tid + 256 * i;
            if (e < cnt * MD_REC4) lds[e] = rec[(long)f0 * MD_REC4 + e];
        }
        __syncthreads();
        for (int tt = 0; tt < tiles; ++tt) {
            const int u0 = tt * MD_TILE, u1 = min(cnt, u0 + MD_TILE);
            if constexpr (CULL) {
                if (__all(md_cannot_improve(tile_sph[c * MD_CHUNK_TILES + tt], qx, qy, qz, bestd))) { nskip += 1; continue; }   // wave-uniform
            }
            for (int u = u0; u < u1; ++u) {
                const MdRec t = md_load(lds + u * MD_REC4);
                md_take(md_pair(t, qx, qy, qz, dx, dy, dz), f0 + u, best, idx);
            }
            if constexpr (CULL) bestd = __fsqrt_rn(best);
        }
    }
    if (n < Q) {
        pd[(long)blockIdx.y * Q + n] = best;
        pi[(long)blockIdx.y * Q + n] = idx;
    }
    if constexpr (CULL) {
        if (skipped && lane == 0 && n < Q && nskip) atomicAdd(skipped, (unsigned long long)nskip);
    }
}

// squared distances from q to the nearest point (D2) and to the farthest corner (F2) of a box
__device__ __forceinline__ void bvm_box(float lox, float loy, float loz, float hix, float hiy, float hiz, float qx, float qy, float qz,
                                        float &D2, float &F2) {
    const float ax = lox - qx, ay = loy - qy, az = loz - qz, bx = qx - hix, by = qy - hiy, bz = qz - hiz;
    const float nx = fmaxf(fmaxf(ax, bx), 0.f), ny = fmaxf(fmaxf(ay, by), 0.f), nz = fmaxf(fmaxf(az, bz), 0.f);
    const float fx = fmaxf(fabsf(ax), fabsf(bx)), fy = fmaxf(fabsf(ay), fabsf(by)), fz = fmaxf(fabsf(az), fabsf(bz));
    D2 = md_dot(nx, ny, nz, nx, ny, nz);
    F2 = md_dot(fx, fy, fz, fx, fy, fz);
}

// true where no triangle inside the box can beat or tie the lane's best squared distance (header: box bound)
__device__ __forceinline__ bool bvm_cannot_improve(float D2, float F2, float best2) {
    return D2 > fmaf(best2 + F2, MD_CULL_MARGIN, best2);
}

// the children of a node that the lane has to enter: bit c for child c
__device__ __forceinline__ unsigned bvm_children(const BvhNode &n, float qx, float qy, float qz, float best2, unsigned &nbox) {
    unsigned m = 0;
#pragma unroll
    for (int c = 0; c < BVH_W; ++c) {
        const float lox = bvh_comp(n.lox, c), hix = bvh_comp(n.hix, c);
        const bool there = bvh_child_exists(lox, hix);
        float D2, F2;
        bvm_box(lox, bvh_comp(n.loy, c), bvh_comp(n.loz, c), hix, bvh_comp(n.hiy, c), bvh_comp(n.hiz, c), qx, qy, qz, D2, F2);
        nbox += there ? 1u : 0u;
        m |= (there && !bvm_cannot_improve(D2, F2, best2)) ? (1u << c) : 0u;
    }
    return m;
}

// the existing child whose box is nearest to q (the lowest on a tie; child 0 of a node always exists)
__device__ __forceinline__ unsigned bvm_nearest(const BvhNode &n, float qx, float qy, float qz, unsigned &nbox) {
    unsigned best = 0;
    float bd = INFINITY;
#pragma unroll
    for (int c = 0; c < BVH_W; ++c) {
        const float lox = bvh_comp(n.lox, c), hix = bvh_comp(n.hix, c);
        const bool there = bvh_child_exists(lox, hix);
        float D2, F2;
        bvm_box(lox, bvh_comp(n.loy, c), bvh_comp(n.loz, c), hix, bvh_comp(n.hiy, c), bvh_comp(n.hiz, c), qx, qy, qz, D2, F2);
        nbox += there ? 1u : 0u;
        const bool take = there && D2 < bd;
        bd = take ? D2 : bd;
        best = take ? (unsigned)c : best;
    }
    return best;
}

__device__ __forceinline__ void bvm_leaf(const float4 *__restrict__ rec, int F, int4 ids, float qx, float qy, float qz, float &best, int &idx,
                                         unsigned &npair) {
    float dx, dy, dz;
#pragma unroll
    for (int i = 0; i < BVH_L; ++i) {
        const int f = bvh_comp(ids, i);
        if ((unsigned)f >= (unsigned)F) continue;                  // -1: the last leaf has fewer than L triangles
        md_take(md_pair(md_load(rec + (long)f * MD_REC4), qx, qy, qz, dx, dy, dz), f, best, idx);
        npair += 1;
    }
}

// queries [Q, 3]; results pd / pi [Q] (one split).  visits: null, or two counters (box tests, pair tests)
__global__ __launch_bounds__(256) void bvm_closest_kernel(const float4 *__restrict__ rec, int F, const float4 *__restrict__ boxes,
                                                          const int4 *__restrict__ leaf_tri, const int *__restrict__ level_off, int top,
                                                          int nleaf, const float *__restrict__ queries, int Q, float *__restrict__ pd,
                                                          int *__restrict__ pi, unsigned long long *__restrict__ visits) {
    __shared__ int off[BVH_MAX_LEVELS];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < BVH_MAX_LEVELS) off[tid] = level_off[tid];
    __syncthreads();
    const int n = blockIdx.x * MD_CHUNK + tid;
    const int nq = n < Q ? n : Q - 1;
    const float qx = queries[(long)nq * 3], qy = queries[(long)nq * 3 + 1], qz = queries[(long)nq * 3 + 2];
    float best = INFINITY;
    int idx = INT_MAX;
    unsigned nbox = 0, npair = 0;
    // the first bound: down to one leaf through the nearest boxes
    unsigned node = 0;
#pragma unroll 1
    for (int level = top; level >= 0; --level) node = node * BVH_W + bvm_nearest(bvh_load(boxes, off[level], node), qx, qy, qz, nbox);
    if (node < (unsigned)nleaf) bvm_leaf(rec, F, leaf_tri[node], qx, qy, qz, best, idx, npair);
    // the whole tree, children in ascending order
    int level = top;
    unsigned child = 0;
    node = 0;
    unsigned long long mask = bvh_mask_bits(top, bvm_children(bvh_load(boxes, off[top], 0), qx, qy, qz, best, nbox));
#pragma unroll 1
    while (bvh_next(top, level, node, mask, child)) {
        if (level > 0) {
            bvh_enter(level, node, child);
            mask |= bvh_mask_bits(level, bvm_children(bvh_load(boxes, off[level], node), qx, qy, qz, best, nbox));
        } else {
            bvm_leaf(rec, F, leaf_tri[child], qx, qy, qz, best, idx, npair);
        }
    }
    if (n < Q) {
        pd[n] = best;
        pi[n] = idx;
    }
    if (visits && n - lane < Q) bvh_count_visits(visits, n < Q ? nbox : 0u, n < Q ? npair : 0u, lane);
}

// the minimum of the S partial results of query n under (squared distance, index), then the pair test on the winner
__global__ __launch_bounds__(256) void md_finish_kernel(const float4 *__restrict__ rec, int F, const float *__restrict__ queries, int Q,
                                                        const float *__restrict__ pd, const int *__restrict__ pi, int S,
                                                        float *__restrict__ dist, float *__restrict__ closest, int *__restrict__ tri) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= Q) return;
    float best = INFINITY;
    int idx = INT_MAX;
    for (int s = 0; s < S; ++s) md_take(pd[(long)s * Q + n], pi[(long)s * Q + n], best, idx);
    idx = idx >= 0 && idx < F ? idx : 0;                     // INT_MAX only where every pair gave a NaN or an Inf (not a finite query)
    const float qx = queries[(long)n * 3], qy = queries[(long)n * 3 + 1], qz = queries[(long)n * 3 + 2];
    float dx, dy, dz;
    const float dd = md_pair(md_load(rec + (long)idx * MD_REC4), qx, qy, qz, dx, dy, dz);
    if (dist) dist[n] = __fsqrt_rn(dd);
    if (closest) {
        closest[(long)n * 3] = qx - dx;
        closest[(long)n * 3 + 1] = qy - dy;
        closest[(long)n * 3 + 2] = qz - dz;
    }
    if (tri) tri[n] = idx;
}

}  // namespace surfd

using namespace surfd;

struct surfd_mesh {
    int F = 0, ntile = 0, nchunk = 0;
    float4 *rec = nullptr;            // [F] records of 4 float4
    float4 *tile_sph = nullptr;       // [ntile]
    float4 *chunk_sph = nullptr;      // [nchunk]
    mutable DeviceArena ws;           // partial results of surfd_mesh_closest: the calls take a const handle
    MeshBvh bvh;                      // the hierarchy of surfd_mesh_build_bvh (meshbvh.hip)
};

extern "C" {

int surfd_mesh_create(const float *vertices, int V, const int32_t *triangles, int F, surfd_stream s, surfd_mesh **out) {
    int rc = mesh_create_args("surfd_mesh_create", vertices, V, triangles, F, out, 1 << 28);
    if (rc != SURFD_OK) return rc;
    hipStream_t st = as_stream(s);
    surfd_mesh *m = new surfd_mesh();
    m->F = F;
    m->ntile = ceil_div(F, MD_TILE);
    m->nchunk = ceil_div(F, MD_CHUNK);
    CreateFlags bad(1);
    int flag = 0;
    auto run = [&]() -> int {
        HIP_TRY(hipMalloc(&m->rec, (size_t)F * sizeof(MdRec)));
        HIP_TRY(hipMalloc(&m->tile_sph, (size_t)m->ntile * sizeof(float4)));
        HIP_TRY(hipMalloc(&m->chunk_sph, (size_t)m->nchunk * sizeof(float4)));
        if (int e = bad.init(st)) return e;
        hipLaunchKernelGGL(md_prepare_kernel, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, st, vertices, V, triangles, F, m->rec, bad.dev);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(md_bounds_kernel, dim3((unsigned)ceil_div(m->ntile, 64)), dim3(64), 0, st, (const float4 *)m->rec, F, MD_TILE,
                           m->ntile, m->tile_sph);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(md_bounds_kernel, dim3((unsigned)ceil_div(m->nchunk, 64)), dim3(64), 0, st, (const float4 *)m->rec, F, MD_CHUNK,
                           m->nchunk, m->chunk_sph);
        LAUNCH_CHECK();
        return bad.read(&flag, st);
    };
    rc = run();
    if (rc == SURFD_OK && flag) rc = mesh_bad_index("surfd_mesh_create", V);
    if (rc != SURFD_OK) { surfd_mesh_destroy(m); return rc; }
    *out = m;
    return SURFD_OK;
}

void surfd_mesh_destroy(surfd_mesh *m) {
    if (!m) return;
    (void)hipFree(m->rec); (void)hipFree(m->tile_sph); (void)hipFree(m->chunk_sph);
    m->ws.release();
    bvh_free(&m->bvh);
    delete m;
}

int surfd_mesh_num_triangles(const surfd_mesh *m) { return m ? m->F : 0; }

int surfd_mesh_closest(const surfd_mesh *m, const float *queries, int Q, int flags, float *dist, float *closest, int32_t *tri,
                       int64_t *skipped_tiles, surfd_stream s) {
    if (Q < 0) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mesh_closest: Q = %d is negative", Q);
    if (flags & ~SURFD_MESH_BRUTE_FORCE) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mesh_closest: unknown flags 0x%x", flags);
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mesh_closest: null handle");
    if (Q == 0) return SURFD_OK;
    if (!queries) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mesh_closest: null queries");
    if (Q > (1 << 28)) SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_mesh_closest: Q = %d is beyond the supported size", Q);
    hipStream_t st = as_stream(s);
    const Split sp = split_units(Q, MD_CHUNK, m->nchunk, MD_MAX_SPLITS);      // splits of the chunk range per query block
    const int S = sp.S, span = sp.span;
    const size_t np = (size_t)S * Q;
    if (int rc = m->ws.reserve(2 * np * sizeof(float), st)) return rc;
    float *pd = (float *)m->ws.ptr;
    int *pi = (int *)(pd + np);
    if (skipped_tiles) HIP_TRY(hipMemsetAsync(skipped_tiles, 0, sizeof(int64_t), st));
    const dim3 grid((unsigned)ceil_div(Q, MD_CHUNK), (unsigned)S);
    if (flags & SURFD_MESH_BRUTE_FORCE)
        hipLaunchKernelGGL(md_closest_kernel<false>, grid, dim3(256), 0, st, (const float4 *)m->rec, m->F, (const float4 *)m->tile_sph,
                           (const float4 *)m->chunk_sph, m->nchunk, span, queries, Q, pd, pi, (unsigned long long *)nullptr);
    else
        hipLaunchKernelGGL(md_closest_kernel<true>, grid, dim3(256), 0, st, (const float4 *)m->rec, m->F, (const float4 *)m->tile_sph,
                           (const float4 *)m->chunk_sph, m->nchunk, span, queries, Q, pd, pi, (unsigned long long *)skipped_tiles);
    LAUNCH_CHECK();
    if (dist || closest || tri) {
        hipLaunchKernelGGL(md_finish_kernel, dim3((unsigned)ceil_div(Q, 256)), dim3(256), 0, st, (const float4 *)m->rec, m->F, queries, Q,
                           (const float *)pd, (const int *)pi, S, dist, closest, tri);
        LAUNCH_CHECK();
    }
    return SURFD_OK;
}

int surfd_mesh_build_bvh(surfd_mesh *m, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mesh_build_bvh: null handle");
    return bvh_build(&m->bvh, (const float4 *)m->rec, MD_REC4, true, m->F, as_stream(s));
}

int surfd_mesh_closest_bvh(const surfd_mesh *m, const float *queries, int Q, int flags, float *dist, float *closest, int32_t *tri,
                           int64_t *skipped_tiles, surfd_stream s) {
    if (Q < 0) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mesh_closest_bvh: Q = %d is negative", Q);
    if (flags & ~(SURFD_MESH_BRUTE_FORCE | SURFD_MESH_COUNT_VISITS)) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mesh_closest_bvh: unknown flags 0x%x", flags);
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mesh_closest_bvh: null handle");
    if (flags & SURFD_MESH_BRUTE_FORCE) return surfd_mesh_closest(m, queries, Q, SURFD_MESH_BRUTE_FORCE, dist, closest, tri, skipped_tiles, s);
    if (!m->bvh.built) SURFD_FAIL(SURFD_ERR_STATE, "surfd_mesh_closest_bvh: the hierarchy was not built (surfd_mesh_build_bvh)");
    if (Q == 0) return SURFD_OK;
    if (!queries) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mesh_closest_bvh: null queries");
    if (Q > (1 << 28)) SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_mesh_closest_bvh: Q = %d is beyond the supported size", Q);
    hipStream_t st = as_stream(s);
    int rc;
    if ((rc = m->ws.reserve(2 * (size_t)Q * sizeof(float), st))) return rc;
    float *pd = (float *)m->ws.ptr;
    int *pi = (int *)(pd + Q);
    if (skipped_tiles) HIP_TRY(hipMemsetAsync(skipped_tiles, 0, sizeof(int64_t), st));      // no tiles on this path
    if ((flags & SURFD_MESH_COUNT_VISITS) && (rc = bvh_visits_reset(&m->bvh, st))) return rc;
    hipLaunchKernelGGL(bvm_closest_kernel, dim3((unsigned)ceil_div(Q, MD_CHUNK)), dim3(256), 0, st, (const float4 *)m->rec, m->F,
                       (const float4 *)m->bvh.boxes, (const int4 *)m->bvh.leaf_tri, (const int *)m->bvh.level_off, m->bvh.lay.levels - 1,
                       m->bvh.lay.nleaf, queries, Q, pd, pi, (flags & SURFD_MESH_COUNT_VISITS) ? m->bvh.visits : nullptr);
    LAUNCH_CHECK();
    if (dist || closest || tri) {
        hipLaunchKernelGGL(md_finish_kernel, dim3((unsigned)ceil_div(Q, 256)), dim3(256), 0, st, (const float4 *)m->rec, m->F, queries, Q,
                           (const float *)pd, (const int *)pi, 1, dist, closest, tri);
        LAUNCH_CHECK();
    }
    return SURFD_OK;
}

int surfd_mesh_visits(const surfd_mesh *m, int64_t *box_tests, int64_t *pair_tests, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mesh_visits: null handle");
    return bvh_visits_read("surfd_mesh_visits", &m->bvh, box_tests, pair_tests, as_stream(s));
}

int surfd_mesh_bvh_info(const surfd_mesh *m, int *levels, int *leaves, int *nodes, int32_t *level_sizes, int capacity) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mesh_bvh_info: null handle");
    return bvh_info("surfd_mesh_bvh_info", &m->bvh, levels, leaves, nodes, level_sizes, capacity);
}

int surfd_mesh_bvh_read(const surfd_mesh *m, float *boxes, int32_t *leaf_triangles, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mesh_bvh_read: null handle");
    return bvh_read("surfd_mesh_bvh_read", &m->bvh, boxes, leaf_triangles, as_stream(s));
}

}  // extern "C"
