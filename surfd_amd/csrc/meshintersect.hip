// Intersection tests between the triangles of one mesh (self-intersections) or of two meshes (collisions): which pairs of
// triangles have a common point.  No reference counterpart (the reference ships no evaluation code); the number is the share of
// self-intersecting faces that work on meshing unsigned distance fields reports next to the Chamfer distance.  One fp32 snap
// per vertex, then int64 on int32 differences: no epsilon, no floating-point atomics, no MFMA.
//
// The contract of one pair, restated decision for decision in tests/meshintersect_ref.py:
//   snap      q = rint(x * 2^L) in fp32 (the product with a power of two is exact, so rint is the only rounding), converted to
//             int32.  L = lattice_log2 of create.  A NaN or |q| > 2^19 is refused by create, so is an index outside [0, V).  Two
//             vertices are the same point when their snapped coordinates are equal, whatever their indices.
//   o3        o3(a, b, c, d) = ((b - a) x (c - a)) . (d - a).  |q| <= 2^19: differences <= 2^20, cross components <= 2^41, every
//             partial sum of the dot product < 3 * 2^61.  Integer arithmetic is exact, so the grouping of the sums is free.
//   o2        the 2-D orientation after dropping the axis of the largest |normal component| of the triangle concerned (the
//             lower axis on a tie); kept axes (axis + 1, axis + 2) mod 3.  Values <= 2^41.
//   degenerate  a triangle whose normal is (0, 0, 0) after the snap: flagged, intersects nothing.
//   segment pq against triangle abc, both closed:  sp = sign o3(a, b, c, p), sq = sign o3(a, b, c, q).  Both strictly on one
//             side: no.  Both zero (coplanar): yes iff p or q lies in the triangle (o2(a, b, .), o2(b, c, .), o2(c, a, .) all >= 0
//             or all <= 0) or pq meets one of its edges: the closed 2-D segment test (the signs of o2(p, q, a), o2(p, q, b) differ
//             and those of o2(a, b, p), o2(a, b, q) differ, or one of the four is zero and its point lies in the other segment's
//             box on both kept axes).  Otherwise: yes iff o3(p, q, a, b), o3(p, q, b, c), o3(p, q, c, a) are all >= 0 or all <= 0.
//   closed test  some edge of A meets B, or some edge of B meets A.
//   verdict   inside one mesh, by the number k of points the two triangles share:
//             k = 0  the closed test: touching counts.
//             k = 1  the edge of A opposite the shared point meets B, or the edge of B opposite it meets A ("a common point other
//                    than the shared one": the intersection is convex and leaves one of the wedges through its opposite edge).
//                    A T-junction therefore counts.
//             k = 2  shared edge uw, opposite corners c of A and d of B: yes iff o3(u, w, c, d) == 0 and o2(u, w, c), o2(u, w, d)
//                    have equal signs in A's projection: a fold laid flat onto itself.  Any other pair sharing an edge is a
//                    proper neighbour.
//             k = 3  yes: duplicate faces, in either winding.
//             Between two meshes the closed test applies to every pair, no sharing rule.
// The verdict of a pair depends on the two triangles alone; hits are integer sums and the pair list is a set: any order of
// the triangles, split count or culling gives the same answer.  Culling uses exact integer boxes with a closed overlap test
// (lo <= hi on all three axes); two triangles with a common point have overlapping boxes, and so have any boxes that contain
// them, so culling drops only pairs that every verdict above refuses: culled equals brute force with no error analysis.
//
// Kernels:
//   mi_snap_kernel     one thread per vertex: the snap, and the count of vertices that are refused.
//   mi_gather_kernel   one thread per triangle: three int4 (A | degenerate flag, B, C); an index outside [0, V) raises a flag.
//   mi_bounds_kernel   one thread per box: tiles of 32 consecutive triangles and chunks of 256; two int4 (lo, hi) each.
//   mi_pair_kernel     one triangle per lane (nine coordinates, normal and box in registers), 256 lanes per workgroup; grid.y
//                      splits the partner chunks.  A partner chunk of 256 triangles is staged in LDS and all lanes of a wave read
//                      the same partner at the same time (a broadcast).  <CULL>: a chunk is not staged when no lane's box meets
//                      the chunk box, a tile is skipped on the wave's ballot, a lane evaluates the predicate only for partners
//                      whose own box meets its box.  <SELF>: lane i evaluates the pair (i, j) for j > i only, and chunks wholly
//                      below the workgroup's first triangle are never visited.  The predicate runs under the lane's own test:
//                      the divergence is accepted (unmeasured alternatives).  The coplanar branch is a
//                      function of its own (mi_coplanar, not inlined), outside the common path's registers.
//   mi_flags_kernel    the degenerate flags as bytes, and their count.
//
// Bounds.  Vertex v < V reads vertices[3 v .. 3 v + 2] and writes q[3 v .. 3 v + 2].  Triangle f < F reads triangles[3 f .. 3 f + 2],
// reads q at an index clamped into [0, V) and writes rec[3 f .. 3 f + 2].  Box s < count reads rec[3 f ..] for f < F only.  In the
// pair kernel lane i >= FA reads record FA - 1 and writes nothing; chunk c < nchunkB, staging reads rec[3 (256 c) + e] for
// e < 3 cnt with 256 c + cnt <= FB; LDS is indexed with 3 u + 2 < 3 cnt <= 768; box arrays with 2 c + 1 < 2 nchunkB and
// 2 (8 c + tt) + 1 < 2 ntileB (tt < ceil(cnt / 32), so 8 c + tt < ntileB); hits with i < FA and j = 256 c + u < FB; pairs with a
// slot < capacity only.  Hazards: the LDS chunk is bracketed by a barrier on both sides.  No workgroup waits for another.
// The host side of create, the split count and the skipped read-back are meshscene.h's; this handle keeps no arena.
#include "common.h"
#include "meshscene.h"
#include <climits>
#include <cmath>
#include <algorithm>

namespace surfd {

constexpr int MI_TILE = 32;                       // triangles per tile box
constexpr int MI_CHUNK_TILES = 8;
constexpr int MI_CHUNK = MI_TILE * MI_CHUNK_TILES;    // triangles per LDS chunk, and lanes per workgroup
constexpr int MI_MAX_SPLITS = 64;
constexpr float MI_SNAP_MAX = 524288.f;           // 2^19
constexpr int MI_MAX_LOG2 = 100;

typedef long long i64;
struct I3 { int x, y, z; };
struct L3 { i64 x, y, z; };
struct MiTri { I3 a, b, c; };

__device__ __forceinline__ I3 mi_sub(I3 p, I3 q) { return {p.x - q.x, p.y - q.y, p.z - q.z}; }
__device__ __forceinline__ bool mi_same(I3 p, I3 q) { return p.x == q.x && p.y == q.y && p.z == q.z; }
__device__ __forceinline__ L3 mi_cross(I3 u, I3 v) {
    return {(i64)u.y * v.z - (i64)u.z * v.y, (i64)u.z * v.x - (i64)u.x * v.z, (i64)u.x * v.y - (i64)u.y * v.x};
}
__device__ __forceinline__ i64 mi_dot(L3 n, I3 e) { return (n.x * e.x + n.y * e.y) + n.z * e.z; }
__device__ __forceinline__ int mi_sgn(i64 x) { return (x > 0) - (x < 0); }
__device__ __forceinline__ L3 mi_normal(const MiTri &t) { return mi_cross(mi_sub(t.b, t.a), mi_sub(t.c, t.a)); }
__device__ __forceinline__ bool mi_same_side(i64 x, i64 y, i64 z) { return (x >= 0 && y >= 0 && z >= 0) || (x <= 0 && y <= 0 && z <= 0); }
__device__ __forceinline__ I3 mi_i3(int4 v) { return {v.x, v.y, v.z}; }
// corner k of t, k in 0 .. 5 (k and k - 3 name the same corner)
__device__ __forceinline__ I3 mi_corner(const MiTri &t, int k) { return (k == 0 || k == 3) ? t.a : ((k == 1 || k == 4) ? t.b : t.c); }

struct P2 { int u, v; };
__device__ __forceinline__ P2 mi_flat(I3 p, int ax) { return ax == 0 ? P2{p.y, p.z} : (ax == 1 ? P2{p.z, p.x} : P2{p.x, p.y}); }
__device__ __forceinline__ i64 mi_o2(P2 p, P2 q, P2 r) { return (i64)(q.u - p.u) * (r.v - p.v) - (i64)(q.v - p.v) * (r.u - p.u); }
__device__ __forceinline__ int mi_drop_axis(L3 n) {
    const i64 x = n.x < 0 ? -n.x : n.x, y = n.y < 0 ? -n.y : n.y, z = n.z < 0 ? -n.z : n.z;
    return (x >= y && x >= z) ? 0 : (y >= z ? 1 : 2);
}
__device__ __forceinline__ bool mi_in_box(P2 x, P2 p, P2 q) {
    return min(p.u, q.u) <= x.u && x.u <= max(p.u, q.u) && min(p.v, q.v) <= x.v && x.v <= max(p.v, q.v);
}
__device__ __forceinline__ bool mi_seg_seg(P2 p, P2 q, P2 a, P2 b) {
    const int s1 = mi_sgn(mi_o2(p, q, a)), s2 = mi_sgn(mi_o2(p, q, b)), s3 = mi_sgn(mi_o2(a, b, p)), s4 = mi_sgn(mi_o2(a, b, q));
    return (s1 != s2 && s3 != s4) || (s1 == 0 && mi_in_box(a, p, q)) || (s2 == 0 && mi_in_box(b, p, q)) ||
           (s3 == 0 && mi_in_box(p, a, b)) || (s4 == 0 && mi_in_box(q, a, b));
}
__device__ __forceinline__ bool mi_in_tri(P2 x, P2 a, P2 b, P2 c) { return mi_same_side(mi_o2(a, b, x), mi_o2(b, c, x), mi_o2(c, a, x)); }

// the coplanar case of the segment test: rare, kept out of the caller's registers
__device__ __noinline__ bool mi_coplanar(int px, int py, int pz, int qx, int qy, int qz, int ax_, int ay_, int az_, int bx, int by, int bz,
                                         int cx, int cy, int cz, int axis) {
    const P2 p = mi_flat({px, py, pz}, axis), q = mi_flat({qx, qy, qz}, axis);
    const P2 a = mi_flat({ax_, ay_, az_}, axis), b = mi_flat({bx, by, bz}, axis), c = mi_flat({cx, cy, cz}, axis);
    return mi_in_tri(p, a, b, c) || mi_in_tri(q, a, b, c) || mi_seg_seg(p, q, a, b) || mi_seg_seg(p, q, b, c) || mi_seg_seg(p, q, c, a);
}

// closed segment pq against closed triangle t with normal n; sp, sq = the signs of o3(a, b, c, p) and o3(a, b, c, q)
__device__ __forceinline__ bool mi_seg_tri(I3 p, I3 q, int sp, int sq, const MiTri &t, L3 n) {
    if (sp * sq > 0) return false;
    if ((sp | sq) == 0)
        return mi_coplanar(p.x, p.y, p.z, q.x, q.y, q.z, t.a.x, t.a.y, t.a.z, t.b.x, t.b.y, t.b.z, t.c.x, t.c.y, t.c.z, mi_drop_axis(n));
    const I3 e = mi_sub(q, p), ea = mi_sub(t.a, p), eb = mi_sub(t.b, p), ec = mi_sub(t.c, p);
    return mi_same_side(mi_dot(mi_cross(e, ea), eb), mi_dot(mi_cross(e, eb), ec), mi_dot(mi_cross(e, ec), ea));
}
__device__ __forceinline__ bool mi_seg_tri(I3 p, I3 q, const MiTri &t, L3 n) {
    return mi_seg_tri(p, q, mi_sgn(mi_dot(n, mi_sub(p, t.a))), mi_sgn(mi_dot(n, mi_sub(q, t.a))), t, n);
}

__device__ __forceinline__ bool mi_closed(const MiTri &A, L3 nA, const MiTri &B, L3 nB) {
    const int a0 = mi_sgn(mi_dot(nB, mi_sub(A.a, B.a))), a1 = mi_sgn(mi_dot(nB, mi_sub(A.b, B.a))), a2 = mi_sgn(mi_dot(nB, mi_sub(A.c, B.a)));
    const int b0 = mi_sgn(mi_dot(nA, mi_sub(B.a, A.a))), b1 = mi_sgn(mi_dot(nA, mi_sub(B.b, A.a))), b2 = mi_sgn(mi_dot(nA, mi_sub(B.c, A.a)));
    return mi_seg_tri(A.a, A.b, a0, a1, B, nB) || mi_seg_tri(A.b, A.c, a1, a2, B, nB) || mi_seg_tri(A.c, A.a, a2, a0, B, nB) ||
           mi_seg_tri(B.a, B.b, b0, b1, A, nA) || mi_seg_tri(B.b, B.c, b1, b2, A, nA) || mi_seg_tri(B.c, B.a, b2, b0, A, nA);
}

// the verdict of two triangles that are not degenerate
template <bool SELF>
__device__ __forceinline__ bool mi_verdict(const MiTri &A, L3 nA, const MiTri &B, L3 nB) {
    if constexpr (SELF) {
        int ma = 0, mb = 0;                                   // the corners of A / of B that are a corner of the other
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (mi_same(mi_corner(A, i), mi_corner(B, j))) { ma |= 1 << i; mb |= 1 << j; }
        const int k = __popc(ma);
        if (k == 3) return true;
        if (k == 2) {
            const int i = __ffs(~ma & 7) - 1, j = __ffs(~mb & 7) - 1;
            const I3 c = mi_corner(A, i), u = mi_corner(A, i + 1), w = mi_corner(A, i + 2), d = mi_corner(B, j);
            if (mi_dot(mi_cross(mi_sub(w, u), mi_sub(c, u)), mi_sub(d, u)) != 0) return false;
            const int axis = mi_drop_axis(nA);
            const P2 fu = mi_flat(u, axis), fw = mi_flat(w, axis);
            return mi_sgn(mi_o2(fu, fw, mi_flat(c, axis))) == mi_sgn(mi_o2(fu, fw, mi_flat(d, axis)));
        }
        if (k == 1) {
            const int i = __ffs(ma) - 1, j = __ffs(mb) - 1;
            return mi_seg_tri(mi_corner(A, i + 1), mi_corner(A, i + 2), B, nB) || mi_seg_tri(mi_corner(B, j + 1), mi_corner(B, j + 2), A, nA);
        }
    }
    return mi_closed(A, nA, B, nB);
}

struct MiBox { int lx, ly, lz, hx, hy, hz; };
__device__ __forceinline__ bool mi_overlap(const MiBox &b, int4 lo, int4 hi) {
    return b.lx <= hi.x && lo.x <= b.hx && b.ly <= hi.y && lo.y <= b.hy && b.lz <= hi.z && lo.z <= b.hz;
}
__device__ __forceinline__ int mi_min3(int a, int b, int c) { return min(a, min(b, c)); }
__device__ __forceinline__ int mi_max3(int a, int b, int c) { return max(a, max(b, c)); }

// one thread per vertex
__global__ __launch_bounds__(256) void mi_snap_kernel(const float *__restrict__ vtx, int V, float scale, int *__restrict__ q,
                                                      int *__restrict__ bad) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float r = rintf(vtx[(long)v * 3 + c] * scale);
        const bool in = fabsf(r) <= MI_SNAP_MAX;              // false for a NaN
        ok = ok && in;
        q[(long)v * 3 + c] = in ? (int)r : 0;
    }
    if (!ok) atomicAdd(bad, 1);
}

// one thread per triangle
__global__ __launch_bounds__(256) void mi_gather_kernel(const int *__restrict__ q, int V, const int *__restrict__ tri, int F,
                                                        int4 *__restrict__ rec, int *__restrict__ bad) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    MiTri t;
    I3 *p[3] = {&t.a, &t.b, &t.c};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int k = tri[(long)f * 3 + c];
        if (k < 0 || k >= V) { atomicOr(bad, 1); k = 0; }
        *p[c] = {q[(long)k * 3], q[(long)k * 3 + 1], q[(long)k * 3 + 2]};
    }
    const L3 n = mi_normal(t);
    const int degenerate = (n.x | n.y | n.z) == 0 ? 1 : 0;
    rec[(long)f * 3] = make_int4(t.a.x, t.a.y, t.a.z, degenerate);
    rec[(long)f * 3 + 1] = make_int4(t.b.x, t.b.y, t.b.z, 0);
    rec[(long)f * 3 + 2] = make_int4(t.c.x, t.c.y, t.c.z, 0);
}

// one thread per box: box s holds the triangles [s * per, min(F, (s + 1) * per))
__global__ __launch_bounds__(64) void mi_bounds_kernel(const int4 *__restrict__ rec, int F, int per, int count, int4 *__restrict__ box) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= count) return;
    const long last = ((long)s + 1) * per;
    const long e0 = (long)s * per * 3, e1 = (last < F ? last : (long)F) * 3;
    int4 lo = make_int4(INT_MAX, INT_MAX, INT_MAX, 0), hi = make_int4(INT_MIN, INT_MIN, INT_MIN, 0);
    for (long e = e0; e < e1; ++e) {
        const int4 p = rec[e];
        lo.x = min(lo.x, p.x); lo.y = min(lo.y, p.y); lo.z = min(lo.z, p.z);
        hi.x = max(hi.x, p.x); hi.y = max(hi.y, p.y); hi.z = max(hi.z, p.z);
    }
    box[(long)s * 2] = lo;
    box[(long)s * 2 + 1] = hi;
}

__global__ __launch_bounds__(256) void mi_flags_kernel(const int4 *__restrict__ rec, int F, unsigned char *__restrict__ flags,
                                                       unsigned long long *__restrict__ count) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int d = rec[(long)f * 3].w & 1;
    if (flags) flags[f] = (unsigned char)d;
    if (count && d) atomicAdd(count, 1ull);
}

// lane i = triangle i of A; split blockIdx.y covers the chunks [y * span, min(nchunkB, (y + 1) * span)) of B
template <bool CULL, bool SELF>
__global__ __launch_bounds__(256) void mi_pair_kernel(const int4 *__restrict__ recA, int FA, const int4 *__restrict__ recB, int FB,
                                                      const int4 *__restrict__ tile_box, const int4 *__restrict__ chunk_box, int nchunkB,
                                                      int span, int *__restrict__ hitsA, int *__restrict__ hitsB,
                                                      unsigned long long *__restrict__ pairs, long long capacity,
                                                      unsigned long long *__restrict__ count, unsigned long long *__restrict__ skipped) {
    __shared__ int4 lds[MI_CHUNK * 3];
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = blockIdx.x * MI_CHUNK + tid;
    const long ir = i < FA ? i : FA - 1;
    const int4 ra = recA[ir * 3], rb = recA[ir * 3 + 1], rc = recA[ir * 3 + 2];
    const MiTri A = {mi_i3(ra), mi_i3(rb), mi_i3(rc)};
    const L3 nA = mi_normal(A);
    const bool live = i < FA && !(ra.w & 1);                 // a degenerate triangle intersects nothing
    MiBox box;
    box.lx = live ? mi_min3(A.a.x, A.b.x, A.c.x) : INT_MAX; box.hx = live ? mi_max3(A.a.x, A.b.x, A.c.x) : INT_MIN;
    box.ly = live ? mi_min3(A.a.y, A.b.y, A.c.y) : INT_MAX; box.hy = live ? mi_max3(A.a.y, A.b.y, A.c.y) : INT_MIN;
    box.lz = live ? mi_min3(A.a.z, A.b.z, A.c.z) : INT_MAX; box.hz = live ? mi_max3(A.a.z, A.b.z, A.c.z) : INT_MIN;
    unsigned nskip = 0;
    int c0 = blockIdx.y * span;
    const int c1 = min(nchunkB, c0 + span);
    if constexpr (SELF) c0 = max(c0, (int)blockIdx.x);       // chunk c < blockIdx.x holds only partners j < i
#pragma unroll 1
    for (int c = c0; c < c1; ++c) {
        const int f0 = c * MI_CHUNK;
        const int cnt = min(MI_CHUNK, FB - f0);
        const int tiles = (cnt + MI_TILE - 1) / MI_TILE;
        if constexpr (CULL) {
            // a barrier (every lane is done with the previous chunk) that also tells whether any lane needs this chunk
            const int need = __syncthreads_or(mi_overlap(box, chunk_box[c * 2], chunk_box[c * 2 + 1]));
            if (!need) { nskip += tiles; continue; }         // the same in every lane of the workgroup
        } else {
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int e = tid + 256 * k;
            if (e < cnt * 3) lds[e] = recB[(long)f0 * 3 + e];
        }
        __syncthreads();
#pragma unroll 1
        for (int tt = 0; tt < tiles; ++tt) {
            const int u0 = tt * MI_TILE, u1 = min(cnt, u0 + MI_TILE);
            if constexpr (CULL) {
                const int t = c * MI_CHUNK_TILES + tt;
                if (!__any(mi_overlap(box, tile_box[t * 2], tile_box[t * 2 + 1]))) { nskip += 1; continue; }   // wave-uniform
            }
#pragma unroll 1
            for (int u = u0; u < u1; ++u) {
                const int4 pa = lds[u * 3], pb = lds[u * 3 + 1], pc = lds[u * 3 + 2];
                const int j = f0 + u;
                bool test = live && !(pa.w & 1) && (!SELF || j > i);
                if constexpr (CULL) {
                    const int4 lo = make_int4(mi_min3(pa.x, pb.x, pc.x), mi_min3(pa.y, pb.y, pc.y), mi_min3(pa.z, pb.z, pc.z), 0);
                    const int4 hi = make_int4(mi_max3(pa.x, pb.x, pc.x), mi_max3(pa.y, pb.y, pc.y), mi_max3(pa.z, pb.z, pc.z), 0);
                    test = test && mi_overlap(box, lo, hi);
                }
                if (test) {
                    const MiTri B = {mi_i3(pa), mi_i3(pb), mi_i3(pc)};
                    if (mi_verdict<SELF>(A, nA, B, mi_normal(B))) {
                        if (hitsA) atomicAdd(&hitsA[i], 1);
                        if (hitsB) atomicAdd(&hitsB[j], 1);
                        const unsigned long long slot = atomicAdd(count, 1ull);
                        if (pairs && slot < (unsigned long long)capacity) pairs[slot] = ((unsigned long long)(unsigned)i << 32) | (unsigned)j;
                    }
                }
            }
        }
    }
    if constexpr (CULL) {
        if (skipped && lane == 0 && i < FA && nskip) atomicAdd(skipped, (unsigned long long)nskip);
    }
}

}  // namespace surfd

using namespace surfd;

struct surfd_isect {
    int F = 0, L = 0, ntile = 0, nchunk = 0;
    int4 *rec = nullptr;              // [F] triangles of 3 int4
    int4 *tile_box = nullptr;         // [ntile] boxes of 2 int4
    int4 *chunk_box = nullptr;        // [nchunk]
    unsigned long long *counters = nullptr;   // [0] the pair count of a call without a count pointer, [1] skipped (wave, tile) visits
    long long last_total = 0;         // the visits the last call with SURFD_ISECT_COUNT_SKIPPED had in all
};

static int mi_run(const char *who, surfd_isect *a, surfd_isect *b, bool self, int flags, int32_t *hits_a, int32_t *hits_b, int64_t *pairs,
                  int64_t capacity, int64_t *count, hipStream_t st) {
    if (!a || !b) SURFD_FAIL(SURFD_ERR_ARG, "%s: null handle", who);
    if (flags & ~(SURFD_ISECT_BRUTE_FORCE | SURFD_ISECT_COUNT_SKIPPED)) SURFD_FAIL(SURFD_ERR_ARG, "%s: unknown flags 0x%x", who, flags);
    if (capacity < 0) SURFD_FAIL(SURFD_ERR_ARG, "%s: capacity = %lld is negative", who, (long long)capacity);
    if (capacity > 0 && !pairs) SURFD_FAIL(SURFD_ERR_ARG, "%s: capacity = %lld without a pairs buffer", who, (long long)capacity);
    if (a->L != b->L)
        SURFD_FAIL(SURFD_ERR_ARG, "%s: the two meshes were snapped to different lattices (lattice_log2 = %d and %d)", who, a->L, b->L);
    unsigned long long *cnt = count ? (unsigned long long *)count : a->counters;
    HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), st));
    if (hits_a) HIP_TRY(hipMemsetAsync(hits_a, 0, (size_t)a->F * sizeof(int32_t), st));
    if (hits_b) HIP_TRY(hipMemsetAsync(hits_b, 0, (size_t)b->F * sizeof(int32_t), st));
    const bool brute = flags & SURFD_ISECT_BRUTE_FORCE;
    unsigned long long *skipped = nullptr;
    if (flags & SURFD_ISECT_COUNT_SKIPPED) {
        HIP_TRY(hipMemsetAsync(a->counters + 1, 0, sizeof(unsigned long long), st));
        long long total = 0;                                  // the (wave, tile) visits of the brute-force path
        for (long x = 0; x * MI_CHUNK < a->F; ++x) {
            const long waves = ceil_div<long>(std::min<long>(MI_CHUNK, a->F - x * MI_CHUNK), 64);
            total += waves * (self ? b->ntile - x * MI_CHUNK_TILES : b->ntile);
        }
        a->last_total = total;
        skipped = brute ? nullptr : a->counters + 1;
    }
    const Split sp = split_units(a->F, MI_CHUNK, b->nchunk, MI_MAX_SPLITS);   // splits of the partner chunk range per block of triangles
    const int span = sp.span;
    const dim3 grid((unsigned)ceil_div(a->F, MI_CHUNK), (unsigned)sp.S);
#define MI_LAUNCH(CULL, SELF)                                                                                                        \
    hipLaunchKernelGGL((mi_pair_kernel<CULL, SELF>), grid, dim3(256), 0, st, (const int4 *)a->rec, a->F, (const int4 *)b->rec, b->F, \
                       (const int4 *)b->tile_box, (const int4 *)b->chunk_box, b->nchunk, span, hits_a, hits_b,                       \
                       (unsigned long long *)pairs, (long long)capacity, cnt, skipped)
    if (self) { if (brute) MI_LAUNCH(false, true); else MI_LAUNCH(true, true); }
    else { if (brute) MI_LAUNCH(false, false); else MI_LAUNCH(true, false); }
#undef MI_LAUNCH
    LAUNCH_CHECK();
    return SURFD_OK;
}

extern "C" {

int surfd_isect_create(const float *vertices, int V, const int32_t *triangles, int F, int lattice_log2, surfd_stream s, surfd_isect **out) {
    int rc = mesh_create_args("surfd_isect_create", vertices, V, triangles, F, out, INT_MAX);    // the size test below is this file's
    if (rc != SURFD_OK) return rc;
    if (lattice_log2 < -MI_MAX_LOG2 || lattice_log2 > MI_MAX_LOG2)
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_isect_create: lattice_log2 = %d outside -%d .. %d", lattice_log2, MI_MAX_LOG2, MI_MAX_LOG2);
    if (F > (1 << 28) || V > (1 << 28)) SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_isect_create: V = %d, F = %d is beyond the supported size", V, F);
    hipStream_t st = as_stream(s);
    surfd_isect *m = new surfd_isect();
    m->F = F;
    m->L = lattice_log2;
    m->ntile = ceil_div(F, MI_TILE);
    m->nchunk = ceil_div(F, MI_CHUNK);
    int *q = nullptr;                                         // snapped vertices
    CreateFlags bad(2);                                       // [0] refused vertices, [1] bad indices
    int flag[2] = {0, 0};
    auto run = [&]() -> int {
        HIP_TRY(hipMalloc(&m->rec, (size_t)F * 3 * sizeof(int4)));
        HIP_TRY(hipMalloc(&m->tile_box, (size_t)m->ntile * 2 * sizeof(int4)));
        HIP_TRY(hipMalloc(&m->chunk_box, (size_t)m->nchunk * 2 * sizeof(int4)));
        HIP_TRY(hipMalloc(&m->counters, 2 * sizeof(unsigned long long)));
        HIP_TRY(hipMalloc(&q, (size_t)V * 3 * sizeof(int)));
        if (int e = bad.init(st)) return e;
        HIP_TRY(hipMemsetAsync(m->counters, 0, 2 * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(mi_snap_kernel, dim3((unsigned)ceil_div(V, 256)), dim3(256), 0, st, vertices, V, ldexpf(1.f, lattice_log2), q, bad.dev);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(mi_gather_kernel, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, st, (const int *)q, V, triangles, F, m->rec, bad.dev + 1);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(mi_bounds_kernel, dim3((unsigned)ceil_div(m->ntile, 64)), dim3(64), 0, st, (const int4 *)m->rec, F, MI_TILE, m->ntile,
                           m->tile_box);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(mi_bounds_kernel, dim3((unsigned)ceil_div(m->nchunk, 64)), dim3(64), 0, st, (const int4 *)m->rec, F, MI_CHUNK,
                           m->nchunk, m->chunk_box);
        LAUNCH_CHECK();
        return bad.read(flag, st);
    };
    rc = run();
    (void)hipFree(q);
    if (rc == SURFD_OK && flag[0]) {
        set_error("surfd_isect_create: %d of %d vertices are NaN or beyond the lattice (|x * 2^%d| > 2^19)", flag[0], V, lattice_log2);
        rc = SURFD_ERR_ARG;
    } else if (rc == SURFD_OK && flag[1]) {
        rc = mesh_bad_index("surfd_isect_create", V);
    }
    if (rc != SURFD_OK) { surfd_isect_destroy(m); return rc; }
    *out = m;
    return SURFD_OK;
}

void surfd_isect_destroy(surfd_isect *m) {
    if (!m) return;
    (void)hipFree(m->rec); (void)hipFree(m->tile_box); (void)hipFree(m->chunk_box); (void)hipFree(m->counters);
    delete m;
}

int surfd_isect_num_triangles(const surfd_isect *m) { return m ? m->F : 0; }

int surfd_isect_degenerate(surfd_isect *m, uint8_t *flags, int64_t *count, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_isect_degenerate: null handle");
    hipStream_t st = as_stream(s);
    if (count) HIP_TRY(hipMemsetAsync(count, 0, sizeof(int64_t), st));
    if (!flags && !count) return SURFD_OK;
    hipLaunchKernelGGL(mi_flags_kernel, dim3((unsigned)ceil_div(m->F, 256)), dim3(256), 0, st, (const int4 *)m->rec, m->F, flags,
                       (unsigned long long *)count);
    LAUNCH_CHECK();
    return SURFD_OK;
}

int surfd_isect_self(surfd_isect *m, int flags, int32_t *hits, int64_t *pairs, int64_t capacity, int64_t *count, surfd_stream s) {
    return mi_run("surfd_isect_self", m, m, true, flags, hits, hits, pairs, capacity, count, as_stream(s));
}

int surfd_isect_between(surfd_isect *a, surfd_isect *b, int flags, int32_t *hits_a, int32_t *hits_b, int64_t *pairs, int64_t capacity,
                        int64_t *count, surfd_stream s) {
    if (a && a == b) SURFD_FAIL(SURFD_ERR_ARG, "surfd_isect_between: the two handles are the same (surfd_isect_self is the call for one mesh)");
    return mi_run("surfd_isect_between", a, b, false, flags, hits_a, hits_b, pairs, capacity, count, as_stream(s));
}

int surfd_isect_skipped(surfd_isect *m, int64_t *skipped, int64_t *total, surfd_stream s) {
    if (!m || !skipped || !total) SURFD_FAIL(SURFD_ERR_ARG, "surfd_isect_skipped: null argument");
    return read_counter(m->counters + 1, m->last_total, skipped, total, as_stream(s));
}

}  // extern "C"
