// Ray casting on a triangle mesh: first hit per ray and the number of triangles a ray meets.  The ray half of open3d's
// RaycastingScene (cast_rays, count_intersections, and through the crossing count compute_occupancy / compute_signed_distance,
// which the reference's AutoEncoder/utils.py:242-264 calls); the closest-point half is meshdist.hip.  fp32 in, fp64 pair
// arithmetic on the VALU, no MFMA, no atomics except the integer one of the skipped-tile count.
//
// The contract of one (ray, triangle) pair: rc_ray() and rc_pair(), restated operation for operation in tests/raycast_ref.py.
// Every operation is ONE fp64 IEEE rounding (the library is built with -ffp-contract=off; nothing in the pair test is an fma)
// and only + - * / occur.  The form is the shear-and-scale test of Woop, Benthin and Wald (Watertight Ray/Triangle
// Intersection, JCGT 2013):
//   ray     ok = all six components finite and d != 0.  kz = the axis of the largest |d| (lower axis on a tie), kx = kz + 1,
//           ky = kz + 2 (mod 3), exchanged when d[kz] < 0 so that the winding survives;  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz],
//           Sz = 1 / d[kz].
//   vertex  Pz = P[kz] - o[kz];  Px = (P[kx] - o[kx]) - Sx Pz;  Py = (P[ky] - o[ky]) - Sy Pz: a function of the vertex and the
//           ray alone.
//   edges   U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax.  The triangle on the other side of an edge forms the same
//           two products and subtracts them the other way round, so its value is the exact negative: no ray slips between two
//           triangles, none is counted by both.  det = (U + V) + W; det == 0 (no area in the ray's frame) is never a hit.
//           s = sign(det); a hit needs s U, s V, s W each > 0, or == 0 on an edge that owns its zero.  After the
//           normalisation by s the triangle runs counter-clockwise along eU = s (B - C), eV = s (C - A), eW = s (A - B) (sheared
//           x, y); an edge owns its zero when e.y < 0 or (e.y == 0 and e.x < 0): the top-left rule.  The neighbour's edge vector
//           is the exact negative, so exactly one of the two owns a shared edge where the surface crosses the ray; where it
//           folds back both or neither do (count 2 or 0).
//   t       T = (U Az + V Bz) + W Cz;  t = float((Sz T) / det), -0 made +0;  a hit needs tmin <= t < tmax on that fp32 value.
//   winner  of a cast: the minimum of the 64-bit key bits(t) << 32 | triangle (t >= +0: its bits order like its value).
//   finish  for the winner only: uv = float(V / det), float(W / det);  normal = (B - A) x (C - A) in fp64, divided by its fp64
//           length (sqrt of (nx nx + ny ny) + nz nz), rounded to fp32; zero where that length is 0.
//   miss    t = +inf, tri = -1, uv = normal = 0, count = 0; also for a ray that is not ok, whose components are never used.
// The key of a pair does not depend on the traversal, and the minimum of a total order does not depend on the order in which
// it is taken: any split count, tile order or culling gives the same bits.
//
// Kernels:
//   rc_gather_kernel   (vertices, triangles) -> three float4 per triangle (A, B, C); an index outside [0, V) raises a flag.
//   rc_bounds_kernel   one bounding sphere per tile of 32 triangles and per chunk of 8 tiles.
//   rc_trace_kernel    one ray per lane, 256 rays per workgroup; kz, the shear and the origin stay in registers.  The triangles
//                      of one split stream through LDS in chunks of 256; all lanes of a wave read the same triangle at the same
//                      time (a broadcast).  grid.y = the splits of the triangle range.  <CULL>: a chunk is not staged when no
//                      lane of the workgroup can hit its sphere, a tile is skipped when no lane of the wave can.  <COUNT>:
//                      counts hits instead of keeping the smallest key.
//   rc_finish_*_kernel the minimum key / the sum of the counts over the splits; the cast one evaluates the winner once more.
//
// Culling bound (rc_cannot_hit), derived, not tuned.  u = 2^-24.  A sphere (c, rs) of a tile: c = the middle of the bounding
// box, r~ = the largest computed vertex distance (>= r (1 - 4u), r the true one), rs = r~ (1 + 2^-12) + 2^-60.  A lane may
// only vote for a skip when its ray is TAME: |o_i| <= 2^20 and 2^-20 <= max |d_i| <= 2^20, and a sphere with a |c_i| > 2^20 or a
// radius that is not finite gets rs = +inf and is never skipped; inside these ranges no product below overflows and the
// absolute error of an underflowing product (<= 2^-149) reaches the results by at most 2^-84, which the 2^-60 in rs covers.
// A pair that the test accepts has the true line within the pair test's own fp64 rounding (2^-50 relative to |P - o|, see the
// caveat) of a point of the triangle, hence of the sphere, and its t~ = (Sz T) / det is a combination of Sz Az, Sz Bz, Sz Cz
// with the computed weights U / det .. >= 0 that sum to 1: it lies between the smallest and the largest of the three.
//   1  line: w = fl(c - o), s = fl(fl(w.d) / fl(d.d)), D~2 = |fl(w - s d)|^2, all fp32.  |s - s*| |d| <= 8.1u |w| (the dot
//      products carry 3u |w| |d| and 3u |d|^2, w itself u |w|, the division u), the difference vector 2u (|w| + D) more, its
//      squared length 3u: D~ <= D (1 + 5u) + 11u |w| for the true distance D from c to the line.  A hit has D <= r <= rho with
//      rho = rs / (1 + 2^-13) (r <= r~ / (1 - 4u)), and (rho (1 + 5u) + y)^2 <= rho^2 (1 + 5u)^2 (1 + 2^-11) + y^2 (1 + 2^11)
//      with y = 11u |w|:
//      y^2 (1 + 2^11) = 121 * 2049 * 2^-48 |w|^2 < 2^-30 |w|^2.  The test skips when D~2 > rs^2 (1 + 2^-10) + 2^-27 fl(w.w):
//      a factor 2 on the first term's margin and 8 on the second in hand for the roundings of the right-hand side itself.
//   2  slab along kz: q = fl(fl(c[kz] - o[kz]) * fl(1 / d[kz])) is within 3u |q| of the centre's parameter, h = fl(rs |1 / d[kz]|)
//      is above the half width r / |d[kz]| of the parameters of everything in the sphere, so every t~ of the tile lies in
//      [q - h, q + h] and its fp32 value within u (|q| + h) of that.  With e = 2^-20 (|q| + h) + 2^-100 (the roundings listed and
//      those of the test's own three operations stay below 2^-21 (|q| + h)) the test skips when (q - h) - e > hi or
//      (q + h) + e < tmin;  hi = tmax, or in a cast the lane's best t so far: strict, so a pair that ties the best t and might
//      win on the index is never skipped.
//   A NaN or Inf anywhere in the test makes its compares false: no skip.
//   Caveat: the pair test itself rounds (2^-53 (|Px Qy| + |Py Qx|) per edge function).  A triangle whose sheared area is below
//   that, a needle seen edge-on, can be reported hit by a ray that passes its supporting line outside the triangle; the culled
//   and the brute-force path can differ for such a pair only.  The restatement and SURFD_RAY_BRUTE_FORCE always agree.
//
// Hierarchy (SURFD_RAY_BVH, the bvr_ kernels; built by meshbvh.hip, whose header describes the tree).  bvr_trace_kernel: one ray
// per lane, 256 rays per workgroup, every lane walks the whole implicit tree on its own (meshbvh_layout.h: level, node and one
// 64-bit word of waiting children; no stack, no private array), so the triangle range is not split and the existing finish
// kernels run with S = 1.  A leaf's triangles go through rc_pair() with the handle's own index, so keys and ties are those of
// the other two paths; every triangle is in exactly one leaf, so a crossing is counted once.  The children of a node are taken
// in ascending order, whatever the ray: the result cannot depend on the order (the minimum of a total order, a sum of integers).
//
// Box bound (bvr_cannot_hit), derived like rc_cannot_hit's, u = 2^-24.  A lane may skip only when its ray is TAME as above and
// the box is finite (a box of meshbvh.hip has |coordinates| <= 2^20 or is (-inf, +inf)^3, which fails M < inf below).
//   What an accepted pair guarantees.  With the computed weights (U, V, W) / det >= 0 (sum 1 to 2^-52) the fp64 value
//   t* = (Sz T) / det is the same combination of the vertices' own parameters along kz, and o + t* d is the same combination p
//   of the vertices, minus (in the two sheared axes) the residual rho = (U Ax + V Bx + W Cx) / det, which is zero in exact
//   arithmetic.  p lies in every box that holds the vertices.  |rho| is the rounding of the edge functions over det: below
//   2^-50 |P - o| except for the needle of the caveat above, exactly the "true line within the pair test's own rounding of a point
//   of the triangle" that bound 1 of rc_cannot_hit relies on.  So for every axis j: o_j + t* d_j in [lo_j - |rho|, hi_j + |rho|].
//   1  positions: a_j = fl(lo_j - o_j), b_j = fl(hi_j - o_j), M = the largest of the six sizes, s = fl(2^-16 M + 2^-60),
//      a'_j = fl(a_j - s), b'_j = fl(b_j + s).  The four roundings are below 4u M = 2^-22 M, so [a'_j, b'_j] holds
//      [lo_j - o_j - 2^-17 M, hi_j - o_j + 2^-17 M]: a factor 2 on s in hand, and 2^-17 M against |rho| <= 2^-50 |P - o| <= 2^-49 M
//      leaves what the needle caveat is about the same room rc_cannot_hit gives it or more: that test passes a line up to
//      sqrt(rs^2 (1 + 2^-10) + 2^-27 |w|^2) - rs from its sphere, at its least (rs = 2^-8.5 |w|) 2^-18.5 |w| <= 2^-17.7 M.
//   2  an axis with |d_j| < 2^-40 max |d| is PARALLEL: over every t with |t d_kz| <= M + s the ray moves along j by less than
//      2^-39 M, inside the room of 1.  Such an axis skips when a'_j > 0 or b'_j < 0 and constrains t in no other way.  d_j = 0 is
//      the plain case of it; no division by a small d_j occurs.
//   3  every other axis (kz always is one): i_j = fl(1 / d_j), 2^-20 <= |i_j| <= 2^60, t1 = fl(a'_j i_j), t2 = fl(b'_j i_j), each
//      within 2u of the exact quotient and never a NaN or an Inf (|a'_j| < 2^22); t* lies between the exact quotients and the
//      fp32 t of the pair within u |t*| of t*.  With e_j = fl(2^-20 max(|t1|, |t2|) + 2^-100) (needed: 3.1u max, so a factor 5 in
//      hand for e_j's own rounding and that of the two operations below) the pair's t lies in [min(t1, t2) - e_j, max(t1, t2) + e_j].
//      near = the largest lower end, far = the smallest upper end over these axes.  The box is skipped when near > far, when
//      far < tmin, or when near > hi; hi = tmax, or in a cast the lane's best t so far: STRICT, so a pair that ties the best t
//      and might win on the index is never skipped.
//   A NaN anywhere makes the compares false: no skip.  A ray that is not ok walks nothing; a ray that is ok but not tame skips
//   nothing and meets every triangle.  The needle caveat carries over as it stands; nothing else is excused.
//
// Bounds: ray n >= R reads ray R - 1 and writes nothing.  Staging reads records below F only; LDS is indexed with u < cnt <= 256.
// The sphere arrays are indexed with c < nchunk and c * 8 + tt < ntile.  Partial results [S, R] live in the handle's arena
// (meshscene.h).  Hazards: the LDS chunk is bracketed by a barrier on both sides.  bvr_trace_kernel reads
// node off[level] + node with node < size[level] and leaf_tri[child] with child < nleaf: only children whose box exists are ever
// entered (meshbvh_layout.h); a triangle index outside [0, F) is not read.  Its LDS holds the level offsets, written once
// before one barrier.
#include "common.h"
#include "meshbvh.h"
#include "meshscene.h"
#include <cfloat>
#include <climits>
#include <cmath>
#include <algorithm>

namespace surfd {

constexpr int RC_TILE = 32;                       // triangles per bounding sphere
constexpr int RC_CHUNK_TILES = 8;
constexpr int RC_CHUNK = RC_TILE * RC_CHUNK_TILES;    // triangles per LDS chunk, and rays per workgroup
constexpr int RC_MAX_SPLITS = 64;
constexpr int RC_REC4 = 3;                        // float4 per triangle: A, B, C
constexpr unsigned long long RC_MISS = 0xFFFFFFFFFFFFFFFFull;
constexpr float RC_TAME_HI = 1048576.f;           // 2^20
constexpr float RC_TAME_LO = 9.5367431640625e-07f;   // 2^-20
constexpr float RC_RADIUS_REL = 2.44140625e-04f;  // 2^-12
constexpr float RC_RADIUS_ABS = 8.67361737988403547e-19f;   // 2^-60
constexpr float RC_R2_MARGIN = 9.765625e-04f;     // 2^-10
constexpr float RC_W2_MARGIN = 7.450580596923828125e-09f;   // 2^-27
constexpr float RC_T_REL = 9.5367431640625e-07f;  // 2^-20
constexpr float RC_T_ABS = 7.88860905221011805e-31f;        // 2^-100

constexpr float BVR_PARALLEL = 9.094947017729282379e-13f;      // 2^-40
constexpr float BVR_POS_REL = 1.52587890625e-05f;              // 2^-16
constexpr float BVR_POS_ABS = 8.67361737988403547e-19f;        // 2^-60

struct RcRay {
    double ox, oy, oz;       // the origin, permuted to (kx, ky, kz)
    double Sx, Sy, Sz;
    int kx, ky, kz;
    bool ok;
};

__host__ __device__ __forceinline__ float rc_sel(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

__host__ __device__ __forceinline__ bool rc_finite(float x) { return x - x == 0.f; }

__host__ __device__ __forceinline__ RcRay rc_ray(float ox, float oy, float oz, float dx, float dy, float dz) {
    RcRay r;
    r.ok = rc_finite(ox) && rc_finite(oy) && rc_finite(oz) && rc_finite(dx) && rc_finite(dy) && rc_finite(dz) &&
           (dx != 0.f || dy != 0.f || dz != 0.f);
    if (!r.ok) { ox = oy = oz = dx = dy = 0.f; dz = 1.f; }
    const float ax = __builtin_fabsf(dx), ay = __builtin_fabsf(dy), az = __builtin_fabsf(dz);
    const int kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    int kx = kz == 2 ? 0 : kz + 1;
    int ky = kx == 2 ? 0 : kx + 1;
    const double dk = (double)rc_sel(dx, dy, dz, kz);
    if (dk < 0.0) { const int t = kx; kx = ky; ky = t; }
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.ox = (double)rc_sel(ox, oy, oz, kx);
    r.oy = (double)rc_sel(ox, oy, oz, ky);
    r.oz = (double)rc_sel(ox, oy, oz, kz);
    r.Sx = (double)rc_sel(dx, dy, dz, kx) / dk;
    r.Sy = (double)rc_sel(dx, dy, dz, ky) / dk;
    r.Sz = 1.0 / dk;
    return r;
}

__host__ __device__ __forceinline__ bool rc_owns(double s, double ex, double ey) {
    ex = s * ex; ey = s * ey;
    return ey < 0.0 || (ey == 0.0 && ex < 0.0);
}

// The pair test.  true = a hit with tmin <= t < tmax; V, W, det feed the finish (dead code elsewhere).
__host__ __device__ __forceinline__ bool rc_pair(const RcRay &r, float4 a, float4 b, float4 c, float tmin, float tmax, float &t,
                                                 double &V, double &W, double &det) {
    const double Az = (double)rc_sel(a.x, a.y, a.z, r.kz) - r.oz;
    const double Ax = ((double)rc_sel(a.x, a.y, a.z, r.kx) - r.ox) - r.Sx * Az;
    const double Ay = ((double)rc_sel(a.x, a.y, a.z, r.ky) - r.oy) - r.Sy * Az;
    const double Bz = (double)rc_sel(b.x, b.y, b.z, r.kz) - r.oz;
    const double Bx = ((double)rc_sel(b.x, b.y, b.z, r.kx) - r.ox) - r.Sx * Bz;
    const double By = ((double)rc_sel(b.x, b.y, b.z, r.ky) - r.oy) - r.Sy * Bz;
    const double Cz = (double)rc_sel(c.x, c.y, c.z, r.kz) - r.oz;
    const double Cx = ((double)rc_sel(c.x, c.y, c.z, r.kx) - r.ox) - r.Sx * Cz;
    const double Cy = ((double)rc_sel(c.x, c.y, c.z, r.ky) - r.oy) - r.Sy * Cz;
    const double U = Cx * By - Cy * Bx;
    V = Ax * Cy - Ay * Cx;
    W = Bx * Ay - By * Ax;
    det = (U + V) + W;
    const double s = det > 0.0 ? 1.0 : -1.0;
    const double nU = s * U, nV = s * V, nW = s * W;
    const bool in = (nU > 0.0 || (nU == 0.0 && rc_owns(s, Bx - Cx, By - Cy))) &&
                    (nV > 0.0 || (nV == 0.0 && rc_owns(s, Cx - Ax, Cy - Ay))) &&
                    (nW > 0.0 || (nW == 0.0 && rc_owns(s, Ax - Bx, Ay - By)));
    if (!in || !(det != 0.0)) return false;
    const double T = (U * Az + V * Bz) + W * Cz;
    t = (float)((r.Sz * T) / det);
    t = t + 0.f;                                            // -0 -> +0 (not folded: the library is not built with fast-math)
    return t >= tmin && t < tmax;
}

__host__ __device__ __forceinline__ unsigned rc_float_bits(float x) {
    union { float f; unsigned u; } v;
    v.f = x;
    return v.u;
}

__host__ __device__ __forceinline__ float rc_bits_float(unsigned x) {
    union { float f; unsigned u; } v;
    v.u = x;
    return v.f;
}

__device__ __forceinline__ float rc_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return fmaf(az, bz, fmaf(ay, by, ax * bx));
}

// what a lane needs of its ray to vote on a sphere (fp32)
struct RcCull {
    float ox, oy, oz, dx, dy, dz;
    float dd;            // d.d
    float ok_z, iz;      // o[kz], 1 / d[kz]
    int kz;
    bool dead;           // no ray here, or a ray that hits nothing: always votes for the skip
    bool tame;           // the bound holds for this ray (header); otherwise it never votes for a skip
};

__device__ __forceinline__ RcCull rc_cull_setup(float ox, float oy, float oz, float dx, float dy, float dz, int kz, bool live) {
    RcCull q;
    q.ox = ox; q.oy = oy; q.oz = oz; q.dx = dx; q.dy = dy; q.dz = dz;
    q.dd = rc_dot(dx, dy, dz, dx, dy, dz);
    q.kz = kz;
    q.ok_z = rc_sel(ox, oy, oz, kz);
    const float dk = rc_sel(dx, dy, dz, kz);
    q.iz = __fdiv_rn(1.f, dk);
    q.dead = !live;
    const float adk = fabsf(dk);
    q.tame = fabsf(ox) <= RC_TAME_HI && fabsf(oy) <= RC_TAME_HI && fabsf(oz) <= RC_TAME_HI && adk >= RC_TAME_LO && adk <= RC_TAME_HI;
    return q;
}

// true where no triangle inside the sphere (c.xyz, rs = c.w) can be a hit of this lane's ray with tmin <= t < (or, in a cast,
// <=) hi: the two tests of the header
__device__ __forceinline__ bool rc_cannot_hit(float4 c, const RcCull &q, float tmin, float hi) {
    const float wx = c.x - q.ox, wy = c.y - q.oy, wz = c.z - q.oz;
    const float s = __fdiv_rn(rc_dot(wx, wy, wz, q.dx, q.dy, q.dz), q.dd);
    const float ex = wx - s * q.dx, ey = wy - s * q.dy, ez = wz - s * q.dz;
    const float D2 = rc_dot(ex, ey, ez, ex, ey, ez);
    const float W2 = rc_dot(wx, wy, wz, wx, wy, wz);
    const float r2 = c.w * c.w;
    const float rhs = fmaf(W2, RC_W2_MARGIN, fmaf(r2, RC_R2_MARGIN, r2));
    const bool off_line = D2 > rhs && D2 < INFINITY;
    const float z = rc_sel(c.x, c.y, c.z, q.kz) - q.ok_z;
    const float p = z * q.iz;
    const float h = c.w * fabsf(q.iz);
    const float e = fmaf(fabsf(p) + h, RC_T_REL, RC_T_ABS);
    const bool off_range = (p - h) - e > hi || (p + h) + e < tmin;
    return q.dead || (q.tame && (off_line || off_range));
}

// one thread per triangle
__global__ __launch_bounds__(256) void rc_gather_kernel(const float *__restrict__ vtx, int V, const int *__restrict__ tri, int F,
                                                        float4 *__restrict__ rec, int *__restrict__ bad) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int k = tri[(long)f * 3 + c];
        if (k < 0 || k >= V) { atomicOr(bad, 1); k = 0; }
        rec[(long)f * RC_REC4 + c] = make_float4(vtx[(long)k * 3], vtx[(long)k * 3 + 1], vtx[(long)k * 3 + 2], 0.f);
    }
}

// one thread per sphere: sphere s holds the triangles [s * per, min(F, (s + 1) * per))
__global__ __launch_bounds__(64) void rc_bounds_kernel(const float4 *__restrict__ rec, int F, int per, int count, float4 *__restrict__ sph) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= count) return;
    const long e0 = (long)s * per * RC_REC4, e1 = (long)min(F, (s + 1) * per) * RC_REC4;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long e = e0; e < e1; ++e) {
        const float4 p = rec[e];
        lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
        hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
    }
    const float cx = 0.5f * lo[0] + 0.5f * hi[0], cy = 0.5f * lo[1] + 0.5f * hi[1], cz = 0.5f * lo[2] + 0.5f * hi[2];
    float r2 = 0.f;
    bool finite = true;
    for (long e = e0; e < e1; ++e) {
        const float4 p = rec[e];
        const float x = p.x - cx, y = p.y - cy, z = p.z - cz;
        const float d2 = rc_dot(x, y, z, x, y, z);
        finite = finite && d2 < INFINITY;                     // false for a NaN as well
        r2 = fmaxf(r2, d2);
    }
    const float r = __fsqrt_rn(r2);
    float rs = fmaf(r, RC_RADIUS_REL, r) + RC_RADIUS_ABS;
    const bool tame = finite && fabsf(cx) <= RC_TAME_HI && fabsf(cy) <= RC_TAME_HI && fabsf(cz) <= RC_TAME_HI;
    if (!tame) rs = INFINITY;
    sph[s] = make_float4(tame ? cx : 0.f, tame ? cy : 0.f, tame ? cz : 0.f, rs);
}

// rays [R, 6]; split blockIdx.y covers the chunks [y * span, min(nchunk, (y + 1) * span)); partial results pk / pc [S, R]
template <bool CULL, bool COUNT>
__global__ __launch_bounds__(256) void rc_trace_kernel(const float4 *__restrict__ rec, int F, const float4 *__restrict__ tile_sph,
                                                       const float4 *__restrict__ chunk_sph, int nchunk, int span,
                                                       const float *__restrict__ rays, int R, float tmin, float tmax,
                                                       unsigned long long *__restrict__ pk, int *__restrict__ pc,
                                                       unsigned long long *__restrict__ skipped) {
    __shared__ float4 lds[RC_CHUNK * RC_REC4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = blockIdx.x * RC_CHUNK + tid;
    const long nr = n < R ? n : R - 1;
    const float ox = rays[nr * 6], oy = rays[nr * 6 + 1], oz = rays[nr * 6 + 2];
    const float dx = rays[nr * 6 + 3], dy = rays[nr * 6 + 4], dz = rays[nr * 6 + 5];
    const RcRay r = rc_ray(ox, oy, oz, dx, dy, dz);
    const bool live = n < R && r.ok;
    RcCull q;
    if constexpr (CULL) q = rc_cull_setup(ox, oy, oz, dx, dy, dz, r.kz, live);
    unsigned long long key = RC_MISS;
    int hits = 0;
    float hi = tmax;
    unsigned nskip = 0;
    const int c0 = blockIdx.y * span, c1 = min(nchunk, c0 + span);
#pragma unroll 1
    for (int c = c0; c < c1; ++c) {
        const int f0 = c * RC_CHUNK;
        const int cnt = min(RC_CHUNK, F - f0);
        const int tiles = (cnt + RC_TILE - 1) / RC_TILE;
        if constexpr (CULL) {
            // a barrier (every lane is done with the previous chunk) that also tells whether any lane needs this chunk
            const int need = __syncthreads_or(!rc_cannot_hit(chunk_sph[c], q, tmin, hi));
            if (!need) { nskip += tiles; continue; }         // the same in every lane of the workgroup
        } else {
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < RC_REC4; ++i) {
            const int e = tid + 256 * i;
            if (e < cnt * RC_REC4) lds[e] = rec[(long)f0 * RC_REC4 + e];
        }
        __syncthreads();
#pragma unroll 1
        for (int tt = 0; tt < tiles; ++tt) {
            const int u0 = tt * RC_TILE, u1 = min(cnt, u0 + RC_TILE);
            if constexpr (CULL) {
                if (__all(rc_cannot_hit(tile_sph[c * RC_CHUNK_TILES + tt], q, tmin, hi))) { nskip += 1; continue; }   // wave-uniform
            }
            // the counting form is a reduction, which the loop vectoriser would interleave 32 deep (256 registers and scratch)
#pragma clang loop unroll_count(2) vectorize(disable) interleave(disable)
            for (int u = u0; u < u1; ++u) {
                float t = 0.f;
                double V, W, det;
                const bool hit = rc_pair(r, lds[u * RC_REC4], lds[u * RC_REC4 + 1], lds[u * RC_REC4 + 2], tmin, tmax, t, V, W, det) && live;
                if constexpr (COUNT) {
                    hits += hit ? 1 : 0;
                } else {
                    const unsigned long long k = ((unsigned long long)rc_float_bits(t) << 32) | (unsigned)(f0 + u);
                    key = hit && k < key ? k : key;
                }
            }
            if constexpr (CULL && !COUNT) hi = key == RC_MISS ? tmax : rc_bits_float((unsigned)(key >> 32));
        }
    }
    if (n < R) {
        if constexpr (COUNT) pc[(long)blockIdx.y * R + n] = hits;
        else pk[(long)blockIdx.y * R + n] = key;
    }
    if constexpr (CULL) {
        if (skipped && lane == 0 && n < R && nskip) atomicAdd(skipped, (unsigned long long)nskip);
    }
}

// what a lane needs of its ray to test a box (fp32): the origin, 1 / d_j of the axes that are not parallel, and which are
struct BvrRay {
    float ox, oy, oz, ix, iy, iz;
    bool px, py, pz;     // parallel axes (header, 2)
    bool tame;
};

__device__ __forceinline__ BvrRay bvr_setup(float ox, float oy, float oz, float dx, float dy, float dz) {
    BvrRay q;
    q.ox = ox; q.oy = oy; q.oz = oz;
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    const float m = fmaxf(ax, fmaxf(ay, az));
    const float lim = m * BVR_PARALLEL;
    q.px = !(ax >= lim) || ax == 0.f; q.py = !(ay >= lim) || ay == 0.f; q.pz = !(az >= lim) || az == 0.f;
    q.ix = q.px ? 0.f : __fdiv_rn(1.f, dx);
    q.iy = q.py ? 0.f : __fdiv_rn(1.f, dy);
    q.iz = q.pz ? 0.f : __fdiv_rn(1.f, dz);
    q.tame = fabsf(ox) <= RC_TAME_HI && fabsf(oy) <= RC_TAME_HI && fabsf(oz) <= RC_TAME_HI && m >= RC_TAME_LO && m <= RC_TAME_HI;
    return q;
}

// one axis of the box test: a, b = the widened box relative to the origin.  Returns true where the axis alone rules the box out
__device__ __forceinline__ bool bvr_axis(float a, float b, float inv, bool parallel, float &near, float &far) {
    const float t1 = a * inv, t2 = b * inv;
    const float e = fmaf(fmaxf(fabsf(t1), fabsf(t2)), RC_T_REL, RC_T_ABS);
    const float n = fminf(t1, t2) - e, f = fmaxf(t1, t2) + e;
    near = parallel ? near : fmaxf(near, n);
    far = parallel ? far : fminf(far, f);
    return parallel && (a > 0.f || b < 0.f);
}

// true where no triangle with all its vertices inside the box can be a hit of this lane's ray with tmin <= t < (or, in a cast,
// <=) hi: the bound of the header
__device__ __forceinline__ bool bvr_cannot_hit(float lox, float loy, float loz, float hix, float hiy, float hiz, const BvrRay &q,
                                               float tmin, float hi) {
    float ax = lox - q.ox, ay = loy - q.oy, az = loz - q.oz, bx = hix - q.ox, by = hiy - q.oy, bz = hiz - q.oz;
    const float M = fmaxf(fmaxf(fmaxf(fabsf(ax), fabsf(bx)), fmaxf(fabsf(ay), fabsf(by))), fmaxf(fabsf(az), fabsf(bz)));
    const float s = fmaf(M, BVR_POS_REL, BVR_POS_ABS);
    ax -= s; ay -= s; az -= s; bx += s; by += s; bz += s;
    float near = -INFINITY, far = INFINITY;
    bool out = bvr_axis(ax, bx, q.ix, q.px, near, far);
    out = bvr_axis(ay, by, q.iy, q.py, near, far) || out;
    out = bvr_axis(az, bz, q.iz, q.pz, near, far) || out;
    out = out || near > far || far < tmin || near > hi;
    return q.tame && M < INFINITY && out;
}

// the children of a node that the lane has to enter: bit c for child c; nbox counts the box tests made
__device__ __forceinline__ unsigned bvr_children(const BvhNode &n, const BvrRay &q, float tmin, float hi, unsigned &nbox) {
    unsigned m = 0;
#pragma unroll
    for (int c = 0; c < BVH_W; ++c) {
        const float lox = bvh_comp(n.lox, c), hix = bvh_comp(n.hix, c);
        const bool there = bvh_child_exists(lox, hix);
        const bool skip = bvr_cannot_hit(lox, bvh_comp(n.loy, c), bvh_comp(n.loz, c), hix, bvh_comp(n.hiy, c), bvh_comp(n.hiz, c), q, tmin, hi);
        nbox += there ? 1u : 0u;
        m |= (there && !skip) ? (1u << c) : 0u;
    }
    return m;
}

// rays [R, 6]; results pk / pc [R] (one split).  visits: null, or two counters (box tests, pair tests)
template <bool COUNT>
__global__ __launch_bounds__(256) void bvr_trace_kernel(const float4 *__restrict__ rec, int F, const float4 *__restrict__ boxes,
                                                        const int4 *__restrict__ leaf_tri, const int *__restrict__ level_off, int top,
                                                        const float *__restrict__ rays, int R, float tmin, float tmax,
                                                        unsigned long long *__restrict__ pk, int *__restrict__ pc,
                                                        unsigned long long *__restrict__ visits) {
    __shared__ int off[BVH_MAX_LEVELS];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < BVH_MAX_LEVELS) off[tid] = level_off[tid];
    __syncthreads();
    const int n = blockIdx.x * RC_CHUNK + tid;
    const long nr = n < R ? n : R - 1;
    const float ox = rays[nr * 6], oy = rays[nr * 6 + 1], oz = rays[nr * 6 + 2];
    const float dx = rays[nr * 6 + 3], dy = rays[nr * 6 + 4], dz = rays[nr * 6 + 5];
    const RcRay r = rc_ray(ox, oy, oz, dx, dy, dz);
    const bool live = n < R && r.ok;
    const BvrRay q = bvr_setup(ox, oy, oz, dx, dy, dz);
    unsigned long long key = RC_MISS;
    int hits = 0;
    float hi = tmax;
    unsigned nbox = 0, npair = 0;
    int level = top;
    unsigned node = 0, child = 0;
    unsigned long long mask = 0;
    if (live) mask = bvh_mask_bits(top, bvr_children(bvh_load(boxes, off[top], 0), q, tmin, hi, nbox));
#pragma unroll 1
    while (bvh_next(top, level, node, mask, child)) {
        if (level > 0) {
            bvh_enter(level, node, child);
            mask |= bvh_mask_bits(level, bvr_children(bvh_load(boxes, off[level], node), q, tmin, hi, nbox));
            continue;
        }
        const int4 ids = leaf_tri[child];
#pragma unroll
        for (int i = 0; i < BVH_L; ++i) {
            const int f = bvh_comp(ids, i);
            if ((unsigned)f >= (unsigned)F) continue;              // -1: the last leaf has fewer than L triangles
            float t = 0.f;
            double V, W, det;
            const bool hit = rc_pair(r, rec[(long)f * RC_REC4], rec[(long)f * RC_REC4 + 1], rec[(long)f * RC_REC4 + 2], tmin, tmax, t, V, W, det);
            npair += 1;
            if constexpr (COUNT) {
                hits += hit ? 1 : 0;
            } else {
                const unsigned long long k = ((unsigned long long)rc_float_bits(t) << 32) | (unsigned)f;
                key = hit && k < key ? k : key;
            }
        }
        if constexpr (!COUNT) hi = key == RC_MISS ? tmax : rc_bits_float((unsigned)(key >> 32));
    }
    if (n < R) {
        if constexpr (COUNT) pc[n] = hits;
        else pk[n] = key;
    }
    if (visits) bvh_count_visits(visits, nbox, npair, lane);
}

// the minimum key of ray n over the S splits, then the pair test once more on the winner
__global__ __launch_bounds__(256) void rc_finish_cast_kernel(const float4 *__restrict__ rec, int F, const float *__restrict__ rays, int R,
                                                             const unsigned long long *__restrict__ pk, int S, float tmin, float tmax,
                                                             float *__restrict__ t_out, int *__restrict__ tri, float *__restrict__ uv,
                                                             float *__restrict__ normal) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= R) return;
    unsigned long long key = RC_MISS;
    for (int s = 0; s < S; ++s) key = min(key, pk[(long)s * R + n]);
    const unsigned f = (unsigned)(key & 0xFFFFFFFFull);
    const bool got = key != RC_MISS && f < (unsigned)F;
    float u = 0.f, v = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    if (got && (uv || normal)) {
        const float4 a = rec[(long)f * RC_REC4], b = rec[(long)f * RC_REC4 + 1], c = rec[(long)f * RC_REC4 + 2];
        const RcRay r = rc_ray(rays[(long)n * 6], rays[(long)n * 6 + 1], rays[(long)n * 6 + 2], rays[(long)n * 6 + 3],
                               rays[(long)n * 6 + 4], rays[(long)n * 6 + 5]);
        float t;
        double V, W, det;
        (void)rc_pair(r, a, b, c, tmin, tmax, t, V, W, det);
        u = (float)(V / det);
        v = (float)(W / det);
        const double e1x = (double)b.x - (double)a.x, e1y = (double)b.y - (double)a.y, e1z = (double)b.z - (double)a.z;
        const double e2x = (double)c.x - (double)a.x, e2y = (double)c.y - (double)a.y, e2z = (double)c.z - (double)a.z;
        const double mx = e1y * e2z - e1z * e2y, my = e1z * e2x - e1x * e2z, mz = e1x * e2y - e1y * e2x;
        const double nn = (mx * mx + my * my) + mz * mz;
        if (nn > 0.0 && nn - nn == 0.0) {
            const double len = __builtin_sqrt(nn);
            nx = (float)(mx / len); ny = (float)(my / len); nz = (float)(mz / len);
        }
    }
    if (t_out) t_out[n] = got ? rc_bits_float((unsigned)(key >> 32)) : INFINITY;
    if (tri) tri[n] = got ? (int)f : -1;
    if (uv) { uv[(long)n * 2] = u; uv[(long)n * 2 + 1] = v; }
    if (normal) { normal[(long)n * 3] = nx; normal[(long)n * 3 + 1] = ny; normal[(long)n * 3 + 2] = nz; }
}

__global__ __launch_bounds__(256) void rc_finish_count_kernel(const int *__restrict__ pc, int S, int R, int *__restrict__ count) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= R) return;
    int total = 0;
    for (int s = 0; s < S; ++s) total += pc[(long)s * R + n];
    count[n] = total;
}

}  // namespace surfd

#ifndef SURFD_RAYCAST_HOST_TEST
using namespace surfd;

struct surfd_rayscene {
    int F = 0, ntile = 0, nchunk = 0;
    float4 *rec = nullptr;            // [F] triangles of 3 float4
    float4 *tile_sph = nullptr;       // [ntile]
    float4 *chunk_sph = nullptr;      // [nchunk]
    unsigned long long *skipped = nullptr;   // (wave, tile) visits the last call with SURFD_RAY_COUNT_SKIPPED skipped
    long long last_total = 0;         // and how many visits that call had in all
    DeviceArena ws;                   // partial results
    MeshBvh bvh;                      // the hierarchy of surfd_rayscene_build_bvh (meshbvh.hip)
};

static int rc_check(const char *who, const surfd_rayscene *m, const float *rays, int R, float tmin, float tmax, int flags) {
    if (R < 0) SURFD_FAIL(SURFD_ERR_ARG, "%s: R = %d is negative", who, R);
    if (flags & ~(SURFD_RAY_BRUTE_FORCE | SURFD_RAY_COUNT_SKIPPED | SURFD_RAY_BVH | SURFD_RAY_COUNT_VISITS))
        SURFD_FAIL(SURFD_ERR_ARG, "%s: unknown flags 0x%x", who, flags);
    if ((flags & SURFD_RAY_BVH) && !(flags & SURFD_RAY_BRUTE_FORCE) && !(m && m->bvh.built))
        SURFD_FAIL(m ? SURFD_ERR_STATE : SURFD_ERR_ARG, "%s: flags 0x%x ask for the hierarchy, which was not built (surfd_rayscene_build_bvh)",
                   who, flags);
    if (!(tmin >= 0.f) || !(tmin < INFINITY)) SURFD_FAIL(SURFD_ERR_ARG, "%s: tmin = %g must be finite and not negative", who, (double)tmin);
    if (tmax != tmax) SURFD_FAIL(SURFD_ERR_ARG, "%s: tmax is a NaN", who);
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "%s: null handle", who);
    if (R > 0 && !rays) SURFD_FAIL(SURFD_ERR_ARG, "%s: null rays", who);
    if (R > (1 << 28)) SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "%s: R = %d is beyond the supported size", who, R);
    return SURFD_OK;
}

template <bool COUNT>
static int rc_trace(surfd_rayscene *m, const float *rays, int R, float tmin, float tmax, int flags, unsigned long long **pk, int **pc,
                    int *S_out, hipStream_t st) {
    int rc;
    const bool brute = flags & SURFD_RAY_BRUTE_FORCE;
    const bool tree = (flags & SURFD_RAY_BVH) && !brute;      // the brute-force flag wins
    const Split sp = split_units(R, RC_CHUNK, m->nchunk, RC_MAX_SPLITS);      // splits of the chunk range per block of rays
    const int S = tree ? 1 : sp.S, span = sp.span;
    const size_t np = (size_t)S * R;
    if ((rc = m->ws.reserve(np * sizeof(unsigned long long), st))) return rc;
    *pk = (unsigned long long *)m->ws.ptr;
    *pc = (int *)m->ws.ptr;
    *S_out = S;
    if (m->bvh.built && (flags & SURFD_RAY_COUNT_VISITS) && (rc = bvh_visits_reset(&m->bvh, st))) return rc;
    if (tree) {
        if (flags & SURFD_RAY_COUNT_SKIPPED) {
            HIP_TRY(hipMemsetAsync(m->skipped, 0, sizeof(unsigned long long), st));
            m->last_total = 0;                                // no tiles on this path
        }
        hipLaunchKernelGGL((bvr_trace_kernel<COUNT>), dim3((unsigned)ceil_div(R, RC_CHUNK)), dim3(256), 0, st, (const float4 *)m->rec, m->F,
                           (const float4 *)m->bvh.boxes, (const int4 *)m->bvh.leaf_tri, (const int *)m->bvh.level_off, m->bvh.lay.levels - 1,
                           rays, R, tmin, tmax, *pk, *pc, (flags & SURFD_RAY_COUNT_VISITS) ? m->bvh.visits : nullptr);
        LAUNCH_CHECK();
        return SURFD_OK;
    }
    unsigned long long *skipped = nullptr;
    if (flags & SURFD_RAY_COUNT_SKIPPED) {
        HIP_TRY(hipMemsetAsync(m->skipped, 0, sizeof(unsigned long long), st));
        m->last_total = (long long)ceil_div(R, 64) * m->ntile;
        skipped = brute ? nullptr : m->skipped;
    }
    const dim3 grid((unsigned)ceil_div(R, RC_CHUNK), (unsigned)S);
    if (brute)
        hipLaunchKernelGGL((rc_trace_kernel<false, COUNT>), grid, dim3(256), 0, st, (const float4 *)m->rec, m->F, (const float4 *)m->tile_sph,
                           (const float4 *)m->chunk_sph, m->nchunk, span, rays, R, tmin, tmax, *pk, *pc, skipped);
    else
        hipLaunchKernelGGL((rc_trace_kernel<true, COUNT>), grid, dim3(256), 0, st, (const float4 *)m->rec, m->F, (const float4 *)m->tile_sph,
                           (const float4 *)m->chunk_sph, m->nchunk, span, rays, R, tmin, tmax, *pk, *pc, skipped);
    LAUNCH_CHECK();
    return SURFD_OK;
}

extern "C" {

int surfd_rayscene_create(const float *vertices, int V, const int32_t *triangles, int F, surfd_stream s, surfd_rayscene **out) {
    int rc = mesh_create_args("surfd_rayscene_create", vertices, V, triangles, F, out, 1 << 28);
    if (rc != SURFD_OK) return rc;
    hipStream_t st = as_stream(s);
    surfd_rayscene *m = new surfd_rayscene();
    m->F = F;
    m->ntile = ceil_div(F, RC_TILE);
    m->nchunk = ceil_div(F, RC_CHUNK);
    CreateFlags bad(1);
    int flag = 0;
    auto run = [&]() -> int {
        HIP_TRY(hipMalloc(&m->rec, (size_t)F * RC_REC4 * sizeof(float4)));
        HIP_TRY(hipMalloc(&m->tile_sph, (size_t)m->ntile * sizeof(float4)));
        HIP_TRY(hipMalloc(&m->chunk_sph, (size_t)m->nchunk * sizeof(float4)));
        HIP_TRY(hipMalloc(&m->skipped, sizeof(unsigned long long)));
        if (int e = bad.init(st)) return e;
        HIP_TRY(hipMemsetAsync(m->skipped, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(rc_gather_kernel, dim3((unsigned)ceil_div(F, 256)), dim3(256), 0, st, vertices, V, triangles, F, m->rec, bad.dev);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(rc_bounds_kernel, dim3((unsigned)ceil_div(m->ntile, 64)), dim3(64), 0, st, (const float4 *)m->rec, F, RC_TILE,
                           m->ntile, m->tile_sph);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(rc_bounds_kernel, dim3((unsigned)ceil_div(m->nchunk, 64)), dim3(64), 0, st, (const float4 *)m->rec, F, RC_CHUNK,
                           m->nchunk, m->chunk_sph);
        LAUNCH_CHECK();
        return bad.read(&flag, st);
    };
    rc = run();
    if (rc == SURFD_OK && flag) rc = mesh_bad_index("surfd_rayscene_create", V);
    if (rc != SURFD_OK) { surfd_rayscene_destroy(m); return rc; }
    *out = m;
    return SURFD_OK;
}

void surfd_rayscene_destroy(surfd_rayscene *m) {
    if (!m) return;
    (void)hipFree(m->rec); (void)hipFree(m->tile_sph); (void)hipFree(m->chunk_sph); (void)hipFree(m->skipped);
    m->ws.release();
    bvh_free(&m->bvh);
    delete m;
}

int surfd_rayscene_num_triangles(const surfd_rayscene *m) { return m ? m->F : 0; }

int surfd_rayscene_cast(surfd_rayscene *m, const float *rays, int R, float tmin, float tmax, int flags, float *t, int32_t *tri, float *uv,
                        float *normal, surfd_stream s) {
    int rc = rc_check("surfd_rayscene_cast", m, rays, R, tmin, tmax, flags);
    if (rc != SURFD_OK || R == 0) return rc;
    hipStream_t st = as_stream(s);
    unsigned long long *pk;
    int *pc, S;
    if ((rc = rc_trace<false>(m, rays, R, tmin, tmax, flags, &pk, &pc, &S, st))) return rc;
    if (t || tri || uv || normal) {
        hipLaunchKernelGGL(rc_finish_cast_kernel, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, st, (const float4 *)m->rec, m->F, rays, R,
                           (const unsigned long long *)pk, S, tmin, tmax, t, tri, uv, normal);
        LAUNCH_CHECK();
    }
    return SURFD_OK;
}

int surfd_rayscene_count(surfd_rayscene *m, const float *rays, int R, float tmin, float tmax, int flags, int32_t *count, surfd_stream s) {
    int rc = rc_check("surfd_rayscene_count", m, rays, R, tmin, tmax, flags);
    if (rc != SURFD_OK || R == 0) return rc;
    if (!count) SURFD_FAIL(SURFD_ERR_ARG, "surfd_rayscene_count: null count");
    hipStream_t st = as_stream(s);
    unsigned long long *pk;
    int *pc, S;
    if ((rc = rc_trace<true>(m, rays, R, tmin, tmax, flags, &pk, &pc, &S, st))) return rc;
    hipLaunchKernelGGL(rc_finish_count_kernel, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, st, (const int *)pc, S, R, count);
    LAUNCH_CHECK();
    return SURFD_OK;
}

int surfd_rayscene_skipped(surfd_rayscene *m, int64_t *skipped, int64_t *total, surfd_stream s) {
    if (!m || !skipped || !total) SURFD_FAIL(SURFD_ERR_ARG, "surfd_rayscene_skipped: null argument");
    return read_counter(m->skipped, m->last_total, skipped, total, as_stream(s));
}

int surfd_rayscene_build_bvh(surfd_rayscene *m, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_rayscene_build_bvh: null handle");
    return bvh_build(&m->bvh, (const float4 *)m->rec, RC_REC4, false, m->F, as_stream(s));
}

int surfd_rayscene_visits(surfd_rayscene *m, int64_t *box_tests, int64_t *pair_tests, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_rayscene_visits: null handle");
    return bvh_visits_read("surfd_rayscene_visits", &m->bvh, box_tests, pair_tests, as_stream(s));
}

int surfd_rayscene_bvh_info(const surfd_rayscene *m, int *levels, int *leaves, int *nodes, int32_t *level_sizes, int capacity) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_rayscene_bvh_info: null handle");
    return bvh_info("surfd_rayscene_bvh_info", &m->bvh, levels, leaves, nodes, level_sizes, capacity);
}

int surfd_rayscene_bvh_read(const surfd_rayscene *m, float *boxes, int32_t *leaf_triangles, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_rayscene_bvh_read: null handle");
    return bvh_read("surfd_rayscene_bvh_read", &m->bvh, boxes, leaf_triangles, as_stream(s));
}

}  // extern "C"
#endif  // SURFD_RAYCAST_HOST_TEST
