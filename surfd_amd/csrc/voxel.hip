// Occupancy grids of meshes and clouds, and volumetric IoU between them.  No reference counterpart (the reference ships no
// evaluation code); stands for the voxel grids and the intersection-over-union of the single-view reconstruction protocol.
// One fp32 step (the snap), everything after it int64 and exact: a grid has the same bits for any face order, winding, batch,
// path or launch geometry.  VALU only.  DESIGN.md section 8.5.
//
//   vx_surface_small_kernel — one lane per triangle: snap and set-up; a triangle whose clipped voxel box holds at most
//                             VX_SMALL_MAX voxels is voxelised by that lane, a larger one is appended to a list.
//   vx_surface_large_kernel — walks the list one triangle per wave, the 64 lanes striding over the box.
//   vx_solid_small_kernel / vx_solid_large_kernel — the same split over the columns of the xy box: parity fill along +z.
//   vx_solid_merge_kernel   — one lane per column: ORs the fill into the caller's grid and counts the odd columns.
//   vx_points_kernel        — one lane per point.
//   vx_iou_kernel           — popcounts of a AND b, a OR b for pairs of grids; vx_iou_finish_kernel divides.
//
// Grid: the cube [lo, hi]^3 cut into R^3 voxels, 1 <= R <= 512; voxel (i, j, k) is the CLOSED box [i, i+1] x [j, j+1] x [k, k+1]
// in voxel units, axis order (x, y, z) = (i, j, k).  Bit-packed along z: bits[R, R, W] uint32, W = ceil(R / 32), bit k & 31 of
// word k >> 5 of column (i, j) is voxel k; padding bits are never set.
//
// Arithmetic:
//   snap      q = rint(__fmul_rn(__fsub_rn(x, lo), s)) to int32 (nearest even), s = fp32(256 R / (hi - lo)) formed on the host
//             in fp64: units of 1/256 voxel.  A vertex is invalid when it is NaN or |q| > 2^19; a triangle with an invalid vertex
//             or with an index outside [0, V) is DROPPED and counted, never a fault.
//   surface   n = (q1 - q0) x (q2 - q0) in int64 (edge components <= 2^20, n components <= 2^41); n = 0: skipped and counted as
//             degenerate.  vx_hit(), the one place a (triangle, voxel) pair is decided: the separating-axis test of
//             Akenine-Moller on v_i = q_i - c, c = 256 idx + 128, half-size 128 (|v| < 2^20):
//               3 box axes     min(v.a) > 128 or max(v.a) < -128
//               normal         |n . v0| > 128 (|nx| + |ny| + |nz|)              (|n . v0| <= 3 * 2^61 < 2^63)
//               9 edge x axis  for edge e from u to u', opposite vertex w:  p = (axis x e) . v at u and at w (u' gives u's value),
//                              r = 128 (|e.b| + |e.c|); min(p) > r or max(p) < -r    (|p| < 2^41)
//             an axis separates on STRICT inequality only: touching counts.  Traversal: the triangle's voxel box
//             [(min - 1) >> 8, max >> 8] clipped to the grid.
//   solid     for every column (i, j) whose centre (256 i + 128, 256 j + 128) the xy projection covers — the raster's integer
//             edge functions and top-left rule after the winding swap, so a crossing on a shared edge or through a vertex counts
//             once — the first k with S < (256 k + 128) A2, S = E0 z0 + E1 z1 + E2 z2 (post-swap order), A2 the doubled projected
//             area > 0; found by bisection over [0, R] with that comparison, no division (|S| <= 2^59, the right side < 2^58:
//             DESIGN.md section 8.5 holds the proof of every bound quoted here).
//             All bits >= k of the column are flipped (atomicXor on a fill buffer) and so is bit 0 of the column's crossing
//             parity.  A2 = 0: nothing.  odd_columns = columns with an odd crossing total: 0 for a closed snapped mesh.
//   points    the same snap, voxel = q >> 8 (floor), q = 256 R belongs to the last voxel; anything else outside [0, R) (or
//             invalid) is counted as outside.
//   iou       inter = popcount(a & b), uni = popcount(a | b) summed as int32 (R^3 <= 2^27); iou = __fdiv_rn(float(inter),
//             float(uni)), 1.0 when uni = 0.
//
// Hazards: the grid, the fill buffer, the parity buffer and the counters are the only memory two lanes may write, and they do so
// with 32-bit vector atomics only (atomicOr / atomicXor / atomicAdd: commutative, so the result is order-free).  The list of
// large triangles is filled through an atomicAdd slot; its order varies from run to run, the grid does not.  Kernels of one call
// run in stream order.  Every loop is bounded by a clipped box, the list length, W or 10 bisection steps; no kernel waits on
// another workgroup.
#include "common.h"
#include <cmath>
#include <climits>
#include <algorithm>

namespace surfd {

constexpr int VX_MAX_R = 512;
constexpr int VX_SNAP_MAX = 1 << 19;      // largest snapped coordinate in 1/256-voxel units
// SURFD_VOXEL_FORCE_SMALL / _FORCE_LARGE are TEST switches: under FORCE_SMALL one lane walks its triangle's whole clipped box, which
// for a grid-spanning triangle at R = 512 is 2^27 voxels; the default split never gives a lane more than VX_SMALL_MAX.
constexpr int VX_SMALL_MAX = 32;          // voxels in a clipped box up to which the set-up lane voxelises it itself
constexpr int VX_SOLID_SMALL_MAX = 16;    // column centres in a clipped xy box up to which the set-up lane fills them itself
constexpr int VX_LARGE_WGS = 1024;        // workgroups of 4 waves that walk the list of large triangles
constexpr int VX_HDR = 16;                // workspace header in 32-bit words: list length, dropped, degenerate, odd columns
constexpr int VX_IOU_CHUNK = 256 * 16;    // words of a grid per workgroup of vx_iou_kernel

struct VxGrid { float lo, s; int R, W; };

struct VxTri {                            // a snapped triangle
    int x0, y0, z0, x1, y1, z1, x2, y2, z2;
    int i0, i1, j0, j1, k0, k1;           // clipped box (inclusive); surface: voxels, solid: column centres (k unused)
};

__device__ __forceinline__ bool vx_snap(float x, const VxGrid &g, int &q) {
    const float r = rintf(__fmul_rn(__fsub_rn(x, g.lo), g.s));
    if (!(fabsf(r) <= (float)VX_SNAP_MAX)) return false;       // NaN, Inf or out of range
    q = (int)r;
    return true;
}

// loads and snaps triangle f; false = dropped (invalid vertex or an index outside [0, V))
__device__ __forceinline__ bool vx_load(const float *__restrict__ vertices, int V, const int *__restrict__ faces, int f, const VxGrid &g, VxTri &t) {
    const int a = faces[(size_t)f * 3], b = faces[(size_t)f * 3 + 1], c = faces[(size_t)f * 3 + 2];
    if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) return false;
    bool ok = vx_snap(vertices[(size_t)a * 3], g, t.x0) & vx_snap(vertices[(size_t)a * 3 + 1], g, t.y0) & vx_snap(vertices[(size_t)a * 3 + 2], g, t.z0);
    ok &= vx_snap(vertices[(size_t)b * 3], g, t.x1) & vx_snap(vertices[(size_t)b * 3 + 1], g, t.y1) & vx_snap(vertices[(size_t)b * 3 + 2], g, t.z1);
    ok &= vx_snap(vertices[(size_t)c * 3], g, t.x2) & vx_snap(vertices[(size_t)c * 3 + 1], g, t.y2) & vx_snap(vertices[(size_t)c * 3 + 2], g, t.z2);
    return ok;
}

__device__ __forceinline__ int vx_min3(int a, int b, int c) { return min(a, min(b, c)); }
__device__ __forceinline__ int vx_max3(int a, int b, int c) { return max(a, max(b, c)); }
__device__ __forceinline__ long long vx_abs(long long a) { return a < 0 ? -a : a; }

struct VxNormal { long long x, y, z; };

__device__ __forceinline__ VxNormal vx_normal(const VxTri &t) {
    const long long ax = t.x1 - t.x0, ay = t.y1 - t.y0, az = t.z1 - t.z0, bx = t.x2 - t.x0, by = t.y2 - t.y0, bz = t.z2 - t.z0;
    return {ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx};
}

// the voxels a triangle's bounding box touches (closed voxels: a coordinate on a voxel face belongs to both), clipped to the grid
__device__ __forceinline__ bool vx_voxel_box(VxTri &t, int R) {
    t.i0 = max(0, (vx_min3(t.x0, t.x1, t.x2) - 1) >> 8); t.i1 = min(R - 1, vx_max3(t.x0, t.x1, t.x2) >> 8);
    t.j0 = max(0, (vx_min3(t.y0, t.y1, t.y2) - 1) >> 8); t.j1 = min(R - 1, vx_max3(t.y0, t.y1, t.y2) >> 8);
    t.k0 = max(0, (vx_min3(t.z0, t.z1, t.z2) - 1) >> 8); t.k1 = min(R - 1, vx_max3(t.z0, t.z1, t.z2) >> 8);
    return t.i0 <= t.i1 && t.j0 <= t.j1 && t.k0 <= t.k1;
}

// true when the axis (b, c components ex, ey of an edge crossed with a box axis) separates: p at a vertex of the edge and at the
// opposite vertex, radius 128 (|eb| + |ec|)
__device__ __forceinline__ bool vx_edge_axis(int eb, int ec, int ub, int uc, int wb, int wc) {
    const long long pu = (long long)eb * uc - (long long)ec * ub, pw = (long long)eb * wc - (long long)ec * wb;
    const long long r = 128LL * (abs(eb) + abs(ec));
    return min(pu, pw) > r || max(pu, pw) < -r;
}

// the three axes of one edge e = (ex, ey, ez) from u (a vertex of the edge) with opposite vertex w, all relative to the centre
__device__ __forceinline__ bool vx_edge(int ex, int ey, int ez, int ux, int uy, int uz, int wx, int wy, int wz) {
    return vx_edge_axis(ey, ez, uy, uz, wy, wz)       // x axis: p = ey vz - ez vy
        || vx_edge_axis(ez, ex, uz, ux, wz, wx)       // y axis: p = ez vx - ex vz
        || vx_edge_axis(ex, ey, ux, uy, wx, wy);      // z axis: p = ex vy - ey vx
}

// the one place a (triangle, voxel) pair is decided
__device__ __forceinline__ bool vx_hit(const VxTri &t, const VxNormal &n, int i, int j, int k) {
    const int cx = 256 * i + 128, cy = 256 * j + 128, cz = 256 * k + 128;
    const int ax = t.x0 - cx, ay = t.y0 - cy, az = t.z0 - cz;
    const int bx = t.x1 - cx, by = t.y1 - cy, bz = t.z1 - cz;
    const int gx = t.x2 - cx, gy = t.y2 - cy, gz = t.z2 - cz;
    if (vx_min3(ax, bx, gx) > 128 || vx_max3(ax, bx, gx) < -128) return false;
    if (vx_min3(ay, by, gy) > 128 || vx_max3(ay, by, gy) < -128) return false;
    if (vx_min3(az, bz, gz) > 128 || vx_max3(az, bz, gz) < -128) return false;
    const long long d = n.x * ax + n.y * ay + n.z * az;
    const long long r = 128LL * (vx_abs(n.x) + vx_abs(n.y) + vx_abs(n.z));
    if (d > r || d < -r) return false;
    if (vx_edge(bx - ax, by - ay, bz - az, ax, ay, az, gx, gy, gz)) return false;
    if (vx_edge(gx - bx, gy - by, gz - bz, bx, by, bz, ax, ay, az)) return false;
    if (vx_edge(ax - gx, ay - gy, az - gz, gx, gy, gz, bx, by, bz)) return false;
    return true;
}

// the voxels k0 .. k1 of word w of column (i, j): one atomicOr for the whole word
__device__ __forceinline__ void vx_surface_word(const VxTri &t, const VxNormal &n, int i, int j, int w, const VxGrid &g, unsigned *__restrict__ bits) {
    const int ka = max(t.k0, w * 32), kb = min(t.k1, w * 32 + 31);
    unsigned m = 0;
    for (int k = ka; k <= kb; ++k)
        if (vx_hit(t, n, i, j, k)) m |= 1u << (k & 31);
    if (m) atomicOr(bits + ((size_t)i * g.R + j) * g.W + w, m);
}

// counters: hdr[0] list length, hdr[1] dropped, hdr[2] degenerate
__global__ __launch_bounds__(256) void vx_surface_small_kernel(const float *__restrict__ vertices, int V, const int *__restrict__ faces, int F, VxGrid g,
                                                               int flags, unsigned *__restrict__ bits, unsigned *__restrict__ hdr,
                                                               unsigned *__restrict__ list) {
    const long long fl = (long long)blockIdx.x * 256 + threadIdx.x;
    if (fl >= F) return;
    const int f = (int)fl;
    VxTri t;
    if (!vx_load(vertices, V, faces, f, g, t)) { atomicAdd(hdr + 1, 1u); return; }
    const VxNormal n = vx_normal(t);
    if (n.x == 0 && n.y == 0 && n.z == 0) { atomicAdd(hdr + 2, 1u); return; }
    if (!vx_voxel_box(t, g.R)) return;
    const int count = (t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1) * (t.k1 - t.k0 + 1);          // at most 512^3 = 2^27
    const bool large = (flags & SURFD_VOXEL_FORCE_LARGE) || (count > VX_SMALL_MAX && !(flags & SURFD_VOXEL_FORCE_SMALL));
    if (large) {
        list[atomicAdd(hdr, 1u)] = (unsigned)f;               // slot below F, the capacity of the list
        return;
    }
    for (int i = t.i0; i <= t.i1; ++i)
        for (int j = t.j0; j <= t.j1; ++j)
            for (int w = t.k0 >> 5; w <= t.k1 >> 5; ++w) vx_surface_word(t, n, i, j, w, g, bits);
}

// VX_LARGE_WGS workgroups of 4 waves; wave w takes the list entries w, w + waves, ...; a lane takes (column, word) units of the box
__global__ __launch_bounds__(256) void vx_surface_large_kernel(const float *__restrict__ vertices, int V, const int *__restrict__ faces, VxGrid g,
                                                               unsigned *__restrict__ bits, const unsigned *__restrict__ hdr,
                                                               const unsigned *__restrict__ list, unsigned capacity) {
    const unsigned n_list = min(hdr[0], capacity);
    const unsigned waves = gridDim.x * 4, lane = threadIdx.x & 63;
    for (unsigned e = blockIdx.x * 4 + (threadIdx.x >> 6); e < n_list; e += waves) {
        const int f = (int)list[e];
        VxTri t;
        if (!vx_load(vertices, V, faces, f, g, t)) continue;            // cannot happen: it was valid at set-up
        const VxNormal n = vx_normal(t);
        if (!vx_voxel_box(t, g.R)) continue;
        const int w0 = t.k0 >> 5, nw = (t.k1 >> 5) - w0 + 1, bj = t.j1 - t.j0 + 1;
        const int total = (t.i1 - t.i0 + 1) * bj * nw;                  // at most 512 * 512 * 16 = 2^22
        for (int p = lane; p < total; p += 64) {
            const int w = p % nw, c = p / nw;
            vx_surface_word(t, n, t.i0 + c / bj, t.j0 + c % bj, w0 + w, g, bits);
        }
    }
}

// ---- solid ------------------------------------------------------------------------------------------------------------------------
struct VxCol {                            // the xy projection of a triangle, post-swap order, with the z of its vertices
    int ax, ay, az, bx, by, bz, cx, cy, cz;
    long long a2;                         // doubled projected area, > 0
    bool tl0, tl1, tl2;                   // edge (b,c), (c,a), (a,b) is a top or a left edge
};

__device__ __forceinline__ long long vx_edge_fn(int px, int py, int qx, int qy, int sx, int sy) {
    return (long long)(qx - px) * (sy - py) - (long long)(qy - py) * (sx - px);
}

__device__ __forceinline__ bool vx_top_left(int px, int py, int qx, int qy) {
    const int dx = qx - px, dy = qy - py;
    return (dy == 0 && dx > 0) || dy < 0;
}

// false = nothing to fill (zero projected area or no column centre in the box)
__device__ __forceinline__ bool vx_column_setup(VxTri &t, int R, VxCol &c) {
    const long long a2 = (long long)(t.x1 - t.x0) * (t.y2 - t.y0) - (long long)(t.y1 - t.y0) * (t.x2 - t.x0);
    if (a2 == 0) return false;
    const bool swapped = a2 < 0;
    c.a2 = swapped ? -a2 : a2;
    c.ax = t.x0; c.ay = t.y0; c.az = t.z0;
    c.bx = swapped ? t.x2 : t.x1; c.by = swapped ? t.y2 : t.y1; c.bz = swapped ? t.z2 : t.z1;
    c.cx = swapped ? t.x1 : t.x2; c.cy = swapped ? t.y1 : t.y2; c.cz = swapped ? t.z1 : t.z2;
    c.tl0 = vx_top_left(c.bx, c.by, c.cx, c.cy);
    c.tl1 = vx_top_left(c.cx, c.cy, c.ax, c.ay);
    c.tl2 = vx_top_left(c.ax, c.ay, c.bx, c.by);
    // column centres 256 i + 128 inside [min, max]
    t.i0 = max(0, (vx_min3(t.x0, t.x1, t.x2) - 128 + 255) >> 8); t.i1 = min(R - 1, (vx_max3(t.x0, t.x1, t.x2) - 128) >> 8);
    t.j0 = max(0, (vx_min3(t.y0, t.y1, t.y2) - 128 + 255) >> 8); t.j1 = min(R - 1, (vx_max3(t.y0, t.y1, t.y2) - 128) >> 8);
    return t.i0 <= t.i1 && t.j0 <= t.j1;
}

// the one place a (triangle, column) pair is decided and applied
__device__ __forceinline__ void vx_column(const VxCol &c, int i, int j, const VxGrid &g, unsigned *__restrict__ fill, unsigned *__restrict__ parity) {
    const int sx = 256 * i + 128, sy = 256 * j + 128;
    const long long e0 = vx_edge_fn(c.bx, c.by, c.cx, c.cy, sx, sy);
    const long long e1 = vx_edge_fn(c.cx, c.cy, c.ax, c.ay, sx, sy);
    const long long e2 = vx_edge_fn(c.ax, c.ay, c.bx, c.by, sx, sy);
    if (!((e0 > 0 || (e0 == 0 && c.tl0)) && (e1 > 0 || (e1 == 0 && c.tl1)) && (e2 > 0 || (e2 == 0 && c.tl2)))) return;
    const long long S = e0 * c.az + e1 * c.bz + e2 * c.cz;
    int lo = 0, hi = g.R;                                       // the first k in [0, R] with S < (256 k + 128) a2; R = none
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (S < (256LL * mid + 128) * c.a2) hi = mid; else lo = mid + 1;
    }
    const size_t col = (size_t)i * g.R + j;
    atomicXor(parity + col, 1u);
    const unsigned last = (g.R & 31) ? (1u << (g.R & 31)) - 1u : ~0u;          // the valid bits of word W - 1
    for (int w = lo >> 5; w < g.W; ++w) {                       // lo = R with R a multiple of 32 gives w = W: nothing
        unsigned m = w == (lo >> 5) ? ~0u << (lo & 31) : ~0u;
        if (w == g.W - 1) m &= last;
        if (m) atomicXor(fill + col * g.W + w, m);
    }
}

// counters: hdr[0] list length, hdr[1] dropped
__global__ __launch_bounds__(256) void vx_solid_small_kernel(const float *__restrict__ vertices, int V, const int *__restrict__ faces, int F, VxGrid g,
                                                             int flags, unsigned *__restrict__ fill, unsigned *__restrict__ parity,
                                                             unsigned *__restrict__ hdr, unsigned *__restrict__ list) {
    const long long fl = (long long)blockIdx.x * 256 + threadIdx.x;
    if (fl >= F) return;
    const int f = (int)fl;
    VxTri t;
    if (!vx_load(vertices, V, faces, f, g, t)) { atomicAdd(hdr + 1, 1u); return; }
    VxCol c;
    if (!vx_column_setup(t, g.R, c)) return;
    const int count = (t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1);
    const bool large = (flags & SURFD_VOXEL_FORCE_LARGE) || (count > VX_SOLID_SMALL_MAX && !(flags & SURFD_VOXEL_FORCE_SMALL));
    if (large) {
        list[atomicAdd(hdr, 1u)] = (unsigned)f;
        return;
    }
    for (int i = t.i0; i <= t.i1; ++i)
        for (int j = t.j0; j <= t.j1; ++j) vx_column(c, i, j, g, fill, parity);
}

__global__ __launch_bounds__(256) void vx_solid_large_kernel(const float *__restrict__ vertices, int V, const int *__restrict__ faces, VxGrid g,
                                                             unsigned *__restrict__ fill, unsigned *__restrict__ parity,
                                                             const unsigned *__restrict__ hdr, const unsigned *__restrict__ list, unsigned capacity) {
    const unsigned n_list = min(hdr[0], capacity);
    const unsigned waves = gridDim.x * 4, lane = threadIdx.x & 63;
    for (unsigned e = blockIdx.x * 4 + (threadIdx.x >> 6); e < n_list; e += waves) {
        const int f = (int)list[e];
        VxTri t;
        if (!vx_load(vertices, V, faces, f, g, t)) continue;            // cannot happen: it was valid at set-up
        VxCol c;
        if (!vx_column_setup(t, g.R, c)) continue;
        const int bj = t.j1 - t.j0 + 1, total = (t.i1 - t.i0 + 1) * bj;
        for (int p = lane; p < total; p += 64) vx_column(c, t.i0 + p / bj, t.j0 + p % bj, g, fill, parity);
    }
}

// one lane per column: bits |= fill; hdr[3] += columns with an odd crossing total (one atomicAdd per wave)
__global__ __launch_bounds__(256) void vx_solid_merge_kernel(const unsigned *__restrict__ fill, const unsigned *__restrict__ parity, VxGrid g,
                                                             unsigned *__restrict__ bits, unsigned *__restrict__ hdr) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    bool odd = false;
    if (col < g.R * g.R) {
        odd = (parity[col] & 1u) != 0;
        for (int w = 0; w < g.W; ++w) {
            const unsigned m = fill[(size_t)col * g.W + w];
            if (m) atomicOr(bits + (size_t)col * g.W + w, m);
        }
    }
    const unsigned long long b = __ballot(odd);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(hdr + 3, (unsigned)__popcll(b));
}

// ---- points -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vx_points_kernel(const float *__restrict__ points, int P, VxGrid g, unsigned *__restrict__ bits,
                                                        unsigned *__restrict__ outside) {
    const long long pl = (long long)blockIdx.x * 256 + threadIdx.x;
    bool out = false;
    if (pl < P) {
        int q[3], v[3];
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            ok &= vx_snap(points[(size_t)pl * 3 + a], g, q[a]);
            v[a] = ok ? (q[a] == 256 * g.R ? g.R - 1 : q[a] >> 8) : -1;             // a point on the upper grid face: the last voxel
            ok &= v[a] >= 0 && v[a] < g.R;
        }
        if (ok) atomicOr(bits + ((size_t)v[0] * g.R + v[1]) * g.W + (v[2] >> 5), 1u << (v[2] & 31));
        out = !ok;
    }
    const unsigned long long b = __ballot(out);
    if (outside && (threadIdx.x & 63) == 0 && b) atomicAdd(outside, (unsigned)__popcll(b));
}

// ---- iou --------------------------------------------------------------------------------------------------------------------------
// grid (pairs, chunks): pair p = (m, n) = (p / N, p % N), or (p, p) in the paired form; one atomicAdd pair per workgroup
__global__ __launch_bounds__(256) void vx_iou_kernel(const unsigned *__restrict__ a, const unsigned *__restrict__ b, int N, int paired, int words,
                                                     int *__restrict__ inter, int *__restrict__ uni) {
    __shared__ int part[2][4];
    const int pair = blockIdx.x;
    const unsigned *pa = a + (size_t)(paired ? pair : pair / N) * words, *pb = b + (size_t)(paired ? pair : pair % N) * words;     // pair < 2^31
    const int end = min(words, (int)(blockIdx.y + 1) * VX_IOU_CHUNK);
    int si = 0, su = 0;
    for (int w = blockIdx.y * VX_IOU_CHUNK + threadIdx.x; w < end; w += 256) {
        const unsigned x = pa[w], y = pb[w];
        si += __popc(x & y); su += __popc(x | y);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { si += __shfl_down(si, o); su += __shfl_down(su, o); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = si; part[1][threadIdx.x >> 6] = su; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int ti = part[0][0] + part[0][1] + part[0][2] + part[0][3], tu = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        if (ti) atomicAdd(inter + pair, ti);
        if (tu) atomicAdd(uni + pair, tu);
    }
}

__global__ __launch_bounds__(256) void vx_iou_finish_kernel(const int *__restrict__ inter, const int *__restrict__ uni, int pairs, float *__restrict__ iou) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < pairs) iou[p] = uni[p] == 0 ? 1.f : __fdiv_rn((float)inter[p], (float)uni[p]);
}

}  // namespace surfd

using namespace surfd;

// the checks every grid-taking entry shares; they touch no HIP call
static int vx_grid(const char *who, float lo, float hi, int R, VxGrid &g) {
    if (R < 1 || R > VX_MAX_R) SURFD_FAIL(SURFD_ERR_ARG, "%s: R = %d must lie in [1, %d]", who, R, VX_MAX_R);
    if (!(hi > lo) || !std::isfinite(lo) || !std::isfinite(hi)) SURFD_FAIL(SURFD_ERR_ARG, "%s: bounds lo = %g, hi = %g need finite lo < hi", who, (double)lo, (double)hi);
    const float s = (float)(256.0 * R / ((double)hi - (double)lo));
    if (!std::isfinite(s)) SURFD_FAIL(SURFD_ERR_ARG, "%s: bounds lo = %g, hi = %g are too close for R = %d", who, (double)lo, (double)hi, R);
    g.lo = lo; g.s = s; g.R = R; g.W = (R + 31) / 32;
    return SURFD_OK;
}

static int vx_mesh_args(const char *who, const float *vertices, int V, const int32_t *faces, int F, int flags, const void *ws, const void *bits) {
    if (V < 0 || F < 0) SURFD_FAIL(SURFD_ERR_ARG, "%s: V = %d, F = %d must not be negative", who, V, F);
    if ((long long)V * 3 >= (1LL << 31) || (long long)F * 3 >= (1LL << 31)) SURFD_FAIL(SURFD_ERR_ARG, "%s: 3 V and 3 F must stay below 2^31 (V = %d, F = %d)", who, V, F);
    if (flags & ~(SURFD_VOXEL_FORCE_SMALL | SURFD_VOXEL_FORCE_LARGE) ||
        (flags & (SURFD_VOXEL_FORCE_SMALL | SURFD_VOXEL_FORCE_LARGE)) == (SURFD_VOXEL_FORCE_SMALL | SURFD_VOXEL_FORCE_LARGE))
        SURFD_FAIL(SURFD_ERR_ARG, "%s: flags = %d (FORCE_SMALL and FORCE_LARGE exclude each other)", who, flags);
    if ((V > 0 && !vertices) || (F > 0 && !faces)) SURFD_FAIL(SURFD_ERR_ARG, "%s: null vertices or faces", who);
    if (!ws || !bits) SURFD_FAIL(SURFD_ERR_ARG, "%s: null workspace or bits", who);
    return SURFD_OK;
}

static int vx_surface_pass(const float *vertices, int V, const int32_t *faces, int F, const VxGrid &g, int flags, unsigned *hdr, uint32_t *bits, hipStream_t st) {
    unsigned *list = hdr + VX_HDR;
    HIP_TRY(hipMemsetAsync(hdr, 0, VX_HDR * sizeof(unsigned), st));
    if (F == 0) return SURFD_OK;
    hipLaunchKernelGGL(vx_surface_small_kernel, dim3((unsigned)ceil_div<long long>(F, 256)), dim3(256), 0, st, vertices, V, faces, F, g, flags, bits, hdr, list);
    LAUNCH_CHECK();
    if (!(flags & SURFD_VOXEL_FORCE_SMALL)) {
        const unsigned wgs = (unsigned)std::min<long long>(VX_LARGE_WGS, ceil_div<long long>(F, 4));
        hipLaunchKernelGGL(vx_surface_large_kernel, dim3(wgs), dim3(256), 0, st, vertices, V, faces, g, bits, hdr, list, (unsigned)F);
        LAUNCH_CHECK();
    }
    return SURFD_OK;
}

extern "C" {

int64_t surfd_voxel_workspace_bytes(int F, int R) {
    if (F < 0 || R < 1 || R > VX_MAX_R) return 0;
    const int64_t W = (R + 31) / 32;
    return (int64_t)sizeof(unsigned) * (VX_HDR + (int64_t)F + (int64_t)R * R * W + (int64_t)R * R);
}

int surfd_voxel_surface(const float *vertices, int V, const int32_t *faces, int F, float lo, float hi, int R, int flags, void *workspace,
                        uint32_t *bits, int32_t *dropped, int32_t *degenerate, surfd_stream s) {
    VxGrid g;
    if (int rc = vx_grid("surfd_voxel_surface", lo, hi, R, g)) return rc;
    if (int rc = vx_mesh_args("surfd_voxel_surface", vertices, V, faces, F, flags, workspace, bits)) return rc;
    hipStream_t st = as_stream(s);
    unsigned *hdr = static_cast<unsigned *>(workspace);
    if (int rc = vx_surface_pass(vertices, V, faces, F, g, flags, hdr, bits, st)) return rc;
    if (dropped) HIP_TRY(hipMemcpyAsync(dropped, hdr + 1, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (degenerate) HIP_TRY(hipMemcpyAsync(degenerate, hdr + 2, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return SURFD_OK;
}

int surfd_voxel_solid(const float *vertices, int V, const int32_t *faces, int F, float lo, float hi, int R, int flags, void *workspace,
                      int include_surface, uint32_t *bits, int32_t *odd_columns, int32_t *dropped, surfd_stream s) {
    VxGrid g;
    if (int rc = vx_grid("surfd_voxel_solid", lo, hi, R, g)) return rc;
    if (int rc = vx_mesh_args("surfd_voxel_solid", vertices, V, faces, F, flags, workspace, bits)) return rc;
    hipStream_t st = as_stream(s);
    unsigned *hdr = static_cast<unsigned *>(workspace), *list = hdr + VX_HDR;
    unsigned *fill = list + F, *parity = fill + (size_t)R * R * g.W;
    if (include_surface)
        if (int rc = vx_surface_pass(vertices, V, faces, F, g, flags, hdr, bits, st)) return rc;
    HIP_TRY(hipMemsetAsync(hdr, 0, VX_HDR * sizeof(unsigned), st));
    if (F > 0) {
        HIP_TRY(hipMemsetAsync(fill, 0, ((size_t)R * R * g.W + (size_t)R * R) * sizeof(unsigned), st));
        hipLaunchKernelGGL(vx_solid_small_kernel, dim3((unsigned)ceil_div<long long>(F, 256)), dim3(256), 0, st, vertices, V, faces, F, g, flags, fill, parity,
                           hdr, list);
        LAUNCH_CHECK();
        if (!(flags & SURFD_VOXEL_FORCE_SMALL)) {
            const unsigned wgs = (unsigned)std::min<long long>(VX_LARGE_WGS, ceil_div<long long>(F, 4));
            hipLaunchKernelGGL(vx_solid_large_kernel, dim3(wgs), dim3(256), 0, st, vertices, V, faces, g, fill, parity, hdr, list, (unsigned)F);
            LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(vx_solid_merge_kernel, dim3((unsigned)ceil_div(R * R, 256)), dim3(256), 0, st, fill, parity, g, bits, hdr);
        LAUNCH_CHECK();
    }
    if (dropped) HIP_TRY(hipMemcpyAsync(dropped, hdr + 1, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (odd_columns) HIP_TRY(hipMemcpyAsync(odd_columns, hdr + 3, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return SURFD_OK;
}

int surfd_voxel_points(const float *points, int P, float lo, float hi, int R, uint32_t *bits, int32_t *outside, surfd_stream s) {
    VxGrid g;
    if (int rc = vx_grid("surfd_voxel_points", lo, hi, R, g)) return rc;
    if (P < 0 || (long long)P * 3 >= (1LL << 31)) SURFD_FAIL(SURFD_ERR_ARG, "surfd_voxel_points: P = %d must lie in [0, 2^31 / 3)", P);
    if ((P > 0 && !points) || !bits) SURFD_FAIL(SURFD_ERR_ARG, "surfd_voxel_points: null points or bits");
    hipStream_t st = as_stream(s);
    if (outside) HIP_TRY(hipMemsetAsync(outside, 0, sizeof(int32_t), st));
    if (P == 0) return SURFD_OK;
    hipLaunchKernelGGL(vx_points_kernel, dim3((unsigned)ceil_div<long long>(P, 256)), dim3(256), 0, st, points, P, g, bits, reinterpret_cast<unsigned *>(outside));
    LAUNCH_CHECK();
    return SURFD_OK;
}

int surfd_voxel_iou(const uint32_t *a, int M, const uint32_t *b, int N, int R, int paired, int32_t *inter, int32_t *uni, float *iou, surfd_stream s) {
    if (R < 1 || R > VX_MAX_R) SURFD_FAIL(SURFD_ERR_ARG, "surfd_voxel_iou: R = %d must lie in [1, %d]", R, VX_MAX_R);
    if (M < 0 || N < 0) SURFD_FAIL(SURFD_ERR_ARG, "surfd_voxel_iou: M = %d, N = %d must not be negative", M, N);
    if (paired && M != N) SURFD_FAIL(SURFD_ERR_ARG, "surfd_voxel_iou: the paired form needs M = N (M = %d, N = %d)", M, N);
    const long long pairs = paired ? M : (long long)M * N;
    if (pairs >= (1LL << 31)) SURFD_FAIL(SURFD_ERR_ARG, "surfd_voxel_iou: %lld pairs in one call, the count must stay below 2^31", pairs);
    if (pairs == 0) return SURFD_OK;
    if (!a || !b || !inter || !uni || !iou) SURFD_FAIL(SURFD_ERR_ARG, "surfd_voxel_iou: null a, b, inter, uni or iou");
    hipStream_t st = as_stream(s);
    const int words = R * R * ((R + 31) / 32);                // at most 2^22
    HIP_TRY(hipMemsetAsync(inter, 0, (size_t)pairs * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(uni, 0, (size_t)pairs * sizeof(int32_t), st));
    hipLaunchKernelGGL(vx_iou_kernel, dim3((unsigned)pairs, (unsigned)ceil_div(words, VX_IOU_CHUNK)), dim3(256), 0, st, a, b, N, paired, words, inter, uni);   // at most 1 024 chunks
    LAUNCH_CHECK();
    hipLaunchKernelGGL(vx_iou_finish_kernel, dim3((unsigned)ceil_div<long long>(pairs, 256)), dim3(256), 0, st, inter, uni, (int)pairs, iou);
    LAUNCH_CHECK();
    return SURFD_OK;
}

}  // extern "C"
