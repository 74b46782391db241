// Level-set marching cubes on the device: the mesh of surfd_mc_iso (mcubes.cpp, run_iso, step 1) from a volume that never
// leaves the GPU, bit for bit — vertex order, face order, every float, -0 / +0.
//
// The contract, restated from run_iso / emit_edge / choose (mcubes.cpp):
//   scan      cubes z outermost, y, x innermost, 0 .. n-2 each; the LINEAR VOXEL INDEX of a cube's low corner is its place in the scan.
//   pattern   corner k (marching-cubes order) is above iff (double)value - level > 0.0.
//   fan       classic: the CASESCLASSIC row up to its first -1; else CASES -> (case, config) -> choose() with test_face /
//             test_interior in fp64 as written there (TINY terms, the 0 of cases 5 / 10, both face tests of cases 10 / 12).
//   vertices  one per grid edge with a sign change (edge 12: one per cube), created by the first cube of the scan that names it;
//             ids count creations (within a cube: first appearance in the fan, left to right); the creating cube's arithmetic
//             fixes the bits of the position.
//   normals   fp32 sums in the host's order of addition: cubes in scan order, fan positions left to right, corner c1 then c2,
//             each term (float)(cg * (float)w); then normalised in fp64 as surfd_mc_copy does.  A GATHER per vertex — float
//             atomics cannot give these bits.
//   values    the host's running "if (spread > values[v]) values[v] = (float)spread" over the referencing cubes in scan order.
//
// Who creates a vertex is index arithmetic: every fan of every table names exactly the sign-change edges of its pattern (plus,
// in some, edge 12) — tests/test_mcdevice_cpu.py loops over every row of every table — so the cubes that name a grid edge are
// ALL in-range cubes around it (at most four), and its creator is the first of them in scan order.
//
// Passes (all on the caller's stream; one host read between scan and compact, so that outputs can be sized exactly):
//   classify  one thread per voxel, one wave per CHUNK of 64 consecutive voxel indices: ballot = the chunk's active cubes; active
//             lanes count their triangles and the vertices they create (a fan is worked out only where a test of Lewiner's picks it)
//   scan      exclusive prefix of (active, triangles, vertices) in scan order, two levels: chunks inside groups of 1024 (in
//             place), then one workgroup over the groups; grand totals (A, F, V) -> host
//   compact   one thread per chunk: voxel index of every active cube, in scan order
//   records   one thread per active cube: fan (table offset, triangles), the rank of every vertex it creates
//   bases     one thread per active cube: first vertex id and first triangle of the cube (chunk prefix + earlier cubes of the chunk)
//   emit      one thread per active cube: its triangles (vertex ids looked up in the creators' records) and the vertices it
//             creates (position, gathered normal, value)
// Scratch proportional to the volume: per chunk 8 (mask) + 12 (counts, then prefix) bytes, per group 36: 0.31 bytes per voxel.
// Proportional to the active cubes: one 24-byte record.  Nothing is carried from one run to the next: every pass overwrites
// all it reads.  Measurements and the compiler's resource figures: DESIGN.md section 8.13.
#include "common.h"
#include "mc_luts.h"
#include "meshscene.h"

#include <string.h>

#include <memory>
#include <vector>

namespace {

using surfd::ceil_div;

#define MCD_TINY 2.220446049250313e-16       // mcubes.cpp: TINY
const int MCD_BLOCK = 256;                   // voxels (threads) per classify workgroup = 4 chunks
const int MCD_GROUP = 1024;                  // chunks per workgroup of the first scan level

struct DLut { int off, l1, l2; };            // a table of mc_luts.h inside the flat device copy: at(a, b, c) = flat[off + a l1 l2 + b l2 + c]
struct DLuts {
    DLut ex, ey, ez, cases, classic;
    DLut t1, t2, t3_1, t3_2, t4_1, t4_2, t5, t6_1_1, t6_1_2, t6_2, t7_1, t7_2, t7_3, t7_4_1, t7_4_2, t8, t9;
    DLut t10_1_1, t10_1_1_, t10_1_2, t10_2, t10_2_, t11, t12_1_1, t12_1_1_, t12_1_2, t12_2, t12_2_;
    DLut t13_1, t13_1_, t13_2, t13_2_, t13_3, t13_3_, t13_4, t13_5_1, t13_5_2, t14;
    DLut test3, test4, test6, test7, test10, test12, test13, sub13;
};

struct Dims { int nx, ny, nz; double inv_nx, inv_ny; };

struct Rec {                                 // one active cube
    int voxel;                               // linear index of its low corner
    int fan;                                 // table offset | triangles << 16 | created vertices << 24
    unsigned long long ranks;                // nibble e: rank of edge e's vertex among those this cube creates, 15 = not created here
    int vbase, tbase;                        // first vertex id / first triangle
};

// test_interior: per reference edge the corner pair that fixes t, then three (from, to) pairs for B, C, D (mcubes.cpp)
__constant__ signed char MCD_P[12][8] = {{0, 1, 3, 2, 7, 6, 4, 5}, {1, 2, 0, 3, 4, 7, 5, 6}, {2, 3, 1, 0, 5, 4, 6, 7}, {3, 0, 2, 1, 6, 5, 7, 4},
                                         {4, 5, 7, 6, 3, 2, 0, 1}, {5, 6, 4, 7, 0, 3, 1, 2}, {6, 7, 5, 4, 1, 0, 2, 3}, {7, 4, 6, 5, 2, 1, 3, 0},
                                         {0, 4, 3, 7, 2, 6, 1, 5}, {1, 5, 0, 4, 3, 7, 2, 6}, {2, 6, 1, 5, 0, 4, 3, 7}, {3, 7, 2, 6, 1, 5, 0, 4}};

__device__ __forceinline__ int at(const signed char *lut, DLut t, int a) { return lut[t.off + a]; }
__device__ __forceinline__ int at(const signed char *lut, DLut t, int a, int b) { return lut[t.off + a * t.l1 + b]; }
__device__ __forceinline__ int at(const signed char *lut, DLut t, int a, int b, int c) { return lut[t.off + a * t.l1 * t.l2 + b * t.l2 + c]; }

// n / d for n < 2^32 through the reciprocal in fp64 (off by at most one before the fix-up)
__device__ __forceinline__ unsigned div_u32(unsigned n, unsigned d, double inv, unsigned &rem) {
    unsigned q = (unsigned)((double)n * inv);
    int r = (int)(n - q * d);
    if (r < 0) { --q; r += (int)d; }
    else if (r >= (int)d) { ++q; r -= (int)d; }
    rem = (unsigned)r;
    return q;
}

__device__ __forceinline__ void voxel_xyz(unsigned i, const Dims &D, int &x, int &y, int &z) {
    unsigned rx, ry;
    const unsigned row = div_u32(i, (unsigned)D.nx, D.inv_nx, rx);
    z = (int)div_u32(row, (unsigned)D.ny, D.inv_ny, ry);
    x = (int)rx; y = (int)ry;
}

// The corner values of one cube, read where they lie (cache hits: the neighbours of an active cube are active too); nothing
// is kept in indexed registers, so nothing goes to scratch.
struct Cube {
    const float *p;                          // the low corner
    long nx, nxy;
    double level;
    __device__ __forceinline__ double val(int ix, int iy, int iz) const { return (double)p[iz * nxy + iy * nx + ix] - level; }
    // marching-cubes corner k: (0,0,0) (1,0,0) (1,1,0) (0,1,0), then the same at z + 1
    __device__ __forceinline__ double V(int k) const { return val(((k + 1) >> 1) & 1, (k >> 1) & 1, k >> 2); }
    // cg[k * 3 + c] of prepare(): one-sided differences, low minus high, along each axis through corner k
    __device__ __forceinline__ double grad(int k, int c) const {
        const int ox = ((k + 1) >> 1) & 1, oy = (k >> 1) & 1, oz = k >> 2;
        if (c == 0) return val(0, oy, oz) - val(1, oy, oz);
        if (c == 1) return val(ox, 0, oz) - val(ox, 1, oz);
        return val(ox, oy, 0) - val(ox, oy, 1);
    }
    __device__ int pattern() const {
        int pt = 0;
        for (int k = 0; k < 8; ++k) pt |= (V(k) > 0.0) << k;
        return pt;
    }
    __device__ double spread() const {
        double lo = 0.0, hi = 0.0;
        for (int k = 0; k < 8; ++k) { const double c = V(k); if (c > hi) hi = c; if (c < lo) lo = c; }
        return hi - lo;
    }
};

__device__ bool test_face(const Cube &c, int face) {
    const int f = face < 0 ? -face : face;
    double A = 0, B = 0, C = 0, D = 0;
    switch (f) {
        case 1: A = c.V(0); B = c.V(4); C = c.V(5); D = c.V(1); break;
        case 2: A = c.V(1); B = c.V(5); C = c.V(6); D = c.V(2); break;
        case 3: A = c.V(2); B = c.V(6); C = c.V(7); D = c.V(3); break;
        case 4: A = c.V(3); B = c.V(7); C = c.V(4); D = c.V(0); break;
        case 5: A = c.V(0); B = c.V(3); C = c.V(2); D = c.V(1); break;
        case 6: A = c.V(4); B = c.V(7); C = c.V(6); D = c.V(5); break;
        default: break;
    }
    const double q = A * C - B * D;
    if (q > -MCD_TINY && q < MCD_TINY) return face >= 0;
    return face * A * q >= 0;
}

__device__ bool test_interior(const Cube &c, const signed char *lut, const DLuts &L, int mc_case, int config, int subconfig, int s) {
    double t, At = 0.0, Bt = 0.0, Ct = 0.0, Dt = 0.0;
    if (mc_case == 4 || mc_case == 10) {
        const double v0 = c.V(0), v1 = c.V(1), v2 = c.V(2), v3 = c.V(3), v4 = c.V(4), v5 = c.V(5), v6 = c.V(6), v7 = c.V(7);
        const double a = (v4 - v0) * (v6 - v2) - (v7 - v3) * (v5 - v1);
        const double b = v2 * (v4 - v0) + v0 * (v6 - v2) - v1 * (v7 - v3) - v3 * (v5 - v1);
        t = -b / (2 * a + MCD_TINY);
        if (t < 0 || t > 1) return s > 0;
        At = v0 + (v4 - v0) * t; Bt = v3 + (v7 - v3) * t; Ct = v2 + (v6 - v2) * t; Dt = v1 + (v5 - v1) * t;
    } else {
        int edge = -1;
        if (mc_case == 6) edge = at(lut, L.test6, config, 2);
        else if (mc_case == 7) edge = at(lut, L.test7, config, 4);
        else if (mc_case == 12) edge = at(lut, L.test12, config, 3);
        else if (mc_case == 13) edge = at(lut, L.t13_5_1, config, subconfig, 0);
        if (edge >= 0 && edge < 12) {
            const signed char *p = MCD_P[edge];
            const double vp0 = c.V(p[0]);
            t = vp0 / (vp0 - c.V(p[1]) + MCD_TINY);
            At = 0;
            const double vp2 = c.V(p[2]), vp4 = c.V(p[4]), vp6 = c.V(p[6]);
            Bt = vp2 + (c.V(p[3]) - vp2) * t;
            Ct = vp4 + (c.V(p[5]) - vp4) * t;
            Dt = vp6 + (c.V(p[7]) - vp6) * t;
        }
    }
    int test = 0;
    if (At >= 0) test += 1;
    if (Bt >= 0) test += 2;
    if (Ct >= 0) test += 4;
    if (Dt >= 0) test += 8;
    switch (test) {
        case 5: return (At * Ct - Bt * Dt < MCD_TINY) ? s > 0 : false;
        case 10: return (At * Ct - Bt * Dt >= MCD_TINY) ? s > 0 : false;
        case 7: case 11: case 13: case 14: case 15: return s < 0;
        default: return s > 0;
    }
}

struct Fan { int off, nt; };                 // the fan's edges are flat[off .. off + 3 nt)
__device__ __forceinline__ Fan row(DLut t, int config, int nt) { return {t.off + config * t.l1, nt}; }
__device__ __forceinline__ Fan row(DLut t, int config, int sub, int nt) { return {t.off + config * t.l1 * t.l2 + sub * t.l2, nt}; }

// choose() of mcubes.cpp
__device__ Fan choose(const Cube &c, const signed char *lut, const DLuts &L, int mc_case, int config) {
    int sub = 0;
    switch (mc_case) {
        case 1: return row(L.t1, config, 1);
        case 2: return row(L.t2, config, 2);
        case 3: return test_face(c, at(lut, L.test3, config)) ? row(L.t3_2, config, 4) : row(L.t3_1, config, 2);
        case 4: return test_interior(c, lut, L, 4, config, 0, at(lut, L.test4, config)) ? row(L.t4_1, config, 2) : row(L.t4_2, config, 6);
        case 5: return row(L.t5, config, 3);
        case 6:
            if (test_face(c, at(lut, L.test6, config, 0))) return row(L.t6_2, config, 5);
            return test_interior(c, lut, L, 6, config, 0, at(lut, L.test6, config, 1)) ? row(L.t6_1_1, config, 3) : row(L.t6_1_2, config, 9);
        case 7:
            if (test_face(c, at(lut, L.test7, config, 0))) sub += 1;
            if (test_face(c, at(lut, L.test7, config, 1))) sub += 2;
            if (test_face(c, at(lut, L.test7, config, 2))) sub += 4;
            switch (sub) {
                case 0: return row(L.t7_1, config, 3);
                case 1: return row(L.t7_2, config, 0, 5);
                case 2: return row(L.t7_2, config, 1, 5);
                case 3: return row(L.t7_3, config, 0, 9);
                case 4: return row(L.t7_2, config, 2, 5);
                case 5: return row(L.t7_3, config, 1, 9);
                case 6: return row(L.t7_3, config, 2, 9);
                default: return test_interior(c, lut, L, 7, config, 7, at(lut, L.test7, config, 3)) ? row(L.t7_4_2, config, 9) : row(L.t7_4_1, config, 5);
            }
        case 8: return row(L.t8, config, 2);
        case 9: return row(L.t9, config, 4);
        case 10: {
            const bool f0 = test_face(c, at(lut, L.test10, config, 0));
            const bool f1 = test_face(c, at(lut, L.test10, config, 1));
            if (f0) return f1 ? row(L.t10_1_1_, config, 4) : row(L.t10_2, config, 8);
            if (f1) return row(L.t10_2_, config, 8);
            return test_interior(c, lut, L, 10, config, 0, at(lut, L.test10, config, 2)) ? row(L.t10_1_1, config, 4) : row(L.t10_1_2, config, 8);
        }
        case 11: return row(L.t11, config, 4);
        case 12: {
            const bool f0 = test_face(c, at(lut, L.test12, config, 0));
            const bool f1 = test_face(c, at(lut, L.test12, config, 1));
            if (f0) return f1 ? row(L.t12_1_1_, config, 4) : row(L.t12_2, config, 8);
            if (f1) return row(L.t12_2_, config, 8);
            return test_interior(c, lut, L, 12, config, 0, at(lut, L.test12, config, 2)) ? row(L.t12_1_1, config, 4) : row(L.t12_1_2, config, 8);
        }
        case 13: {
            for (int k = 0; k < 6; ++k)
                if (test_face(c, at(lut, L.test13, config, k))) sub += 1 << k;
            sub = at(lut, L.sub13, sub);
            if (sub == 0) return row(L.t13_1, config, 4);
            if (sub <= 6) return row(L.t13_2, config, sub - 1, 6);
            if (sub <= 18) return row(L.t13_3, config, sub - 7, 10);
            if (sub <= 22) return row(L.t13_4, config, sub - 19, 12);
            if (sub <= 26) {
                const int k = sub - 23;
                return test_interior(c, lut, L, 13, config, k, at(lut, L.test13, config, 6)) ? row(L.t13_5_1, config, k, 6) : row(L.t13_5_2, config, k, 10);
            }
            if (sub <= 38) return row(L.t13_3_, config, sub - 27, 10);
            if (sub <= 44) return row(L.t13_2_, config, sub - 39, 6);
            if (sub == 45) return row(L.t13_1_, config, 4);
            return {0, 0};
        }
        case 14: return row(L.t14, config, 4);
        default: return {0, 0};
    }
}

__device__ Fan fan_of(const Cube &c, const signed char *lut, const DLuts &L, int pattern, int classic) {
    if (classic) {
        const int off = L.classic.off + pattern * L.classic.l1;
        int nt = 0;
        while (nt < 5 && lut[off + 3 * nt] != -1) ++nt;
        return {off, nt};
    }
    const int mc_case = at(lut, L.cases, pattern, 0);
    if (mc_case <= 0) return {0, 0};
    return choose(c, lut, L, mc_case, at(lut, L.cases, pattern, 1));
}

// ---- grid edges --------------------------------------------------------------------------------------------------------------
// Edge e < 12 of the cube at (x, y, z) is the grid edge along `axis` that starts at voxel (x + ox, y + oy, z + oz) (cache_slot of
// mcubes.cpp).  The cubes around a grid edge, in scan order, are s = 0 .. 3: the edge's voxel minus (a, b, c), the two free
// offsets counting down from 1, z before y before x.
struct GridEdge { int X, Y, Z, axis; };
struct Sharer { int x, y, z, e; bool ok; };

__device__ __forceinline__ GridEdge grid_edge(int x, int y, int z, int e) {
    int axis, ox = 0, oy = 0, oz = 0;
    if (e < 8) {
        const int h = e & 3;
        axis = h & 1;
        ox = h == 1; oy = h == 2; oz = e >> 2;
    } else {
        axis = 2;
        ox = e == 9 || e == 10; oy = e >= 10;
    }
    return {x + ox, y + oy, z + oz, axis};
}

__device__ __forceinline__ Sharer sharer(const GridEdge &g, int s, const Dims &D) {
    const int mj = 1 - (s >> 1), mn = 1 - (s & 1);
    const int a = g.axis == 0 ? 0 : mn;
    const int b = g.axis == 0 ? mn : (g.axis == 1 ? 0 : mj);
    const int c = g.axis == 2 ? 0 : mj;
    Sharer r;
    r.x = g.X - a; r.y = g.Y - b; r.z = g.Z - c;
    r.ok = r.x >= 0 && r.y >= 0 && r.z >= 0 && r.x <= D.nx - 2 && r.y <= D.ny - 2 && r.z <= D.nz - 2;
    r.e = g.axis == 0 ? 2 * b + 4 * c : (g.axis == 1 ? (a ? 1 : 3) + 4 * c : 8 + (b ? (a ? 2 : 3) : a));
    return r;
}

__device__ __forceinline__ Sharer creator(int x, int y, int z, int e, const Dims &D) {
    const GridEdge g = grid_edge(x, y, z, e);
    Sharer r = sharer(g, 0, D);
    for (int s = 1; s < 4 && !r.ok; ++s) r = sharer(g, s, D);
    return r;                                // ok: the cube itself is one of the four
}

// the vertices the cube creates: nibble e of `ranks` = their order of creation, 15 elsewhere; returns how many
__device__ int created(const signed char *lut, Fan f, int x, int y, int z, const Dims &D, unsigned long long &ranks) {
    ranks = ~0ull;
    unsigned seen = 0;
    int nv = 0;
    for (int k = 0; k < 3 * f.nt; ++k) {
        const int e = lut[f.off + k];
        if ((seen >> e) & 1) continue;
        seen |= 1u << e;
        bool mine = e == 12;
        if (!mine) {
            const Sharer cr = creator(x, y, z, e, D);
            mine = cr.x == x && cr.y == y && cr.z == z;
        }
        if (mine) {
            ranks = (ranks & ~(15ull << (4 * e))) | ((unsigned long long)nv << (4 * e));
            ++nv;
        }
    }
    return nv;
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int above(float v, double level) { return (double)v - level > 0.0; }

// the edges of a cube whose corners lie on different sides, from its pattern: edge k < 4 joins corners k and (k + 1) % 4, edge
// 4 + k the same one layer up, edge 8 + k corners k and 4 + k.  Every fan names exactly these (tests/test_mcdevice_cpu.py).
__device__ __forceinline__ unsigned crossing_edges(int pattern) {
    const unsigned lo = pattern & 15, hi = (pattern >> 4) & 15;
    return (lo ^ (((lo >> 1) | (lo << 3)) & 15)) | (hi ^ (((hi >> 1) | (hi << 3)) & 15)) << 4 | (lo ^ hi) << 8;
}

// the edges whose vertex the cube at (x, y, z) creates if they cross: the cubes before it around the edge lie one step down along
// the edge's free axes, so it is first where its own offset there is 1 or its coordinate is 0 (creator() restated per edge)
__device__ __forceinline__ unsigned owned_edges(int x, int y, int z) {
    const unsigned X0 = x == 0, Y0 = y == 0, Z0 = z == 0;
    return 0x460u | Z0 * 0x006u | Y0 * 0x210u | X0 * 0x880u | (Y0 & Z0) | (X0 & Z0) << 3 | (X0 & Y0) << 8;
}

// ---- classify ----------------------------------------------------------------------------------------------------------------
// mask[chunk]: the chunk's active cubes; chunkcnt[chunk * 3 ..]: its (active, triangles, vertices).  A lane reads its own column
// (x; y, y+1; z, z+1) and takes the column at x + 1 from the next lane: four loads per voxel, coalesced along x.  `thr` is the
// largest float <= level: for a float v, v > thr exactly where (double)v - level > 0.0 (the next float above thr lies above the
// level, and a difference of doubles is 0 only between equal ones), so the stream is compared in fp32.  Counting needs no fan
// where the pattern fixes it (ntab: triangles per pattern, classic table first, then Lewiner's with 255 where a face or
// interior test decides): the vertices a cube creates are its crossing edges among those it owns, plus the interior vertex of
// a fan that names edge 12.
__global__ __launch_bounds__(MCD_BLOCK) void mcd_classify(const float *__restrict__ im, Dims D, double level, float thr, int classic,
                                                          const signed char *__restrict__ lut, const DLuts *__restrict__ L,
                                                          const unsigned char *__restrict__ ntab, unsigned long long *__restrict__ mask,
                                                          int *__restrict__ chunkcnt) {
    const unsigned nvox = (unsigned)D.nx * D.ny * D.nz;
    const unsigned i = blockIdx.x * (unsigned)MCD_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const long nx = D.nx, nxy = (long)D.nx * D.ny;
    int x = 0, y = 0, z = 0;
    const bool in = i < nvox;
    if (in) voxel_xyz(i, D, x, y, z);
    const bool col = in && y <= D.ny - 2 && z <= D.nz - 2;
    const bool cube = col && x <= D.nx - 2;
    // (both sets of loads are issued before either is used: the last lane's second column costs no second round trip)
    float a0 = thr, a1 = thr, a2 = thr, a3 = thr, b0 = thr, b1 = thr, b2 = thr, b3 = thr;
    if (col) {
        const float *p = im + i;
        a0 = p[0]; a1 = p[nx]; a2 = p[nxy]; a3 = p[nxy + nx];
    }
    if (lane == 63 && cube) {
        const float *p = im + i + 1;
        b0 = p[0]; b1 = p[nx]; b2 = p[nxy]; b3 = p[nxy + nx];
    }
    const int nib = (a0 > thr) | (a1 > thr) << 1 | (a2 > thr) << 2 | (a3 > thr) << 3;
    int nb = __shfl_down(nib, 1);
    if (lane == 63) nb = (b0 > thr) | (b1 > thr) << 1 | (b2 > thr) << 2 | (b3 > thr) << 3;
    const int pattern = (nib & 1) | (nb & 1) << 1 | (nb & 2) << 1 | (nib & 2) << 2 | (nib & 4) << 2 | (nb & 4) << 3 | (nb & 8) << 3 | (nib & 8) << 4;
    const bool act = cube && pattern != 0 && pattern != 255;
    const unsigned long long m = __ballot(act);
    int nt = 0, nv = 0;
    if (m) {
        if (act) {
            nt = ntab[(classic ? 0 : 256) + pattern];
            nv = __popc(crossing_edges(pattern) & owned_edges(x, y, z));
            if (nt == 255) {                               // an ambiguous case of Lewiner's: the tests pick the fan
                const Cube c{im + i, nx, nxy, level};
                const Fan f = fan_of(c, lut, *L, pattern, 0);
                nt = f.nt;
                int interior = 0;
                for (int k = 0; k < 3 * f.nt; ++k) interior |= lut[f.off + k] == 12;
                nv += interior;
            }
        }
        nt = wave_sum(nt); nv = wave_sum(nv);
    }
    if (lane == 0) {
        const size_t chunk = i >> 6;
        mask[chunk] = m;
        chunkcnt[chunk * 3] = __popcll(m); chunkcnt[chunk * 3 + 1] = nt; chunkcnt[chunk * 3 + 2] = nv;
    }
}

// One level of the exclusive prefix, in scan order: workgroup g takes `per` consecutive entries (a contiguous segment per thread),
// leaves in base[] what lies before each entry INSIDE the workgroup (base may be cnt: every thread reads its segment before any
// thread writes) and the workgroup's total in tot[g * 3 ..].  Chunks -> groups of 1024 chunks -> one workgroup over the groups.
template <typename TIn>
__global__ __launch_bounds__(1024) void mcd_scan(const TIn *cnt, int *base, int n, int per, long long *__restrict__ tot) {
    __shared__ long long part[3][1024];
    const int t = threadIdx.x, seg = per / 1024;
    const long long first = (long long)blockIdx.x * per;
    const int lo = (int)min((long long)n, first + (long long)t * seg), hi = (int)min((long long)n, (long long)lo + seg);
    long long own[3] = {0, 0, 0};
    for (int j = lo; j < hi; ++j)
        for (int c = 0; c < 3; ++c) own[c] += cnt[(size_t)j * 3 + c];
    for (int c = 0; c < 3; ++c) part[c][t] = own[c];
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        long long v[3] = {0, 0, 0};
        if (t >= off) for (int c = 0; c < 3; ++c) v[c] = part[c][t - off];
        __syncthreads();
        if (t >= off) for (int c = 0; c < 3; ++c) part[c][t] += v[c];
        __syncthreads();
    }
    long long run[3];
    for (int c = 0; c < 3; ++c) run[c] = part[c][t] - own[c];
    for (int j = lo; j < hi; ++j)
        for (int c = 0; c < 3; ++c) {
            const long long here = cnt[(size_t)j * 3 + c];
            base[(size_t)j * 3 + c] = (int)run[c];             // (meaningless past 2^31: the host refuses such a run before anything reads it)
            run[c] += here;
        }
    if (t == 1023) for (int c = 0; c < 3; ++c) tot[(size_t)blockIdx.x * 3 + c] = part[c][t];
}

struct Scratch {
    const unsigned long long *mask;
    const int *chunkpref, *groupbase;
    // (active, triangles, vertices)[c] of everything before the chunk
    __device__ __forceinline__ int before(unsigned chunk, int c) const { return groupbase[(size_t)(chunk / MCD_GROUP) * 3 + c] + chunkpref[(size_t)chunk * 3 + c]; }
    // place of the cube at voxel i among the active cubes, -1 if it is not active
    __device__ __forceinline__ int active_index(unsigned i) const {
        const unsigned chunk = i >> 6, bit = i & 63;
        const unsigned long long m = mask[chunk];
        if (!((m >> bit) & 1)) return -1;
        return before(chunk, 0) + __popcll(m & ((1ull << bit) - 1));
    }
};

__global__ __launch_bounds__(256) void mcd_compact(Scratch S, unsigned nchunks, Rec *__restrict__ recs) {
    const unsigned chunk = blockIdx.x * 256u + threadIdx.x;
    if (chunk >= nchunks) return;
    unsigned long long m = S.mask[chunk];
    if (!m) return;
    int a = S.before(chunk, 0);
    while (m) {
        const int bit = __ffsll((long long)m) - 1;
        m &= m - 1;
        recs[a++].voxel = (int)(chunk * 64u + bit);
    }
}

__global__ __launch_bounds__(256) void mcd_records(const float *__restrict__ im, Dims D, double level, int classic, const signed char *__restrict__ lut, DLuts L,
                                                   int A, Rec *__restrict__ recs) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    const unsigned i = (unsigned)recs[a].voxel;
    int x, y, z;
    voxel_xyz(i, D, x, y, z);
    const Cube c{im + i, (long)D.nx, (long)D.nx * D.ny, level};
    const Fan f = fan_of(c, lut, L, c.pattern(), classic);
    unsigned long long ranks;
    const int nv = created(lut, f, x, y, z, D, ranks);
    recs[a].fan = f.off | f.nt << 16 | nv << 24;
    recs[a].ranks = ranks;
}

__global__ __launch_bounds__(256) void mcd_bases(Scratch S, int A, Rec *__restrict__ recs) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    const unsigned chunk = (unsigned)recs[a].voxel >> 6;
    int t = S.before(chunk, 1), v = S.before(chunk, 2);
    for (int j = S.before(chunk, 0); j < a; ++j) {
        const int fan = recs[j].fan;
        t += (fan >> 16) & 255; v += (fan >> 24) & 255;
    }
    recs[a].tbase = t; recs[a].vbase = v;
}

// ---- emit ------------------------------------------------------------------------------------------------------------------------
// what one cube adds to the vertex on its edge e (emit_edge of mcubes.cpp): per fan position that names e, corner c1 then c2
__device__ void add_cube(const float *im, const Dims &D, double level, const signed char *lut, const DLuts &L, const Sharer &s, int fan,
                         float acc[3], float &value) {
    const long nx = D.nx, nxy = (long)D.nx * D.ny;
    const Cube c{im + (s.z * nxy + s.y * nx + s.x), nx, nxy, level};
    const int off = fan & 0xffff, n3 = 3 * ((fan >> 16) & 255);
    int refs = 0;
    for (int k = 0; k < n3; ++k) refs += lut[off + k] == s.e;
    if (!refs) return;
    const double spread = c.spread();
    if (spread > value) value = (float)spread;
    const int dx1 = at(lut, L.ex, s.e, 0), dx2 = at(lut, L.ex, s.e, 1), dy1 = at(lut, L.ey, s.e, 0), dy2 = at(lut, L.ey, s.e, 1);
    const int dz1 = at(lut, L.ez, s.e, 0), dz2 = at(lut, L.ez, s.e, 1);
    // the weights belong to the corners in xyz-bit order, the gradients are the host's cg[] rows, which lie in marching-cubes order
    const int c1 = dz1 * 4 + dy1 * 2 + dx1, c2 = dz2 * 4 + dy2 * 2 + dx2;
    const float w1 = (float)(1.0 / (MCD_TINY + fabs(c.val(dx1, dy1, dz1)))), w2 = (float)(1.0 / (MCD_TINY + fabs(c.val(dx2, dy2, dz2))));
    for (int q = 0; q < 3; ++q) {
        const float t1 = (float)(c.grad(c1, q) * w1), t2 = (float)(c.grad(c2, q) * w2);
        float sum = acc[q];
        for (int r = 0; r < refs; ++r) { sum += t1; sum += t2; }
        acc[q] = sum;
    }
}

__global__ __launch_bounds__(128) void mcd_emit(const float *__restrict__ im, Dims D, double level, const signed char *__restrict__ lut, DLuts L, Scratch S, int A,
                                                int V, int F, const Rec *__restrict__ recs, float *__restrict__ vertices, int32_t *__restrict__ faces,
                                                float *__restrict__ normals, float *__restrict__ values) {
    const int a = blockIdx.x * 128 + threadIdx.x;
    if (a >= A) return;
    const Rec r = recs[a];
    const unsigned i = (unsigned)r.voxel;
    int x, y, z;
    voxel_xyz(i, D, x, y, z);
    const long nx = D.nx, nxy = (long)D.nx * D.ny;
    const int off = r.fan & 0xffff, nt = (r.fan >> 16) & 255;

    // triangles: every one reversed, as surfd_mc_copy hands them out
    for (int k = 0; k < 3 * nt; ++k) {
        const int e = lut[off + k];
        int id = -1;
        if (e == 12) id = r.vbase + (int)((r.ranks >> 48) & 15);
        else {
            const Sharer cr = creator(x, y, z, e, D);
            if (cr.x == x && cr.y == y && cr.z == z) id = r.vbase + (int)((r.ranks >> (4 * e)) & 15);
            else {
                const int j = S.active_index((unsigned)(cr.z * nxy + cr.y * nx + cr.x));
                if (j >= 0) id = recs[j].vbase + (int)((recs[j].ranks >> (4 * cr.e)) & 15);
            }
        }
        if (r.tbase + k / 3 < F) faces[3 * ((size_t)r.tbase + k / 3) + (2 - k % 3)] = id;      // (always: the counts are classify's own)
    }

    // the vertices this cube creates
    const Cube c{im + i, nx, nxy, level};
#pragma unroll 1
    for (int e = 0; e < 13; ++e) {
        const int rank = (int)((r.ranks >> (4 * e)) & 15);
        if (rank == 15) continue;
        const size_t vi = (size_t)r.vbase + rank;
        if (vi >= (size_t)V) continue;                       // (never: as above; a write stays inside the caller's buffers whatever happens)
        float acc[3] = {0.f, 0.f, 0.f}, value = 0.f;
        double px, py, pz;
        if (e == 12) {
            // centre_vertex(): weights 1 / (TINY + |v|) over the eight corners; the z-sum of the gradients lands in the x slot
            double fx = 0.0, fy = 0.0, fz = 0.0, ff = 0.0, sy = 0.0, sz = 0.0;
            for (int k = 0; k < 8; ++k) {
                const double w = 1.0 / (MCD_TINY + fabs(c.V(k)));
                fx += (double)(((k + 1) >> 1) & 1) * w; fy += (double)((k >> 1) & 1) * w; fz += (double)(k >> 2) * w; ff += w;
                if (k == 0) { sy = w * c.grad(k, 1); sz = w * c.grad(k, 2); }
                else { sy = sy + w * c.grad(k, 1); sz = sz + w * c.grad(k, 2); }
            }
            px = x + 1.0 * fx / ff; py = y + 1.0 * fy / ff; pz = z + 1.0 * fz / ff;
            const double spread = c.spread();
            if (spread > value) value = (float)spread;
            int refs = 0;
            for (int k = 0; k < 3 * nt; ++k) refs += lut[off + k] == 12;
            const float gx = (float)sz, gy = (float)sy, gz = (float)0.0;
            for (int q = 0; q < refs; ++q) { acc[0] += gx; acc[1] += gy; acc[2] += gz; }
        } else {
            const int dx1 = at(lut, L.ex, e, 0), dx2 = at(lut, L.ex, e, 1), dy1 = at(lut, L.ey, e, 0), dy2 = at(lut, L.ey, e, 1);
            const int dz1 = at(lut, L.ez, e, 0), dz2 = at(lut, L.ez, e, 1);
            const double w1 = 1.0 / (MCD_TINY + fabs(c.val(dx1, dy1, dz1))), w2 = 1.0 / (MCD_TINY + fabs(c.val(dx2, dy2, dz2)));
            double fx = 0.0, fy = 0.0, fz = 0.0, ff = 0.0;
            fx += (double)dx1 * w1; fy += (double)dy1 * w1; fz += (double)dz1 * w1; ff += w1;
            fx += (double)dx2 * w2; fy += (double)dy2 * w2; fz += (double)dz2 * w2; ff += w2;
            px = (double)x + 1.0 * fx / ff; py = (double)y + 1.0 * fy / ff; pz = (double)z + 1.0 * fz / ff;
            const GridEdge g = grid_edge(x, y, z, e);
#pragma unroll 1
            for (int s = 0; s < 4; ++s) {
                const Sharer sh = sharer(g, s, D);
                if (!sh.ok) continue;
                const int j = S.active_index((unsigned)(sh.z * nxy + sh.y * nx + sh.x));
                if (j >= 0) add_cube(im, D, level, lut, L, sh, recs[j].fan, acc, value);
            }
        }
        // (z, y, x) columns; the normal normalised in fp64 (surfd_mc_copy)
        vertices[3 * vi] = (float)pz; vertices[3 * vi + 1] = (float)py; vertices[3 * vi + 2] = (float)px;
        if (normals) {
            double len = 0.0;
            for (int q = 0; q < 3; ++q) { const double d = acc[q]; len += d * d; }
            if (len > 0.0) len = 1.0 / sqrt(len);
            for (int q = 0; q < 3; ++q) normals[3 * vi + q] = (float)(acc[2 - q] * len);
        }
        if (values) values[vi] = value;
    }
}

static DLut find_dlut(const char *name, const std::vector<int> &offs) {
    for (int i = 0; i < MC_LUT_COUNT; ++i)
        if (!strcmp(MC_LUT_TABLE[i].name, name))
            return {offs[i], MC_LUT_TABLE[i].ndim > 1 ? MC_LUT_TABLE[i].dims[1] : 1, MC_LUT_TABLE[i].ndim > 2 ? MC_LUT_TABLE[i].dims[2] : 1};
    return {0, 1, 1};
}

}  // namespace

struct surfd_mcd {
    Dims D;
    unsigned nvox = 0, nchunks = 0;
    int nblocks = 0, ngroups = 0;
    DLuts L;
    signed char *lut = nullptr;              // the tables of mc_luts.h, one after the other
    DLuts *dL = nullptr;                     // L on the device (classify reads it only where a test decides)
    unsigned char *ntab = nullptr;           // triangles per pattern: classic [256], Lewiner [256] (255: a test decides)
    unsigned long long *mask = nullptr;
    int *chunkpref = nullptr, *groupbase = nullptr;   // chunkpref: classify's counts, then, in place, their prefix inside the group
    long long *grouptot = nullptr;
    long long *totals = nullptr;
    surfd::DeviceArena recs;                 // grows with the largest run seen
    // the last run
    bool ran = false;
    const float *volume = nullptr;
    double level = 0.0;
    int A = 0, V = 0, F = 0;

    ~surfd_mcd() {
        (void)hipFree(lut); (void)hipFree(dL); (void)hipFree(ntab); (void)hipFree(mask); (void)hipFree(chunkpref); (void)hipFree(groupbase); (void)hipFree(grouptot); (void)hipFree(totals);
        recs.release();
    }
    Scratch scratch() const { return {mask, chunkpref, groupbase}; }
};

extern "C" {

int surfd_mcd_create(int nz, int ny, int nx, surfd_mcd **out) {
    if (!out) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mcd_create: null out");
    *out = nullptr;
    if (nx < 2 || ny < 2 || nz < 2) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mcd_create: volume must be at least 2x2x2, got %dx%dx%d", nz, ny, nx);
    if ((long long)nz * ny * nx >= (1ll << 31)) SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_mcd_create: %dx%dx%d voxels do not fit 31 bits", nz, ny, nx);
    std::unique_ptr<surfd_mcd> h(new surfd_mcd());
    h->D = {nx, ny, nz, 1.0 / nx, 1.0 / ny};
    h->nvox = (unsigned)nx * ny * nz;
    h->nblocks = (int)ceil_div<unsigned>(h->nvox, MCD_BLOCK);
    h->nchunks = (unsigned)h->nblocks * (MCD_BLOCK / 64);    // whole workgroups: classify writes every chunk of its workgroup
    h->ngroups = (int)ceil_div<unsigned>(h->nchunks, MCD_GROUP);
    std::vector<int> offs(MC_LUT_COUNT);
    std::vector<signed char> flat;
    for (int i = 0; i < MC_LUT_COUNT; ++i) {
        size_t n = 1;
        for (int k = 0; k < MC_LUT_TABLE[i].ndim; ++k) n *= MC_LUT_TABLE[i].dims[k];
        offs[i] = (int)flat.size();
        flat.insert(flat.end(), MC_LUT_TABLE[i].values, MC_LUT_TABLE[i].values + n);
    }
    if (flat.size() > 0xffff) SURFD_FAIL(SURFD_ERR_STATE, "surfd_mcd_create: the case tables (%zu bytes) outgrew the 16-bit fan offset", flat.size());
    DLuts &L = h->L;
#define T(field, name) L.field = find_dlut(name, offs)
    T(ex, "EDGESRELX"); T(ey, "EDGESRELY"); T(ez, "EDGESRELZ"); T(cases, "CASES"); T(classic, "CASESCLASSIC");
    T(t1, "TILING1"); T(t2, "TILING2"); T(t3_1, "TILING3_1"); T(t3_2, "TILING3_2"); T(t4_1, "TILING4_1"); T(t4_2, "TILING4_2"); T(t5, "TILING5");
    T(t6_1_1, "TILING6_1_1"); T(t6_1_2, "TILING6_1_2"); T(t6_2, "TILING6_2"); T(t7_1, "TILING7_1"); T(t7_2, "TILING7_2"); T(t7_3, "TILING7_3");
    T(t7_4_1, "TILING7_4_1"); T(t7_4_2, "TILING7_4_2"); T(t8, "TILING8"); T(t9, "TILING9");
    T(t10_1_1, "TILING10_1_1"); T(t10_1_1_, "TILING10_1_1_"); T(t10_1_2, "TILING10_1_2"); T(t10_2, "TILING10_2"); T(t10_2_, "TILING10_2_"); T(t11, "TILING11");
    T(t12_1_1, "TILING12_1_1"); T(t12_1_1_, "TILING12_1_1_"); T(t12_1_2, "TILING12_1_2"); T(t12_2, "TILING12_2"); T(t12_2_, "TILING12_2_");
    T(t13_1, "TILING13_1"); T(t13_1_, "TILING13_1_"); T(t13_2, "TILING13_2"); T(t13_2_, "TILING13_2_"); T(t13_3, "TILING13_3"); T(t13_3_, "TILING13_3_");
    T(t13_4, "TILING13_4"); T(t13_5_1, "TILING13_5_1"); T(t13_5_2, "TILING13_5_2"); T(t14, "TILING14");
    T(test3, "TEST3"); T(test4, "TEST4"); T(test6, "TEST6"); T(test7, "TEST7"); T(test10, "TEST10"); T(test12, "TEST12"); T(test13, "TEST13");
    T(sub13, "SUBCONFIG13");
#undef T
    // triangles per pattern, from the tables themselves: the classic row up to its first -1; Lewiner's cases with one fan
    unsigned char ntab[512];
    for (int p = 0; p < 256; ++p) {
        int nt = 0;
        while (nt < 5 && flat[L.classic.off + p * L.classic.l1 + 3 * nt] != -1) ++nt;
        ntab[p] = (unsigned char)nt;
        const int mc_case = flat[L.cases.off + p * L.cases.l1];
        const DLut *one = mc_case == 1 ? &L.t1 : mc_case == 2 ? &L.t2 : mc_case == 5 ? &L.t5 : mc_case == 8 ? &L.t8 : mc_case == 9 ? &L.t9
                        : mc_case == 11 ? &L.t11 : mc_case == 14 ? &L.t14 : nullptr;
        ntab[256 + p] = (unsigned char)(mc_case <= 0 ? 0 : (one ? one->l1 / 3 : 255));
    }
    HIP_TRY(hipMalloc(&h->dL, sizeof(DLuts)));
    HIP_TRY(hipMemcpy(h->dL, &L, sizeof(DLuts), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&h->ntab, sizeof(ntab)));
    HIP_TRY(hipMemcpy(h->ntab, ntab, sizeof(ntab), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&h->lut, flat.size()));
    HIP_TRY(hipMemcpy(h->lut, flat.data(), flat.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc(&h->mask, (size_t)h->nchunks * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc(&h->chunkpref, (size_t)h->nchunks * 3 * sizeof(int)));
    HIP_TRY(hipMalloc(&h->groupbase, (size_t)h->ngroups * 3 * sizeof(int)));
    HIP_TRY(hipMalloc(&h->grouptot, (size_t)h->ngroups * 3 * sizeof(long long)));
    HIP_TRY(hipMalloc(&h->totals, 3 * sizeof(long long)));
    *out = h.release();
    return SURFD_OK;
}

void surfd_mcd_destroy(surfd_mcd *h) { delete h; }

int surfd_mcd_classify(surfd_mcd *h, const float *volume, double level, int classic, surfd_stream s) {
    if (!h || !volume) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mcd_classify: null argument");
    hipStream_t st = surfd::as_stream(s);
    h->ran = false;                          // the masks and counts of the last run are about to be overwritten
    float thr = (float)level;                // the largest float <= level (NaN stays NaN: nothing is above it)
    if ((double)thr > level) thr = nextafterf(thr, -INFINITY);
    hipLaunchKernelGGL(mcd_classify, dim3(h->nblocks), dim3(MCD_BLOCK), 0, st, volume, h->D, level, thr, classic != 0, h->lut, h->dL, h->ntab, h->mask, h->chunkpref);
    LAUNCH_CHECK();
    return SURFD_OK;
}

int surfd_mcd_run(surfd_mcd *h, const float *volume, double level, int classic, surfd_stream s, int64_t *num_vertices, int64_t *num_faces) {
    if (!h || !volume) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mcd_run: null argument");
    hipStream_t st = surfd::as_stream(s);
    const int rc = surfd_mcd_classify(h, volume, level, classic, s);
    if (rc != SURFD_OK) return rc;
    hipLaunchKernelGGL(mcd_scan<int>, dim3(h->ngroups), dim3(1024), 0, st, h->chunkpref, h->chunkpref, (int)h->nchunks, MCD_GROUP, h->grouptot);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(mcd_scan<long long>, dim3(1), dim3(1024), 0, st, h->grouptot, h->groupbase, h->ngroups, 1024 * ceil_div(h->ngroups, 1024), h->totals);
    LAUNCH_CHECK();
    long long tot[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(tot, h->totals, sizeof(tot), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tot[1] > INT32_MAX / 3 || tot[2] > INT32_MAX)
        SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_mcd_run: %lld vertices / %lld faces do not fit 32-bit indices", tot[2], tot[1]);
    h->A = (int)tot[0]; h->F = (int)tot[1]; h->V = (int)tot[2];
    h->volume = volume; h->level = level;
    if (h->A > 0) {
        const int rr = h->recs.reserve((size_t)h->A * sizeof(Rec), st);
        if (rr != SURFD_OK) return rr;
        Rec *recs = (Rec *)h->recs.ptr;
        hipLaunchKernelGGL(mcd_compact, dim3(ceil_div<unsigned>(h->nchunks, 256)), dim3(256), 0, st, h->scratch(), h->nchunks, recs);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(mcd_records, dim3(ceil_div(h->A, 256)), dim3(256), 0, st, volume, h->D, level, classic != 0, h->lut, h->L, h->A, recs);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(mcd_bases, dim3(ceil_div(h->A, 256)), dim3(256), 0, st, h->scratch(), h->A, recs);
        LAUNCH_CHECK();
    }
    h->ran = true;
    if (num_vertices) *num_vertices = h->V;
    if (num_faces) *num_faces = h->F;
    return SURFD_OK;
}

int surfd_mcd_active(const surfd_mcd *h, int64_t *active) {
    if (!h || !active) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mcd_active: null argument");
    if (!h->ran) SURFD_FAIL(SURFD_ERR_STATE, "surfd_mcd_active: no run to report");
    *active = h->A;
    return SURFD_OK;
}

int surfd_mcd_emit(surfd_mcd *h, float *vertices, int32_t *faces, float *normals, float *values, surfd_stream s) {
    if (!h) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mcd_emit: null handle");
    if (!h->ran) SURFD_FAIL(SURFD_ERR_STATE, "surfd_mcd_emit: surfd_mcd_run comes first");
    if (h->A == 0) return SURFD_OK;
    if (!vertices || !faces) SURFD_FAIL(SURFD_ERR_ARG, "surfd_mcd_emit: null vertices or faces");
    hipLaunchKernelGGL(mcd_emit, dim3(ceil_div(h->A, 128)), dim3(128), 0, surfd::as_stream(s), h->volume, h->D, h->level, h->lut, h->L, h->scratch(), h->A,
                       h->V, h->F, (const Rec *)h->recs.ptr, vertices, faces, normals, values);
    LAUNCH_CHECK();
    return SURFD_OK;
}

}  // extern "C"
