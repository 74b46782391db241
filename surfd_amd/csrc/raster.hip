// Z-buffer rasteriser for triangle meshes: depth, barycentrics, normals, masks, a headlight shading and contour (ink) images
// of a mesh seen from up to 64 cameras.  No reference counterpart (the reference opens open3d / pymeshlab windows to look at a
// mesh and takes its condition images from files).  fp32 + integer, VALU only; two-sided (no back-face culling, normals turned
// to the viewer) because the project's surfaces are open and unoriented.  DESIGN.md section 8.4.
//
//   rs_project_kernel — one lane per (view, vertex): camera-space point, pixel coordinates, snap to a 1/256-pixel grid.
//   rs_small_kernel   — one lane per (view, triangle): set-up; a triangle whose clipped box holds at most RS_SMALL_MAX pixel
//                       centres is rasterised by that lane (a short loop over the box), a larger one is appended to a list.
//   rs_large_kernel   — walks the list one triangle per wave, the 64 lanes striding over the box.
//   rs_resolve_kernel — one lane per pixel: decodes the winner and writes face / depth / bary / normal / mask / shaded.
//   rs_contour_kernel — one lane per pixel: ink where mask, depth or normal break against a 4-neighbour.
//
// A camera is 18 floats: the row-major 3x4 world->camera matrix M (x right, y down, z forward), then mode (0 perspective,
// 1 orthographic), fx, fy, cx, cy (pixels), near.  Built on the host in fp64; no trigonometry here.
//
// Arithmetic (every operation below is one separately rounded fp32 operation; the library is built with -ffp-contract=off):
//   camera point   xc = ((M00 x + M01 y) + M02 z) + M03, yc and zc alike with rows 1 and 2
//   pixel          perspective  u = (fx xc) / zc + cx, v = (fy yc) / zc + cy;  orthographic  u = fx xc + cx, v = fy yc + cy
//                  (pixel centres at integer + 0.5; u runs along a row, v down the rows)
//   snap           sx = rint(256 u), sy = rint(256 v) (nearest even; 256 u is exact), int32
//   invalid        zc <= near (or NaN), or |sx| or |sy| > 2^22 (or NaN).  A triangle with an invalid vertex (or with an index
//                  outside [0, V)) is DROPPED and counted per view: there is no near-plane clipping.
//   compared depth per vertex d = 1 - near / zc (perspective: affine in screen space) or zc (orthographic); both >= 0
//   set-up         A2 = (bx - ax)(cy - ay) - (by - ay)(cx - ax) in int64; A2 = 0 skipped; A2 < 0: vertices 1 and 2 swap
//   coverage       rs_pixel(), the one place coverage and depth are formed: at the sample p = (256 i + 128, 256 j + 128)
//                  E0 = edge(b, c, p), E1 = edge(c, a, p), E2 = edge(a, b, p) with edge(p, q, s) = (qx - px)(sy - py) - (qy - py)(sx - px)
//                  in int64 (exact: coordinates below 2^22 and samples below 2^20 give |E| < 2^47); inside when every E > 0, or
//                  E = 0 on a top edge (dy = 0, dx > 0) or a left edge (dy < 0) — the edge's direction after the swap, so of the
//                  two triangles that share an edge exactly one owns its pixels, whatever their windings were.
//   barycentrics   b_i = float(E_i) / float(A2) (int64 -> fp32 to nearest, one division each)
//   depth          d = (b0 d0 + b1 d1) + b2 d2 in the post-swap vertex order; non-negative, so its bits order as an unsigned
//   selection      the pixel's winner is the minimum of key = (bits(d) << 32) | face, taken with a 64-bit atomicMin on a key
//                  buffer initialised to all ones: ties in depth go to the lower face index, and the result does not depend
//                  on traversal order, launch geometry, batch or path.
//   resolve        the winner's b_i again through rs_pixel(); perspective  w_i = b_i / z_i, s = (w0 + w1) + w2, bary_i = w_i / s,
//                  depth = 1 / s;  orthographic  bary_i = b_i, depth = d.  bary is written in the CALLER's vertex order.
//                  face normal: e1 = v1 - v0, e2 = v2 - v0 (camera space, caller's order), n = e1 x e2 (each component one
//                  product minus another), l = sqrt((nx nx + ny ny) + nz nz), n / l (0 when l = 0), negated when nz > 0.
//                  vertex normals: g = (bary0 n0 + bary1 n1) + bary2 n2 per component (world space), rotated by M's 3x3 as
//                  (Mr0 gx + Mr1 gy) + Mr2 gz, then normalised and turned the same way.
//                  shaded = ambient + (1 - ambient) |(nx lx + ny ly) + nz lz|.
//
// Hazards: the key buffer is the only memory two lanes may write; they do so with atomicMin only (unsigned 64-bit, a vector
// atomic), and the resolve kernel runs after the raster kernels in stream order.  The list of large triangles is filled through
// an atomicAdd counter; its order varies from run to run, the image does not (the minimum is order-free).  The per-view dropped
// counts are integer atomicAdd.  Every loop is bounded by the clipped box or the list length; no kernel waits on another
// workgroup; no LDS.  The projected vertices and the list live in the handle's arena (meshscene.h).
#include "common.h"
#include "meshscene.h"
#include <cmath>
#include <climits>
#include <cstring>
#include <algorithm>

namespace surfd {

constexpr int RS_SMALL_MAX = 16;          // pixel centres in a clipped box up to which the set-up lane rasterises it itself
constexpr int RS_CAM = 18;                // floats per camera
constexpr int RS_MAX_VIEWS = 64;
constexpr int RS_MAX_SIZE = 2048;
constexpr int RS_SNAP_MAX = 1 << 22;      // largest snapped coordinate in sub-pixel units
constexpr int RS_LARGE_WGS = 1024;        // workgroups of 4 waves that walk the list of large triangles

struct RsVert {                           // one projected vertex of one view
    int sx, sy;                           // snapped pixel coordinates (1/256 pixel); sx = INT_MIN marks an invalid vertex
    float d;                              // compared depth
    float x, y, z;                        // camera-space point
};

struct RsTri {                            // a set-up triangle: post-swap order
    int ax, ay, bx, by, cx, cy;
    long long a2;                         // doubled area, > 0
    float d0, d1, d2;
    bool tl0, tl1, tl2;                   // edge (b,c), (c,a), (a,b) is a top or a left edge
    bool swapped;
    int i0, i1, j0, j1;                   // clipped box in pixels (inclusive); empty when i0 > i1 or j0 > j1
};

__device__ __forceinline__ long long rs_edge(int px, int py, int qx, int qy, long long sx, long long sy) {
    return (long long)(qx - px) * (sy - py) - (long long)(qy - py) * (sx - px);
}

__device__ __forceinline__ bool rs_top_left(int px, int py, int qx, int qy) {
    const int dx = qx - px, dy = qy - py;
    return (dy == 0 && dx > 0) || dy < 0;
}

// 0 = drawable, 1 = dropped (invalid vertex), 2 = nothing to draw (zero area or empty box)
__device__ __forceinline__ int rs_setup(const RsVert &v0, const RsVert &v1, const RsVert &v2, int W, int H, RsTri &t) {
    if (v0.sx == INT_MIN || v1.sx == INT_MIN || v2.sx == INT_MIN) return 1;
    const long long a2 = (long long)(v1.sx - v0.sx) * (v2.sy - v0.sy) - (long long)(v1.sy - v0.sy) * (v2.sx - v0.sx);
    if (a2 == 0) return 2;
    t.swapped = a2 < 0;
    const RsVert &b = t.swapped ? v2 : v1, &c = t.swapped ? v1 : v2;
    t.a2 = t.swapped ? -a2 : a2;
    t.ax = v0.sx; t.ay = v0.sy; t.bx = b.sx; t.by = b.sy; t.cx = c.sx; t.cy = c.sy;
    t.d0 = v0.d; t.d1 = b.d; t.d2 = c.d;
    t.tl0 = rs_top_left(t.bx, t.by, t.cx, t.cy);
    t.tl1 = rs_top_left(t.cx, t.cy, t.ax, t.ay);
    t.tl2 = rs_top_left(t.ax, t.ay, t.bx, t.by);
    const int xmin = min(t.ax, min(t.bx, t.cx)), xmax = max(t.ax, max(t.bx, t.cx));
    const int ymin = min(t.ay, min(t.by, t.cy)), ymax = max(t.ay, max(t.by, t.cy));
    // pixel centres 256 i + 128 inside [xmin, xmax]: ceil and floor by arithmetic shift (coordinates are within +-2^22)
    t.i0 = max(0, (xmin - 128 + 255) >> 8); t.i1 = min(W - 1, (xmax - 128) >> 8);
    t.j0 = max(0, (ymin - 128 + 255) >> 8); t.j1 = min(H - 1, (ymax - 128) >> 8);
    return (t.i0 > t.i1 || t.j0 > t.j1) ? 2 : 0;
}

// the one place coverage and depth are formed
__device__ __forceinline__ bool rs_pixel(const RsTri &t, int i, int j, float &b0, float &b1, float &b2, float &d) {
    const long long sx = 256LL * i + 128, sy = 256LL * j + 128;
    const long long e0 = rs_edge(t.bx, t.by, t.cx, t.cy, sx, sy);
    const long long e1 = rs_edge(t.cx, t.cy, t.ax, t.ay, sx, sy);
    const long long e2 = rs_edge(t.ax, t.ay, t.bx, t.by, sx, sy);
    const bool inside = (e0 > 0 || (e0 == 0 && t.tl0)) && (e1 > 0 || (e1 == 0 && t.tl1)) && (e2 > 0 || (e2 == 0 && t.tl2));
    const float fa = (float)t.a2;
    b0 = __fdiv_rn((float)e0, fa);
    b1 = __fdiv_rn((float)e1, fa);
    b2 = __fdiv_rn((float)e2, fa);
    d = __fadd_rn(__fadd_rn(__fmul_rn(b0, t.d0), __fmul_rn(b1, t.d1)), __fmul_rn(b2, t.d2));
    return inside;
}

__device__ __forceinline__ void rs_emit(const RsTri &t, int i, int j, int f, unsigned long long *keys_view, int W) {
    float b0, b1, b2, d;
    if (rs_pixel(t, i, j, b0, b1, b2, d)) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)f;
        atomicMin(keys_view + (size_t)j * W + i, key);
    }
}

__device__ __forceinline__ float rs_row(const float *m, float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z)), m[3]);
}

// grid (ceil(V / 256), views)
__global__ __launch_bounds__(256) void rs_project_kernel(const float *__restrict__ vertices, int V, const float *__restrict__ cams,
                                                         RsVert *__restrict__ out) {
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;       // V may be 2^31 - 1: the last block's lanes pass INT_MAX
    const int view = blockIdx.y;
    if (n >= V) return;
    const float *cam = cams + view * RS_CAM;
    const float x = vertices[(size_t)n * 3], y = vertices[(size_t)n * 3 + 1], z = vertices[(size_t)n * 3 + 2];
    const float xc = rs_row(cam, x, y, z), yc = rs_row(cam + 4, x, y, z), zc = rs_row(cam + 8, x, y, z);
    const bool ortho = cam[12] != 0.f;
    const float fx = cam[13], fy = cam[14], cx = cam[15], cy = cam[16], near = cam[17];
    RsVert r;
    r.x = xc; r.y = yc; r.z = zc;
    r.sx = INT_MIN; r.sy = 0; r.d = 0.f;
    if (zc > near) {                                           // false for NaN; near >= 0, so zc > 0 below
        float u, v;
        if (ortho) {
            u = __fadd_rn(__fmul_rn(fx, xc), cx);
            v = __fadd_rn(__fmul_rn(fy, yc), cy);
            r.d = zc;
        } else {
            u = __fadd_rn(__fdiv_rn(__fmul_rn(fx, xc), zc), cx);
            v = __fadd_rn(__fdiv_rn(__fmul_rn(fy, yc), zc), cy);
            r.d = __fsub_rn(1.f, __fdiv_rn(near, zc));
        }
        const float su = rintf(__fmul_rn(u, 256.f)), sv = rintf(__fmul_rn(v, 256.f));
        if (fabsf(su) <= (float)RS_SNAP_MAX && fabsf(sv) <= (float)RS_SNAP_MAX) {     // false for NaN and Inf
            r.sx = (int)su; r.sy = (int)sv;
        }
    }
    out[(size_t)view * V + n] = r;
}

// loads and sets up triangle f of a view; indices outside [0, V) count as an invalid vertex
__device__ __forceinline__ int rs_load(const RsVert *__restrict__ vv, int V, const int *__restrict__ faces, int f, int W, int H, RsTri &t) {
    const int a = faces[(size_t)f * 3], b = faces[(size_t)f * 3 + 1], c = faces[(size_t)f * 3 + 2];
    if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) return 1;
    const RsVert v0 = vv[a], v1 = vv[b], v2 = vv[c];
    return rs_setup(v0, v1, v2, W, H, t);
}

// grid (ceil(F / 256), views); counters[0] = length of the list, counters[1 + view] = dropped triangles
__global__ __launch_bounds__(256) void rs_small_kernel(const RsVert *__restrict__ verts, int V, const int *__restrict__ faces, int F,
                                                       int W, int H, int flags, unsigned long long *__restrict__ keys,
                                                       unsigned long long *__restrict__ list, unsigned *__restrict__ counters) {
    const long long fl = (long long)blockIdx.x * 256 + threadIdx.x;      // F may be 2^31 - 1
    const int view = blockIdx.y;
    if (fl >= F) return;
    const int f = (int)fl;
    RsTri t;
    const int rc = rs_load(verts + (size_t)view * V, V, faces, f, W, H, t);
    if (rc == 1) atomicAdd(counters + 1 + view, 1u);
    if (rc != 0) return;
    const int count = (t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1);
    const bool large = (flags & SURFD_RASTER_FORCE_LARGE) || (count > RS_SMALL_MAX && !(flags & SURFD_RASTER_FORCE_SMALL));
    if (large) {
        const unsigned slot = atomicAdd(counters, 1u);       // below views * F, the capacity of the list
        list[slot] = ((unsigned long long)view << 32) | (unsigned)f;
        return;
    }
    unsigned long long *kv = keys + (size_t)view * W * H;
    for (int j = t.j0; j <= t.j1; ++j)
        for (int i = t.i0; i <= t.i1; ++i) rs_emit(t, i, j, f, kv, W);
}

// RS_LARGE_WGS workgroups of 4 waves; wave w takes the list entries w, w + waves, ...
__global__ __launch_bounds__(256) void rs_large_kernel(const RsVert *__restrict__ verts, int V, const int *__restrict__ faces, int W, int H,
                                                       unsigned long long *__restrict__ keys, const unsigned long long *__restrict__ list,
                                                       const unsigned *__restrict__ counters, unsigned capacity) {
    const unsigned n = min(counters[0], capacity);
    const unsigned waves = gridDim.x * 4, lane = threadIdx.x & 63;
    for (unsigned e = blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += waves) {
        const unsigned long long ent = list[e];
        const int view = (int)(ent >> 32), f = (int)(ent & 0xffffffffu);
        RsTri t;
        if (rs_load(verts + (size_t)view * V, V, faces, f, W, H, t) != 0) continue;     // cannot happen: it was drawable at set-up
        unsigned long long *kv = keys + (size_t)view * W * H;
        const int bw = t.i1 - t.i0 + 1, total = bw * (t.j1 - t.j0 + 1);
        // (i, j) of box pixel p = lane + 64 k, stepped without a division per pixel: 64 = qs * bw + rs
        const int qs = 64 / bw, rs = 64 % bw;
        int i = (int)lane % bw, j = (int)lane / bw;
        for (int p = lane; p < total; p += 64) {
            rs_emit(t, t.i0 + i, t.j0 + j, f, kv, W);
            i += rs; j += qs;
            if (i >= bw) { i -= bw; ++j; }
        }
    }
}

// grid (ceil(W H / 256), views)
__global__ __launch_bounds__(256) void rs_resolve_kernel(const RsVert *__restrict__ verts, int V, const int *__restrict__ faces, int F,
                                                         const float *__restrict__ vnormals, const float *__restrict__ cams, int W, int H,
                                                         const unsigned long long *__restrict__ keys, float lx, float ly, float lz, float ambient,
                                                         int *__restrict__ o_face, float *__restrict__ o_depth, float *__restrict__ o_bary,
                                                         float *__restrict__ o_normal, unsigned char *__restrict__ o_mask, float *__restrict__ o_shaded) {
    const int p = blockIdx.x * 256 + threadIdx.x, view = blockIdx.y;
    if (p >= W * H) return;
    const size_t q = (size_t)view * W * H + p;
    const unsigned long long key = keys[q];
    int face = -1;
    float depth = INFINITY, c0 = 0.f, c1 = 0.f, c2 = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, shaded = 0.f;
    RsTri t;
    const int f = (int)(key & 0xffffffffu);
    if (key != ~0ULL && f < F && rs_load(verts + (size_t)view * V, V, faces, f, W, H, t) == 0) {
        face = f;
        const float *cam = cams + view * RS_CAM;
        const int ia = faces[(size_t)f * 3], ib = faces[(size_t)f * 3 + 1], ic = faces[(size_t)f * 3 + 2];
        const RsVert *vv = verts + (size_t)view * V;
        const RsVert v0 = vv[ia], v1 = vv[ib], v2 = vv[ic];
        float b0, b1, b2, d;
        rs_pixel(t, p % W, p / W, b0, b1, b2, d);
        if (t.swapped) { const float s = b1; b1 = b2; b2 = s; }          // back to the caller's vertex order
        if (cam[12] != 0.f) {
            c0 = b0; c1 = b1; c2 = b2; depth = d;
        } else {
            const float w0 = __fdiv_rn(b0, v0.z), w1 = __fdiv_rn(b1, v1.z), w2 = __fdiv_rn(b2, v2.z);
            const float s = __fadd_rn(__fadd_rn(w0, w1), w2);
            c0 = __fdiv_rn(w0, s); c1 = __fdiv_rn(w1, s); c2 = __fdiv_rn(w2, s);
            depth = __fdiv_rn(1.f, s);
        }
        float gx, gy, gz;
        if (vnormals) {
            const float *n0 = vnormals + (size_t)ia * 3, *n1 = vnormals + (size_t)ib * 3, *n2 = vnormals + (size_t)ic * 3;
            const float wx = __fadd_rn(__fadd_rn(__fmul_rn(c0, n0[0]), __fmul_rn(c1, n1[0])), __fmul_rn(c2, n2[0]));
            const float wy = __fadd_rn(__fadd_rn(__fmul_rn(c0, n0[1]), __fmul_rn(c1, n1[1])), __fmul_rn(c2, n2[1]));
            const float wz = __fadd_rn(__fadd_rn(__fmul_rn(c0, n0[2]), __fmul_rn(c1, n1[2])), __fmul_rn(c2, n2[2]));
            gx = __fadd_rn(__fadd_rn(__fmul_rn(cam[0], wx), __fmul_rn(cam[1], wy)), __fmul_rn(cam[2], wz));
            gy = __fadd_rn(__fadd_rn(__fmul_rn(cam[4], wx), __fmul_rn(cam[5], wy)), __fmul_rn(cam[6], wz));
            gz = __fadd_rn(__fadd_rn(__fmul_rn(cam[8], wx), __fmul_rn(cam[9], wy)), __fmul_rn(cam[10], wz));
        } else {
            const float e1x = __fsub_rn(v1.x, v0.x), e1y = __fsub_rn(v1.y, v0.y), e1z = __fsub_rn(v1.z, v0.z);
            const float e2x = __fsub_rn(v2.x, v0.x), e2y = __fsub_rn(v2.y, v0.y), e2z = __fsub_rn(v2.z, v0.z);
            gx = __fsub_rn(__fmul_rn(e1y, e2z), __fmul_rn(e1z, e2y));
            gy = __fsub_rn(__fmul_rn(e1z, e2x), __fmul_rn(e1x, e2z));
            gz = __fsub_rn(__fmul_rn(e1x, e2y), __fmul_rn(e1y, e2x));
        }
        // sqrtf, not __fsqrt_rn: HIP's __fsqrt_rn is the native (approximate) v_sqrt_f32, sqrtf is correctly rounded
        const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)), __fmul_rn(gz, gz)));
        if (len > 0.f) {                                       // a zero (or NaN) length leaves the zero normal
            nx = __fdiv_rn(gx, len); ny = __fdiv_rn(gy, len); nz = __fdiv_rn(gz, len);
            if (nz > 0.f) { nx = -nx; ny = -ny; nz = -nz; }
        }
        const float dot = __fadd_rn(__fadd_rn(__fmul_rn(nx, lx), __fmul_rn(ny, ly)), __fmul_rn(nz, lz));
        shaded = __fadd_rn(ambient, __fmul_rn(__fsub_rn(1.f, ambient), fabsf(dot)));
    }
    if (o_face) o_face[q] = face;
    if (o_depth) o_depth[q] = depth;
    if (o_bary) { o_bary[q * 3] = c0; o_bary[q * 3 + 1] = c1; o_bary[q * 3 + 2] = c2; }
    if (o_normal) { o_normal[q * 3] = nx; o_normal[q * 3 + 1] = ny; o_normal[q * 3 + 2] = nz; }
    if (o_mask) o_mask[q] = face >= 0 ? 1 : 0;
    if (o_shaded) o_shaded[q] = shaded;
}

// grid (ceil(W H / 256), views); a neighbour outside the image is background
__global__ __launch_bounds__(256) void rs_contour_kernel(const unsigned char *__restrict__ mask, const float *__restrict__ depth,
                                                         const float *__restrict__ normal, int W, int H, float depth_jump, float cos_crease,
                                                         unsigned char *__restrict__ ink) {
    const int p = blockIdx.x * 256 + threadIdx.x, view = blockIdx.y;
    if (p >= W * H) return;
    const size_t base = (size_t)view * W * H;
    const int i = p % W, j = p / W;
    const bool m = mask[base + p] != 0;
    float dz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    if (m) { dz = depth[base + p]; nx = normal[(base + p) * 3]; ny = normal[(base + p) * 3 + 1]; nz = normal[(base + p) * 3 + 2]; }
    const int di[4] = {-1, 1, 0, 0}, dj[4] = {0, 0, -1, 1};
    bool on = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ii = i + di[k], jj = j + dj[k];
        const bool in = ii >= 0 && ii < W && jj >= 0 && jj < H;
        const size_t qn = base + (size_t)(in ? jj : j) * W + (in ? ii : i);
        const bool mn = in && mask[qn] != 0;
        if (mn != m) on = true;
        if (mn && m) {
            if (fabsf(__fsub_rn(dz, depth[qn])) > depth_jump) on = true;
            const float dot = __fadd_rn(__fadd_rn(__fmul_rn(nx, normal[qn * 3]), __fmul_rn(ny, normal[qn * 3 + 1])), __fmul_rn(nz, normal[qn * 3 + 2]));
            if (dot < cos_crease) on = true;
        }
    }
    ink[base + p] = on ? 1 : 0;
}

}  // namespace surfd

using namespace surfd;

struct surfd_raster {
    int H = 0, W = 0, max_views = 0;
    unsigned long long *keys = nullptr;   // [max_views, H, W]
    unsigned *counters = nullptr;         // [1 + RS_MAX_VIEWS]: list length, dropped per view
    float *cams = nullptr;                // [max_views, RS_CAM]: the call's cameras on the device
    float *cams_pinned = nullptr;         // the same in pinned host memory: the source of the asynchronous copy
    hipEvent_t cams_done = nullptr;       // recorded after that copy; waited for before the pinned buffer is written again
    bool cams_pending = false;
    DeviceArena ws;                       // projected vertices [views, V] and the list of large triangles [views * F]
};

extern "C" {

int surfd_raster_create(int H, int W, int max_views, surfd_raster **out) {
    if (!out) SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_create: null out");
    *out = nullptr;
    if (H < 1 || W < 1 || H > RS_MAX_SIZE || W > RS_MAX_SIZE)
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_create: H = %d, W = %d must lie in [1, %d]", H, W, RS_MAX_SIZE);
    if (max_views < 1 || max_views > RS_MAX_VIEWS)
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_create: max_views = %d must lie in [1, %d]", max_views, RS_MAX_VIEWS);
    surfd_raster *r = new surfd_raster();
    r->H = H; r->W = W; r->max_views = max_views;
    auto fail = [&](hipError_t e) {
        set_error("surfd_raster_create: hipMalloc failed: %s", hipGetErrorString(e));
        (void)hipFree(r->keys); (void)hipFree(r->counters); (void)hipFree(r->cams); (void)hipHostFree(r->cams_pinned);
        if (r->cams_done) (void)hipEventDestroy(r->cams_done);
        delete r;
        return SURFD_ERR_HIP;
    };
    hipError_t e = hipMalloc(&r->keys, (size_t)max_views * H * W * sizeof(unsigned long long));
    if (e != hipSuccess) return fail(e);
    e = hipMalloc(&r->counters, (1 + RS_MAX_VIEWS) * sizeof(unsigned));
    if (e != hipSuccess) return fail(e);
    e = hipMalloc(&r->cams, (size_t)max_views * RS_CAM * sizeof(float));
    if (e != hipSuccess) return fail(e);
    e = hipHostMalloc(&r->cams_pinned, (size_t)max_views * RS_CAM * sizeof(float));
    if (e != hipSuccess) return fail(e);
    e = hipEventCreateWithFlags(&r->cams_done, hipEventDisableTiming);
    if (e != hipSuccess) return fail(e);
    *out = r;
    return SURFD_OK;
}

void surfd_raster_destroy(surfd_raster *r) {
    if (!r) return;
    (void)hipFree(r->keys); (void)hipFree(r->counters); (void)hipFree(r->cams);
    r->ws.release();
    (void)hipHostFree(r->cams_pinned);
    if (r->cams_done) (void)hipEventDestroy(r->cams_done);
    delete r;
}

int surfd_raster_render(surfd_raster *r, const float *vertices, int V, const int32_t *faces, int F, const float *vertex_normals,
                        const float *cameras, int n_views, int flags, const float *light, float ambient,
                        int32_t *face, float *depth, float *bary, float *normal, unsigned char *mask, float *shaded,
                        int32_t *dropped_per_view, surfd_stream s) {
    if (!r) SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_render: null handle");
    if (n_views < 1 || n_views > r->max_views)
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_render: n_views = %d must lie in [1, max_views = %d]", n_views, r->max_views);
    if (V < 0 || F < 0) SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_render: V = %d, F = %d must not be negative", V, F);
    if (!cameras) SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_render: null cameras");
    if ((V > 0 && !vertices) || (F > 0 && !faces)) SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_render: null vertices or faces");
    if (flags & ~(SURFD_RASTER_FORCE_SMALL | SURFD_RASTER_FORCE_LARGE) ||
        (flags & (SURFD_RASTER_FORCE_SMALL | SURFD_RASTER_FORCE_LARGE)) == (SURFD_RASTER_FORCE_SMALL | SURFD_RASTER_FORCE_LARGE))
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_render: flags = %d (FORCE_SMALL and FORCE_LARGE exclude each other)", flags);
    if (!(ambient >= 0.f && ambient <= 1.f)) SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_render: ambient = %g must lie in [0, 1]", (double)ambient);
    for (int v = 0; v < n_views; ++v) {
        const float *c = cameras + v * RS_CAM;
        for (int k = 0; k < RS_CAM; ++k)
            if (!std::isfinite(c[k])) SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_render: camera %d has a NaN or Inf entry", v);
        if (c[12] != 0.f && c[12] != 1.f) SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_render: camera %d: mode must be 0 or 1", v);
        if (c[17] < 0.f || (c[12] == 0.f && !(c[17] > 0.f)))
            SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_render: camera %d: near = %g must be >= 0 (> 0 in perspective mode)", v, (double)c[17]);
    }
    if ((long long)n_views * V > (1LL << 31) - 1 || (long long)n_views * F > (1LL << 31) - 1)
        SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_raster_render: n_views * V and n_views * F must stay below 2^31 (V = %d, F = %d, n_views = %d)", V, F, n_views);
    hipStream_t st = as_stream(s);
    const int W = r->W, H = r->H;
    const size_t vert_bytes = ((size_t)n_views * V * sizeof(RsVert) + 255) / 256 * 256;
    const size_t list_bytes = (size_t)n_views * F * sizeof(unsigned long long);
    if (int rc = r->ws.reserve(vert_bytes + list_bytes, st)) return rc;
    RsVert *verts = reinterpret_cast<RsVert *>(r->ws.ptr);
    unsigned long long *list = reinterpret_cast<unsigned long long *>(static_cast<char *>(r->ws.ptr) + vert_bytes);
    // the caller's cameras are copied into the handle's pinned buffer here, so the caller may free them when the call returns
    if (r->cams_pending) HIP_TRY(hipEventSynchronize(r->cams_done));       // the previous call's copy has read the buffer
    memcpy(r->cams_pinned, cameras, (size_t)n_views * RS_CAM * sizeof(float));
    HIP_TRY(hipMemcpyAsync(r->cams, r->cams_pinned, (size_t)n_views * RS_CAM * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(r->cams_done, st));
    r->cams_pending = true;
    HIP_TRY(hipMemsetAsync(r->keys, 0xFF, (size_t)n_views * W * H * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(r->counters, 0, (1 + RS_MAX_VIEWS) * sizeof(unsigned), st));
    if (F > 0) {                                              // an empty mesh launches no raster kernel
        if (V > 0) {
            hipLaunchKernelGGL(rs_project_kernel, dim3((unsigned)ceil_div<long long>(V, 256), (unsigned)n_views), dim3(256), 0, st, vertices, V, r->cams, verts);
            LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(rs_small_kernel, dim3((unsigned)ceil_div<long long>(F, 256), (unsigned)n_views), dim3(256), 0, st, verts, V, faces, F, W, H, flags,
                           r->keys, list, r->counters);
        LAUNCH_CHECK();
        if (!(flags & SURFD_RASTER_FORCE_SMALL)) {
            const unsigned cap = (unsigned)((long long)n_views * F);
            const unsigned wgs = (unsigned)std::min<long long>(RS_LARGE_WGS, ceil_div<long long>(cap, 4));
            hipLaunchKernelGGL(rs_large_kernel, dim3(wgs), dim3(256), 0, st, verts, V, faces, W, H, r->keys, list, r->counters, cap);
            LAUNCH_CHECK();
        }
    }
    const float lx = light ? light[0] : 0.f, ly = light ? light[1] : 0.f, lz = light ? light[2] : -1.f;
    hipLaunchKernelGGL(rs_resolve_kernel, dim3((unsigned)ceil_div(W * H, 256), (unsigned)n_views), dim3(256), 0, st, verts, V, faces, F, vertex_normals,
                       r->cams, W, H, r->keys, lx, ly, lz, ambient, face, depth, bary, normal, mask, shaded);
    LAUNCH_CHECK();
    if (dropped_per_view)
        HIP_TRY(hipMemcpyAsync(dropped_per_view, r->counters + 1, (size_t)n_views * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return SURFD_OK;
}

int surfd_raster_contours(const surfd_raster *r, const unsigned char *mask, const float *depth, const float *normal, int n_views,
                          float depth_jump, float cos_crease, unsigned char *ink, surfd_stream s) {
    if (!r) SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_contours: null handle");
    if (n_views < 1 || n_views > RS_MAX_VIEWS) SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_contours: n_views = %d must lie in [1, %d]", n_views, RS_MAX_VIEWS);
    if (!mask || !depth || !normal || !ink) SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_contours: null mask, depth, normal or ink");
    if (!(depth_jump >= 0.f) || !(cos_crease >= -1.f && cos_crease <= 1.f))
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_raster_contours: depth_jump = %g must be >= 0 and cos_crease = %g in [-1, 1]", (double)depth_jump, (double)cos_crease);
    hipLaunchKernelGGL(rs_contour_kernel, dim3((unsigned)ceil_div(r->W * r->H, 256), (unsigned)n_views), dim3(256), 0, as_stream(s), mask, depth, normal,
                       r->W, r->H, depth_jump, cos_crease, ink);
    LAUNCH_CHECK();
    return SURFD_OK;
}

}  // extern "C"
