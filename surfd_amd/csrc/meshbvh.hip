// An implicit hierarchy of axis-aligned boxes over the triangles of a mesh handle: what lets a ray (raycast.hip, bvr_ kernels)
// or a query point (meshdist.hip, bvm_ kernels) meet O(log F) boxes instead of every tile of the mesh.  Built on the device from
// the triangle records the handle already holds.  The hierarchy only decides WHICH pairs are tested; a pair's result comes from
// rc_pair() / md_pair() as before and the winner is the minimum of a total order on pairs, so the outputs have the bits of the
// brute-force path whatever the tree looks like.
//
// Build (bvh_build), every step a function of the records alone, no atomics, no floating-point sum whose order could vary:
//   vertices   of triangle f: relative = false: the record's a, b, c.  relative = true (meshdist's a, ab, ac): a, fl(a + ab),
//              fl(a + ac).
//   centroid   g = fl(fl(fl(v0 + v1) + v2) * fl(1/3)) per axis, fp32, one rounding per operation.
//   bounds     lo_j, hi_j = min, max of the FINITE centroids' coordinates (bvh_bounds_kernel, one workgroup; min and max are
//              exact, so the order of the reduction does not matter);  ext = max_j fl(hi_j - lo_j).
//   code       per axis q_j = trunc(min(fl(fl(fl(g_j - lo_j) / ext) * 2097151), 2097151)), 21 bits (0 where ext is not > 0);
//              code = the 63-bit Morton interleave, x the lowest bit; a centroid that is not finite gets 2^63 - 1.
//   sort       hipcub::DeviceRadixSort::SortPairs of (code, f) over all 64 bits: stable, so equal codes keep ascending f.
//   leaves     leaf i = the sorted triangles i L .. i L + L - 1; leaf_tri holds their handle indices (-1 past F).
//   boxes      bvh_leaf_kernel: one thread per node of level 0 bounds each of its leaves; bvh_level_kernel, one launch per
//              level bottom-up, bounds a node's child c by the union of the boxes of that child's children.  min / max of fp32
//              values: nothing is rounded.  relative = false: the box of a leaf is the exact min / max of its vertices.
//              relative = true: md_pair() measures to the triangle (a, a + ab, a + ac) in real numbers, which is within
//              u |ab| of the caller's vertex b and within u |fl(a + ab)| of the fl(a + ab) formed here (u = 2^-24), so the
//              coordinates of v1 and v2 enter the box widened by w = 2^-22 (|ab_j| + |v1_j|) + FLT_MIN on both sides: twice what
//              both displacements need, the rounding of v1_j -+ w (<= u |v1_j| <= w / 4) included.  Such a box holds the
//              caller's vertices and the triangle md_pair() sees.
//   never skip a leaf with a vertex coordinate that is a NaN, an Inf or beyond 2^20 in size (where the margins of the two box
//              tests stop holding) gets the box (-inf, +inf)^3, tested explicitly (fminf / fmaxf would drop a NaN); min / max
//              carry it to every node above.  Both box tests never skip such a box.  A child slot that holds nothing (past the
//              end of a level) is (+inf, -inf): bvh_child_exists() is false and the walk never enters it.
//
// Node storage: BVH_BOX4 = 6 float4 per node (lo.x, lo.y, lo.z, hi.x, hi.y, hi.z), component c = child c; level k at
// lay.off[k].  Index arithmetic: meshbvh_layout.h, checked on the CPU by tools/meshbvh_layout_check.cpp.
//
// Bounds: every kernel guards its thread index against the count it is launched for; a leaf reads sorted[i] for i < F only and
// records f = sorted[i] in [0, F) (the sort permutes 0 .. F - 1); a level kernel reads the boxes of children below
// bvh_child_count() only.
#include "meshbvh.h"
#include "devscratch.h"
#include <cfloat>
#include <cmath>

namespace surfd {

constexpr float BVH_TAME = 1048576.f;                        // 2^20
constexpr float BVH_REL_WIDEN = 2.384185791015625e-07f;      // 2^-22
constexpr unsigned long long BVH_CODE_LAST = 0x7FFFFFFFFFFFFFFFull;

struct BvhTri {
    float v[3][3];        // [vertex][axis]
    float w[3][3];        // by how much a coordinate is widened in a box (0 for absolute records)
};

__device__ __forceinline__ BvhTri bvh_triangle(const float4 *__restrict__ rec, int rec4, bool relative, int f) {
    const float4 a = rec[(long)f * rec4], p = rec[(long)f * rec4 + 1], q = rec[(long)f * rec4 + 2];
    BvhTri t;
    t.v[0][0] = a.x; t.v[0][1] = a.y; t.v[0][2] = a.z;
    const float pe[3] = {p.x, p.y, p.z}, qe[3] = {q.x, q.y, q.z};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        t.w[0][j] = 0.f;
        t.v[1][j] = relative ? t.v[0][j] + pe[j] : pe[j];
        t.v[2][j] = relative ? t.v[0][j] + qe[j] : qe[j];
        t.w[1][j] = relative ? fmaf(fabsf(pe[j]) + fabsf(t.v[1][j]), BVH_REL_WIDEN, FLT_MIN) : 0.f;
        t.w[2][j] = relative ? fmaf(fabsf(qe[j]) + fabsf(t.v[2][j]), BVH_REL_WIDEN, FLT_MIN) : 0.f;
    }
    return t;
}

__device__ __forceinline__ void bvh_centroid(const BvhTri &t, float g[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) g[j] = ((t.v[0][j] + t.v[1][j]) + t.v[2][j]) * 0.3333333432674407958984375f;
}

__device__ __forceinline__ bool bvh_finite(float x) { return fabsf(x) < INFINITY; }

// one workgroup of 1024: bb[0..2] = lo, bb[3..5] = hi of the finite centroids (+inf, -inf where there is none)
__global__ __launch_bounds__(1024) void bvh_bounds_kernel(const float4 *__restrict__ rec, int rec4, int relative, int F, float *__restrict__ bb) {
    __shared__ float red[6][1024];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int f = threadIdx.x; f < F; f += 1024) {
        float g[3];
        bvh_centroid(bvh_triangle(rec, rec4, relative, f), g);
        if (bvh_finite(g[0]) && bvh_finite(g[1]) && bvh_finite(g[2])) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { lo[j] = fminf(lo[j], g[j]); hi[j] = fmaxf(hi[j], g[j]); }
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) { red[j][threadIdx.x] = lo[j]; red[3 + j][threadIdx.x] = hi[j]; }
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                red[j][threadIdx.x] = fminf(red[j][threadIdx.x], red[j][threadIdx.x + s]);
                red[3 + j][threadIdx.x] = fmaxf(red[3 + j][threadIdx.x], red[3 + j][threadIdx.x + s]);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) bb[threadIdx.x] = red[threadIdx.x][0];
}

__device__ __forceinline__ unsigned long long bvh_spread21(unsigned long long x) {
    x &= 0x1FFFFFull;
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x001F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

// one thread per triangle
__global__ __launch_bounds__(256) void bvh_codes_kernel(const float4 *__restrict__ rec, int rec4, int relative, int F,
                                                        const float *__restrict__ bb, unsigned long long *__restrict__ code,
                                                        int *__restrict__ index) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    float g[3];
    bvh_centroid(bvh_triangle(rec, rec4, relative, f), g);
    const float ext = fmaxf(bb[3] - bb[0], fmaxf(bb[4] - bb[1], bb[5] - bb[2]));
    unsigned long long c = BVH_CODE_LAST;
    if (bvh_finite(g[0]) && bvh_finite(g[1]) && bvh_finite(g[2])) {
        unsigned long long q[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float x = ext > 0.f ? fminf(__fdiv_rn(g[j] - bb[j], ext) * 2097151.f, 2097151.f) : 0.f;
            q[j] = (unsigned long long)x;
        }
        c = bvh_spread21(q[0]) | (bvh_spread21(q[1]) << 1) | (bvh_spread21(q[2]) << 2);
    }
    code[f] = c;
    index[f] = f;
}

struct BvhBox {
    float lo[3], hi[3];
};

__device__ __forceinline__ void bvh_store(float4 *__restrict__ node, const BvhBox (&b)[BVH_W]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        node[j] = make_float4(b[0].lo[j], b[1].lo[j], b[2].lo[j], b[3].lo[j]);
        node[3 + j] = make_float4(b[0].hi[j], b[1].hi[j], b[2].hi[j], b[3].hi[j]);
    }
}

// one thread per node of level 0: the indices and the boxes of its leaves
__global__ __launch_bounds__(64) void bvh_leaf_kernel(const float4 *__restrict__ rec, int rec4, int relative, int F, int nleaf, int nnode,
                                                      const int *__restrict__ sorted, int4 *__restrict__ leaf_tri, float4 *__restrict__ boxes) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= nnode) return;
    const int valid = bvh_child_count(nleaf, n);
    BvhBox box[BVH_W];
#pragma unroll
    for (int c = 0; c < BVH_W; ++c) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { box[c].lo[j] = INFINITY; box[c].hi[j] = -INFINITY; }
        if (c >= valid) continue;
        const int leaf = n * BVH_W + c;
        int ids[BVH_L];
        bool tame = true;
#pragma unroll
        for (int i = 0; i < BVH_L; ++i) {
            const long s = (long)leaf * BVH_L + i;
            ids[i] = s < F ? sorted[s] : -1;
            if (ids[i] < 0 || ids[i] >= F) { ids[i] = -1; continue; }
            const BvhTri t = bvh_triangle(rec, rec4, relative, ids[i]);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    tame = tame && fabsf(t.v[k][j]) <= BVH_TAME;             // false for a NaN as well
                    box[c].lo[j] = fminf(box[c].lo[j], t.v[k][j] - t.w[k][j]);
                    box[c].hi[j] = fmaxf(box[c].hi[j], t.v[k][j] + t.w[k][j]);
                }
            }
        }
        leaf_tri[leaf] = make_int4(ids[0], ids[1], ids[2], ids[3]);
        if (!tame) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { box[c].lo[j] = -INFINITY; box[c].hi[j] = INFINITY; }
        }
    }
    bvh_store(boxes + (long)n * BVH_BOX4, box);
}

// one thread per node of a level above 0: child c = the union of the boxes that node c of the level below holds
__global__ __launch_bounds__(64) void bvh_level_kernel(const float4 *__restrict__ below, int nbelow, float4 *__restrict__ level, int nnode) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= nnode) return;
    const int valid = bvh_child_count(nbelow, n);
    BvhBox box[BVH_W];
#pragma unroll
    for (int c = 0; c < BVH_W; ++c) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { box[c].lo[j] = INFINITY; box[c].hi[j] = -INFINITY; }
        if (c >= valid) continue;
        const float4 *p = below + ((long)n * BVH_W + c) * BVH_BOX4;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float4 l = p[j], h = p[3 + j];           // an empty slot is (+inf, -inf): the neutral element of both
            box[c].lo[j] = fminf(fminf(l.x, l.y), fminf(l.z, l.w));
            box[c].hi[j] = fmaxf(fmaxf(h.x, h.y), fmaxf(h.z, h.w));
        }
    }
    bvh_store(level + (long)n * BVH_BOX4, box);
}

void bvh_free(MeshBvh *b) {
    (void)hipFree(b->boxes); (void)hipFree(b->leaf_tri); (void)hipFree(b->level_off); (void)hipFree(b->visits);
    b->boxes = nullptr; b->leaf_tri = nullptr; b->level_off = nullptr; b->visits = nullptr;
    b->built = false;
}

int bvh_build(MeshBvh *b, const float4 *rec, int rec4, bool relative, int F, hipStream_t st) {
    if (b->built) return SURFD_OK;
    BvhLayout lay;
    if (!bvh_layout(F, &lay)) SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "mesh hierarchy: F = %d needs more than %d levels", F, BVH_MAX_LEVELS);
    std::unique_ptr<MeshBvh, void (*)(MeshBvh *)> undo(b, bvh_free);      // a refusal frees what was allocated up to it
    HIP_TRY(hipMalloc(&b->boxes, (size_t)lay.nodes * BVH_BOX4 * sizeof(float4)));
    HIP_TRY(hipMalloc(&b->leaf_tri, (size_t)lay.nleaf * sizeof(int4)));
    HIP_TRY(hipMalloc(&b->level_off, BVH_MAX_LEVELS * sizeof(int)));
    HIP_TRY(hipMalloc(&b->visits, 2 * sizeof(unsigned long long)));
    DeviceScratch scratch;
    CubWorkspace cub{&scratch};
    unsigned long long *code_in, *code_out;
    int *idx_in, *idx_out;
    float *bb;
    SURFD_TRY(scratch.get(&code_in, F)); SURFD_TRY(scratch.get(&code_out, F)); SURFD_TRY(scratch.get(&idx_in, F)); SURFD_TRY(scratch.get(&idx_out, F));
    SURFD_TRY(scratch.get(&bb, 6));
    HIP_TRY(hipMemsetAsync(b->visits, 0, 2 * sizeof(unsigned long long), st));
    HIP_TRY(hipMemcpyAsync(b->level_off, lay.off, BVH_MAX_LEVELS * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(bvh_bounds_kernel, dim3(1), dim3(1024), 0, st, rec, rec4, (int)relative, F, bb);
    LAUNCH_CHECK();
    DEV_LAUNCH(bvh_codes_kernel, F, rec, rec4, (int)relative, F, (const float *)bb, code_in, idx_in);      // F >= 1 (bvh_layout)
    SURFD_TRY(cub.sort_pairs(code_in, code_out, idx_in, idx_out, F, 64, st));
    hipLaunchKernelGGL(bvh_leaf_kernel, dim3((unsigned)ceil_div(lay.size[0], 64)), dim3(64), 0, st, rec, rec4, (int)relative, F, lay.nleaf,
                       lay.size[0], (const int *)idx_out, b->leaf_tri, b->boxes);
    LAUNCH_CHECK();
    for (int k = 1; k < lay.levels; ++k) {
        hipLaunchKernelGGL(bvh_level_kernel, dim3((unsigned)ceil_div(lay.size[k], 64)), dim3(64), 0, st,
                           (const float4 *)(b->boxes + (size_t)lay.off[k - 1] * BVH_BOX4), lay.size[k - 1],
                           b->boxes + (size_t)lay.off[k] * BVH_BOX4, lay.size[k]);
        LAUNCH_CHECK();
    }
    HIP_TRY(hipStreamSynchronize(st));                        // the scratch is freed next
    undo.release();
    b->lay = lay;
    b->built = true;
    return SURFD_OK;
}

int bvh_info(const char *who, const MeshBvh *b, int *levels, int *leaves, int *nodes, int32_t *level_sizes, int capacity) {
    if (!b->built) SURFD_FAIL(SURFD_ERR_STATE, "%s: the hierarchy was not built", who);
    if (capacity < 0 || (capacity > 0 && !level_sizes)) SURFD_FAIL(SURFD_ERR_ARG, "%s: level_sizes is null or capacity negative", who);
    if (levels) *levels = b->lay.levels;
    if (leaves) *leaves = b->lay.nleaf;
    if (nodes) *nodes = b->lay.nodes;
    for (int k = 0; k < capacity && k < b->lay.levels; ++k) level_sizes[k] = b->lay.size[k];
    return SURFD_OK;
}

int bvh_read(const char *who, const MeshBvh *b, float *boxes, int32_t *leaf_triangles, hipStream_t st) {
    if (!b->built) SURFD_FAIL(SURFD_ERR_STATE, "%s: the hierarchy was not built", who);
    if (boxes) HIP_TRY(hipMemcpyAsync(boxes, b->boxes, (size_t)b->lay.nodes * BVH_BOX4 * sizeof(float4), hipMemcpyDefault, st));
    if (leaf_triangles) HIP_TRY(hipMemcpyAsync(leaf_triangles, b->leaf_tri, (size_t)b->lay.nleaf * sizeof(int4), hipMemcpyDefault, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SURFD_OK;
}

int bvh_visits_reset(const MeshBvh *b, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(b->visits, 0, 2 * sizeof(unsigned long long), st));
    return SURFD_OK;
}

int bvh_visits_read(const char *who, const MeshBvh *b, int64_t *box_tests, int64_t *pair_tests, hipStream_t st) {
    if (!box_tests || !pair_tests) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    if (!b->built) SURFD_FAIL(SURFD_ERR_STATE, "%s: the hierarchy was not built", who);
    unsigned long long v[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(v, b->visits, sizeof(v), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *box_tests = (int64_t)v[0];
    *pair_tests = (int64_t)v[1];
    return SURFD_OK;
}

}  // namespace surfd
