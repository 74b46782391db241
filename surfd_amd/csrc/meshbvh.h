// The implicit mesh hierarchy shared by raycast.hip and meshdist.hip (built in meshbvh.hip, contract in its header).
#pragma once
#include "common.h"
#include "meshbvh_layout.h"

namespace surfd {

struct MeshBvh {
    bool built = false;
    BvhLayout lay;
    float4 *boxes = nullptr;                 // [lay.nodes][BVH_BOX4]: the children's boxes of every node, level 0 first
    int4 *leaf_tri = nullptr;                // [lay.nleaf]: the handle's triangle indices of a leaf, -1 where it has fewer than L
    int *level_off = nullptr;                // [BVH_MAX_LEVELS] on the device: lay.off
    unsigned long long *visits = nullptr;    // [2] on the device: box tests, pair tests of the last call that counted them
};

// rec: the handle's triangle records, rec4 float4 each.  relative = false: the first three float4 are the vertices a, b, c
// (raycast.hip).  relative = true: they are a, ab, ac (meshdist.hip).  Idempotent; syncs the stream.
int bvh_build(MeshBvh *b, const float4 *rec, int rec4, bool relative, int F, hipStream_t st);
void bvh_free(MeshBvh *b);
int bvh_info(const char *who, const MeshBvh *b, int *levels, int *leaves, int *nodes, int32_t *level_sizes, int capacity);
int bvh_read(const char *who, const MeshBvh *b, float *boxes, int32_t *leaf_triangles, hipStream_t st);
int bvh_visits_reset(const MeshBvh *b, hipStream_t st);
int bvh_visits_read(const char *who, const MeshBvh *b, int64_t *box_tests, int64_t *pair_tests, hipStream_t st);

// the boxes of the W children of one node: component c of each float4 belongs to child c
struct BvhNode {
    float4 lox, loy, loz, hix, hiy, hiz;
};

__device__ __forceinline__ BvhNode bvh_load(const float4 *__restrict__ boxes, int off, unsigned node) {
    const float4 *p = boxes + ((long)off + (long)node) * BVH_BOX4;
    return BvhNode{p[0], p[1], p[2], p[3], p[4], p[5]};
}

__device__ __forceinline__ float bvh_comp(float4 v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w)); }
__device__ __forceinline__ int bvh_comp(int4 v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w)); }

// a child slot that holds nothing is written as lo = +inf, hi = -inf; a box that must never be skipped as lo = -inf, hi = +inf
__device__ __forceinline__ bool bvh_child_exists(float lox, float hix) { return !(lox > hix); }

// the sum of two per-lane counts over the wave, one integer atomic each
__device__ __forceinline__ void bvh_count_visits(unsigned long long *visits, unsigned nbox, unsigned npair, int lane) {
    unsigned long long b = nbox, p = npair;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        b += __shfl_xor(b, o);
        p += __shfl_xor(p, o);
    }
    if (lane == 0) {
        if (b) atomicAdd(visits, b);
        if (p) atomicAdd(visits + 1, p);
    }
}

}  // namespace surfd
