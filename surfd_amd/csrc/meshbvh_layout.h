// Index arithmetic of the implicit mesh hierarchy (meshbvh.hip).  Plain C++, no HIP header: the kernels, the host code and the
// stand-alone check tools/meshbvh_layout_check.cpp all include this file, so that every index a kernel forms can be checked
// on a CPU under a sanitizer.
//
// Layout.  The F triangles, sorted by Morton code, are cut into nleaf = ceil(F / L) LEAVES of L consecutive triangles.  Level 0
// has size[0] = ceil(nleaf / W) nodes; node n of level 0 has the leaves n W .. n W + W - 1 (those below nleaf) as children.
// Level k > 0 has size[k] = ceil(size[k - 1] / W) nodes over the nodes of level k - 1 in the same way, up to the level
// top = levels - 1 with one node, the root.  A mesh with one leaf still has one level (a root with one child).  Node n of level k
// is stored at off[k] + n.  There are no pointers: child c of node n is n W + c of the level below, its parent is n / W.
//
// Walk.  A lane's whole state is (level, node, mask): the node it is in and, for every level on the path from the root to that
// node, W bits that say which children of the path's node at that level still wait (bit c of nibble `level`).  bvh_next()
// takes the lowest waiting child of the current node; where none waits it goes up (node / W) until one does, and ends when the
// root has none.  The caller descends with bvh_enter() and ORs the new node's children into the mask with bvh_mask_bits().
// There is no stack: the depth bound is the width of the mask, BVH_MAX_LEVELS * W <= 64 bits.  With W = 4 and L = 4 sixteen
// levels hold 4^16 leaves, more than any int F; bvh_layout() still refuses a deeper tree.  Children are taken in ascending
// order, so a full walk meets the leaves in ascending order, each once.
#pragma once

#if defined(__HIPCC__)
#define BVH_HD __host__ __device__ __forceinline__
#else
#define BVH_HD inline
#endif

namespace surfd {

constexpr int BVH_L = 4;                 // triangles per leaf
constexpr int BVH_W = 4;                 // children per node
constexpr int BVH_MAX_LEVELS = 16;
constexpr int BVH_BOX4 = 6;              // float4 per node: lo.x, lo.y, lo.z, hi.x, hi.y, hi.z of the W children
static_assert(BVH_W == 4, "a nibble of the walk's mask per level, and the float4 / int4 loads of a node");
static_assert(BVH_L == 4, "a leaf is one int4 of triangle indices");
static_assert(BVH_MAX_LEVELS * BVH_W <= 64, "the walk keeps W bits per level in one 64-bit word");

struct BvhLayout {
    int F = 0, nleaf = 0, levels = 0, nodes = 0;
    int size[BVH_MAX_LEVELS] = {};
    int off[BVH_MAX_LEVELS] = {};
};

BVH_HD int bvh_num_leaves(int F) { return (int)(((long long)F + BVH_L - 1) / BVH_L); }

// false where F < 1 or the tree would be deeper than BVH_MAX_LEVELS
inline bool bvh_layout(int F, BvhLayout *out) {
    BvhLayout l;
    if (F < 1) return false;
    l.F = F;
    l.nleaf = bvh_num_leaves(F);
    int below = l.nleaf;
    long long total = 0;
    for (;;) {
        if (l.levels == BVH_MAX_LEVELS) return false;
        const int n = (int)(((long long)below + BVH_W - 1) / BVH_W);
        l.size[l.levels] = n;
        l.off[l.levels] = (int)total;
        total += n;
        ++l.levels;
        if (n == 1) break;
        below = n;
    }
    if (total > 0x7FFFFFFF / BVH_BOX4) return false;
    l.nodes = (int)total;
    *out = l;
    return true;
}

// how many entries the level below `level` has: leaves below level 0, nodes otherwise
inline int bvh_below(const BvhLayout &l, int level) { return level == 0 ? l.nleaf : l.size[level - 1]; }

// the number of children of node `node` that exist, given the size of what lies below its level: W but for the last node
BVH_HD int bvh_child_count(int below, int node) {
    const long long rest = (long long)below - (long long)node * BVH_W;
    return rest >= BVH_W ? BVH_W : (rest > 0 ? (int)rest : 0);
}

BVH_HD unsigned long long bvh_mask_bits(int level, unsigned children) {
    return (unsigned long long)(children & ((1u << BVH_W) - 1u)) << (BVH_W * level);
}

// The next waiting child.  true: `child` is child number (child % W) of node `node` of level `level` (the walk may have gone
// up), i.e. a leaf where level == 0 and a node of level - 1 otherwise; its bit is cleared.  false: the walk is over.
BVH_HD bool bvh_next(int top, int &level, unsigned &node, unsigned long long &mask, unsigned &child) {
    for (;;) {
        const unsigned m = (unsigned)(mask >> (BVH_W * level)) & ((1u << BVH_W) - 1u);
        if (m) {
            const unsigned c = (unsigned)__builtin_ctz(m);
            mask &= ~(1ull << (BVH_W * level + (int)c));
            child = node * BVH_W + c;
            return true;
        }
        if (level >= top) return false;
        ++level;
        node /= BVH_W;
    }
}

// into the child that bvh_next() returned at a level > 0
BVH_HD void bvh_enter(int &level, unsigned &node, unsigned child) {
    --level;
    node = child;
}

}  // namespace surfd
