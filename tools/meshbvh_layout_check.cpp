// Stand-alone check of surfd_amd/csrc/meshbvh_layout.h, the index arithmetic of the implicit mesh hierarchy.  Host compiler only,
// meant to be built with -fsanitize=address,undefined (tests/test_meshbvh_cpu.py does) and run on a CPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/meshbvh_layout_check.cpp -o check && ./check
//
// For every leaf count 1 .. 5000 and for counts around W^k up to 2^24 it builds the layout and walks the whole tree with every
// existing child waiting, the way the kernels do with the children whose boxes they cannot skip:
//   * every node index is inside its level and every child index inside the level below (the arrays below have exactly the
//     sizes the device arrays have, so an index outside is a sanitizer report as well);
//   * every leaf is met exactly once, in ascending order;
//   * the walk ends, after exactly nodes + leaves steps, and no tree is deeper than ceil(log_W(nleaf)) (at least one level).
#include "../surfd_amd/csrc/meshbvh_layout.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace surfd;

static int fail(const char *what, long long nleaf, long long a, long long b) {
    std::fprintf(stderr, "meshbvh_layout_check: %s (nleaf = %lld: %lld, %lld)\n", what, nleaf, a, b);
    return 1;
}

static int check(int nleaf) {
    const int F = nleaf * BVH_L - (nleaf % 3);                     // not always a multiple of L
    BvhLayout l;
    if (F < 1 || !bvh_layout(F, &l)) return fail("no layout", nleaf, F, 0);
    if (l.nleaf != nleaf) return fail("leaf count", nleaf, l.nleaf, 0);
    int depth = 1;
    for (long long cap = BVH_W; cap < nleaf; cap *= BVH_W) ++depth;
    if (l.levels != depth || l.levels > BVH_MAX_LEVELS) return fail("depth", nleaf, l.levels, depth);
    if (l.size[l.levels - 1] != 1) return fail("root level size", nleaf, l.size[l.levels - 1], 0);
    long long total = 0;
    for (int k = 0; k < l.levels; ++k) {
        if (l.off[k] != total) return fail("level offset", nleaf, k, l.off[k]);
        total += l.size[k];
    }
    if (total != l.nodes) return fail("node count", nleaf, total, l.nodes);
    std::vector<unsigned char> leaf_seen((size_t)nleaf, 0), node_seen((size_t)l.nodes, 0);
    const int top = l.levels - 1;
    int level = top;
    unsigned node = 0, child = 0;
    unsigned long long mask = bvh_mask_bits(top, (1u << bvh_child_count(bvh_below(l, top), 0)) - 1u);
    node_seen[(size_t)l.off[top]] = 1;
    long long steps = 0, last_leaf = -1;
    const long long bound = (long long)l.nodes + nleaf;
    while (bvh_next(top, level, node, mask, child)) {
        if (++steps > bound) return fail("the walk does not end", nleaf, steps, bound);
        if (level < 0 || level > top) return fail("level outside the tree", nleaf, level, top);
        if ((long long)node >= l.size[level]) return fail("node outside its level", nleaf, level, node);
        const int below = bvh_below(l, level);
        if ((long long)child >= below) return fail("child outside the level below", nleaf, level, child);
        if ((int)(child % BVH_W) >= bvh_child_count(below, (int)node)) return fail("child beyond the valid ones", nleaf, level, child);
        if (level == 0) {
            if ((long long)child <= last_leaf) return fail("leaves out of order", nleaf, child, last_leaf);
            last_leaf = child;
            if (leaf_seen[child]++) return fail("leaf met twice", nleaf, child, 0);
        } else {
            bvh_enter(level, node, child);
            unsigned char &seen = node_seen[(size_t)l.off[level] + node];
            if (seen++) return fail("node met twice", nleaf, level, node);
            mask |= bvh_mask_bits(level, (1u << bvh_child_count(bvh_below(l, level), (int)node)) - 1u);
        }
    }
    if (steps != bound - 1) return fail("steps", nleaf, steps, bound - 1);    // every node but the root, and every leaf
    for (int i = 0; i < nleaf; ++i)
        if (leaf_seen[i] != 1) return fail("leaf not met", nleaf, i, 0);
    for (int i = 0; i < l.nodes; ++i)
        if (node_seen[i] != 1) return fail("node not met", nleaf, i, 0);
    return 0;
}

int main() {
    long long checked = 0;
    for (int n = 1; n <= 5000; ++n, ++checked)
        if (check(n)) return 1;
    for (long long p = BVH_W; p <= (1ll << 24); p *= BVH_W)
        for (long long n : {p - 1, p, p + 1, 2 * p - 1, 2 * p + 1}) {
            if (n < 1 || n > (1ll << 24) + 1) continue;
            if (check((int)n)) return 1;
            ++checked;
        }
    BvhLayout l;
    if (bvh_layout(0, &l) || bvh_layout(-5, &l)) return fail("F < 1 accepted", 0, 0, 0);
    if (!bvh_layout(0x7FFFFFFF, &l) || l.levels > BVH_MAX_LEVELS) return fail("largest F", 0, l.levels, 0);
    std::printf("meshbvh_layout_check: %lld leaf counts, L = %d, W = %d: ok\n", checked, BVH_L, BVH_W);
    return 0;
}
