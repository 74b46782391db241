// The arrays of a remeshing handle (meshremesh.hip) and how they are carved from its ONE block, included after common.h and
// scratcharena.h.  Plain C++, no HIP call: the stand-alone check tools/meshremesh_layout_check.cpp carves a host block with the
// same code, under the sanitizers.  ONE list names every array with its element type and its length in terms of the capacities
// V (vertex slots), F (faces) and H = 3 F (corners; edges are at most as many): the struct, the size of the block and the carving
// are all made from it, so they cannot disagree.
//   rm_block_bytes(V, F)   the bytes of the block: the sum of the slots.
//   rm_carve(a, block, V, F)   the arrays in the order of the list; SURFD_ERR_STATE if the block were too small.
//   rm_round_zero_bytes(V)     vborder .. hlast are RM_ROUND_ZERO consecutive slots of V ints: a round zeroes them with one memset
//                              from vborder (the check asserts the eight are adjacent, in this order, and that the memset ends
//                              where hlast's slot ends).
#pragma once
#include <cstddef>
#include <cstdint>

namespace surfd {

typedef unsigned long long rm_u64;
enum { RM_WORDS = 32, RM_ROUND_ZERO = 8 };

// DO(type, name, elements)
#define RM_ARRAYS(DO, V, F, H)                                                                                                       \
    DO(int, cnt, RM_WORDS)                                                                                                            \
    DO(int, origin, V) DO(int, mbest, V) DO(int, Mbest, V) DO(int, stays, V) DO(int, newid, V) DO(int, rename, V)                          \
    DO(int, vborder, V) DO(int, vheavy, V) DO(int, vfirst, V) DO(int, vlast, V) DO(int, lfirst, V) DO(int, llast, V) DO(int, hfirst, V)     \
    DO(int, hlast, V)                                                                                                                 \
    DO(rm_u64, vmin, V) DO(double, X, 3 * (V)) DO(double, X2, 3 * (V))                                                                  \
    DO(int, live, F) DO(int, lpos, F)                                                                                                  \
    DO(int, iota, H) DO(int, sh, H) DO(int, head, H) DO(int, hpos, H) DO(int, eoh, H) DO(int, vf, H) DO(int, elo, H) DO(int, ehi, H)         \
    DO(int, eval, H) DO(int, hie, H) DO(int, cand, H) DO(int, sel, H) DO(int, selpos, H) DO(int, estart, (H) + 1)                          \
    DO(unsigned, vkey, H) DO(unsigned, vkeys, H)                                                                                       \
    DO(rm_u64, hkey, H) DO(rm_u64, hkeys, H) DO(rm_u64, ehash, H)                                                                       \
    DO(double, nra, H) DO(double, nrb, H)                                                                                              \
    DO(int32_t, fa, H) DO(int32_t, fb, H)

struct rm_arrays {
#define RM_MEMBER(T, name, n) T *name = nullptr;
    RM_ARRAYS(RM_MEMBER, 0, 0, 0)
#undef RM_MEMBER
};

static inline size_t rm_block_bytes(long V, long F) {
    const long H = 3 * F;
    size_t total = 0;
#define RM_SIZE(T, name, n) total += dev_slot<T>(n);
    RM_ARRAYS(RM_SIZE, V, F, H)
#undef RM_SIZE
    return total;
}

static inline size_t rm_round_zero_bytes(long V) { return RM_ROUND_ZERO * dev_slot<int>(V); }

static inline int rm_carve(rm_arrays &a, void *block, long V, long F) {
    const long H = 3 * F;
    ScratchArena arena("meshremesh");
    arena.adopt(block, rm_block_bytes(V, F));
#define RM_GET(T, name, n) \
    if (const int rc = arena.get(&a.name, n); rc != SURFD_OK) return rc;
    RM_ARRAYS(RM_GET, V, F, H)
#undef RM_GET
    return SURFD_OK;
}

}  // namespace surfd
