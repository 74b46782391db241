// Stand-alone check of surfd_amd/csrc/scratcharena.h, the arena the calls of meshclean.hip and meshsimplify.hip carve their
// temporaries from.  Host code only (hipcc --cuda-host-only, for the HIP headers common.h needs); runs without a GPU, and
// tests/test_devscratch_cpu.py runs it once more built with -fsanitize=address,undefined.
//   scratcharena_check F V C KEPT LIVE
// For each of the five call sites (the simplification has two stages: C clusters, KEPT kept and LIVE live faces) it allocates a
// host block of exactly the bytes the call site opens its arena with, adopts it, carves the call site's slots in its order and
// writes the first and the last byte of each (a slot that left the block is a sanitizer report).  It prints
//   <site> <slot> <element bytes> <elements> <offset>      per slot
//   <site> total <bytes>
//   <site> refused <return code> <message>                 one more one-element slot, which must not fit
// and fails where the slots do not fill the block exactly or the slot past the end is handed out.
#include "../surfd_amd/csrc/common.h"
#include "../surfd_amd/csrc/scratcharena.h"
#include <cstdlib>
#include <cstring>

using namespace surfd;

static char g_error[512];
void surfd::set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

typedef unsigned long long u64;
struct Slot { const char *name; int elem; long n; };

template <class T>
static int carve(ScratchArena &arena, const Slot &s, char **at) {
    T *p = nullptr;
    const int rc = arena.get(&p, s.n);
    *at = (char *)p;
    return rc;
}

static int site(const char *who, const char *name, size_t total, const std::vector<Slot> &slots) {
    char *block = (char *)malloc(total);
    if (!block) return 1;
    ScratchArena arena(who);
    arena.adopt(block, total);
    size_t end = 0;
    for (const Slot &s : slots) {
        char *at = nullptr;
        const int rc = s.elem == 8 ? carve<u64>(arena, s, &at) : carve<int>(arena, s, &at);
        if (rc != SURFD_OK) { fprintf(stderr, "%s %s: refused inside the block: %s\n", name, s.name, g_error); return 1; }
        const size_t bytes = (size_t)(s.n > 1 ? s.n : 1) * (size_t)s.elem;
        at[0] = 1; at[bytes - 1] = 1;
        printf("%s %s %d %ld %zu\n", name, s.name, s.elem, s.n, (size_t)(at - block));
        end = (size_t)(at - block) + dev_slot<char>((long)bytes);
    }
    printf("%s total %zu\n", name, total);
    if (end != total) { fprintf(stderr, "%s: the slots end at %zu, the block at %zu\n", name, end, total); return 1; }
    int *past = nullptr;
    const int rc = arena.get(&past, 1);
    if (rc != SURFD_ERR_STATE || past) { fprintf(stderr, "%s: a slot past the end was handed out\n", name); return 1; }
    printf("%s refused %d %s\n", name, rc, g_error);
    free(block);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const long F = atol(argv[1]), V = atol(argv[2]), C = atol(argv[3]), kept = atol(argv[4]), live = atol(argv[5]);
    const long H = 3 * F, R = 3 * kept;
    const size_t words = dev_slot<int>(8);
    int bad = 0;
    bad |= site("meshclean", "cull_and_merge", words + 9 * dev_slot<int>(V) + 2 * dev_slot<u64>(V) + 2 * dev_slot<int>(F),
                {{"cnt", 4, 8}, {"nonfinite", 4, V}, {"used", 4, V}, {"idxa", 4, V}, {"idxb", 4, V}, {"headpos", 4, V}, {"hp", 4, V}, {"rep", 4, V},
                 {"survives", 4, V}, {"newidx", 4, V}, {"key", 8, V}, {"key2", 8, V}, {"keep", 4, F}, {"fpos", 4, F}});
    bad |= site("meshclean", "drop_duplicate_faces", words + 4 * dev_slot<int>(F) + dev_slot<unsigned>(F) + 2 * dev_slot<u64>(F),
                {{"cnt", 4, 8}, {"idxa", 4, F}, {"idxb", 4, F}, {"head", 4, F}, {"rank", 4, F}, {"k0", 4, F}, {"k1", 8, F}, {"k1s", 8, F}});
    bad |= site("meshclean", "drop_degenerate_faces", words + 2 * dev_slot<int>(F), {{"cnt", 4, 8}, {"keep", 4, F}, {"pos", 4, F}});
    bad |= site("meshclean", "fill_small_holes", words + 2 * dev_slot<u64>(H) + 2 * dev_slot<int>(H) + 5 * dev_slot<int>(V) + dev_slot<int32_t>(3 * V),
                {{"cnt", 4, 8}, {"key", 8, H}, {"skey", 8, H}, {"eh", 4, H}, {"sh", 4, H}, {"outcnt", 4, V}, {"start", 4, V}, {"capflag", 4, V}, {"nxt", 4, V},
                 {"cpos", 4, V}, {"captri", 4, 3 * V}});
    bad |= site("meshsimplify", "cluster_stage1",
                words + dev_slot<u64>(3) + dev_slot<double>(3) + 8 * dev_slot<int>(V) + 2 * dev_slot<u64>(V) + 4 * dev_slot<int>(F) + dev_slot<int32_t>(3 * F),
                {{"cnt", 4, 8}, {"omin", 8, 3}, {"org", 8, 3}, {"nonfinite", 4, V}, {"used", 4, V}, {"idxa", 4, V}, {"sidx", 4, V}, {"head", 4, V}, {"hpos", 4, V},
                 {"cluster_of", 4, V}, {"cstart", 4, V}, {"key", 8, V}, {"skey", 8, V}, {"keep", 4, F}, {"kpos", 4, F}, {"live", 4, F}, {"lpos", 4, F},
                 {"fbuf", 4, 3 * F}});
    bad |= site("meshsimplify", "cluster_stage2", dev_slot<double>(3 * C) + 3 * dev_slot<int>(C) + dev_slot<int32_t>(3 * live) + 2 * dev_slot<int>(R) + 2 * dev_slot<unsigned>(R),
                {{"rep", 8, 3 * C}, {"named", 4, C}, {"newid", 4, C}, {"rstart", 4, C}, {"dbuf", 4, 3 * live}, {"rval", 4, R}, {"rvals", 4, R}, {"rkey", 4, R},
                 {"rkeys", 4, R}});
    return bad;
}
