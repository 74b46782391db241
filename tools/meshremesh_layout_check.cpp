// Stand-alone check of surfd_amd/csrc/meshremesh_layout.h, the ONE block a remeshing handle (meshremesh.hip) carves its arrays from,
// with the code the handle itself uses.  Host code only (hipcc --cuda-host-only, for the HIP headers common.h needs); runs without
// a GPU, and tests/test_meshremesh_layout_cpu.py runs it once more built with -fsanitize=address,undefined.
//   meshremesh_layout_check VCAP FCAP
// It allocates a host block of exactly rm_block_bytes(VCAP, FCAP), carves it with rm_carve, fills every array with its own byte
// from its first to its last element (an array that left the block is a sanitizer report), then does what a round does: one
// memset of rm_round_zero_bytes(VCAP) from vborder.  It prints
//   <array> <element bytes> <elements> <offset>      per array, in carving order
//   total <bytes>
//   zeroed <first array> <last array> <bytes>
// and fails where an array does not start on 256 bytes or overlaps the one before, the arrays do not fill the block exactly,
// vborder .. hlast are not RM_ROUND_ZERO adjacent slots in that order, the memset does not end where hlast's slot ends, or any
// byte outside those eight slots changed.
#include "../surfd_amd/csrc/common.h"
#include "../surfd_amd/csrc/scratcharena.h"
#include "../surfd_amd/csrc/meshremesh_layout.h"
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

struct Row { const char *name; char *at; size_t elem; long n; };

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const long V = atol(argv[1]), F = atol(argv[2]), H = 3 * F;
    const size_t total = rm_block_bytes(V, F);
    char *block = (char *)malloc(total);
    if (!block) return 1;
    memset(block, 0x5A, total);
    rm_arrays a;
    if (rm_carve(a, block, V, F) != SURFD_OK) { fprintf(stderr, "refused inside the block: %s\n", g_error); return 1; }
    std::vector<Row> rows;
#define ROW(T, name, n) rows.push_back({#name, (char *)a.name, sizeof(T), (long)(n)});
    RM_ARRAYS(ROW, V, F, H)
#undef ROW
    size_t end = 0;
    int fill = 1;
    for (const Row &r : rows) {
        const size_t at = (size_t)(r.at - block), bytes = (size_t)(r.n > 1 ? r.n : 1) * r.elem;
        if (at != end || at % 256) { fprintf(stderr, "%s starts at %zu, the array before ends at %zu\n", r.name, at, end); return 1; }
        memset(r.at, fill++, bytes);                          // first to last element
        printf("%s %zu %ld %zu\n", r.name, r.elem, r.n, at);
        end = at + dev_slot<char>((long)bytes);
    }
    printf("total %zu\n", total);
    if (end != total) { fprintf(stderr, "the arrays end at %zu, the block at %zu\n", end, total); return 1; }
    // the eight arrays a round zeroes with one memset
    int *const zeroed[RM_ROUND_ZERO] = {a.vborder, a.vheavy, a.vfirst, a.vlast, a.lfirst, a.llast, a.hfirst, a.hlast};
    for (int i = 1; i < RM_ROUND_ZERO; ++i)
        if ((char *)zeroed[i] - (char *)zeroed[i - 1] != (long)dev_slot<int>(V)) { fprintf(stderr, "zeroed array %d is not the slot after array %d\n", i, i - 1); return 1; }
    const size_t z0 = (size_t)((char *)a.vborder - block), z1 = z0 + rm_round_zero_bytes(V);
    if (z1 != (size_t)((char *)a.hlast - block) + dev_slot<int>(V)) { fprintf(stderr, "the memset does not end with hlast's slot\n"); return 1; }
    std::vector<char> before(block, block + total);
    memset(a.vborder, 0, rm_round_zero_bytes(V));
    for (size_t i = 0; i < total; ++i) {
        const bool in = i >= z0 && i < z1;
        if (in ? block[i] != 0 : block[i] != before[i]) { fprintf(stderr, "byte %zu is wrong after the memset\n", i); return 1; }
    }
    printf("zeroed vborder hlast %zu\n", rm_round_zero_bytes(V));
    free(block);
    return 0;
}
