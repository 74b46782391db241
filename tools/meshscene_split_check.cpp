// Prints split_units() of surfd_amd/csrc/meshscene.h as a table: tests/test_meshscene_cpu.py compares it with the four formulas
// the function replaced.  Host code only (hipcc --cuda-host-only, for the HIP headers common.h needs); runs without a GPU.
//   meshscene_split_check BLOCK MAX_SPLITS TARGET  ->  one line "items units S span" per pair
#include "../surfd_amd/csrc/common.h"
#include "../surfd_amd/csrc/meshscene.h"
#include <cstdlib>

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const int block = atoi(argv[1]), max_splits = atoi(argv[2]);
    const long target = atol(argv[3]);
    const long items[] = {1, 63, 64, 255, 256, 257, 4096, 1L << 20, 1L << 28};
    const int units[] = {1, 2, 3, 31, 64, 1000, 65535, 174763};
    for (long i : items)
        for (int u : units) {
            const surfd::Split s = surfd::split_units(i, block, u, max_splits, target);
            printf("%ld %d %d %d\n", i, u, s.S, s.span);
        }
    return 0;
}
