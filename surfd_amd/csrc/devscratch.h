// Host scaffold of the device-side builds (meshtopo.hip, meshsmooth.hip, meshbvh.hip, meshclean.hip, meshsimplify.hip), included
// after common.h: make keys, radix-sort them with hipcub, scan flags, read a count back, size the result, fill it.  What a kernel
// computes is each file's own; the device pieces two of the files share are in meshedit.h.
//   DeviceScratch  the temporaries of one build.  get() allocates, the destructor frees: THE SCOPE ENDS ONLY AFTER THE STREAM HAS
//                  DRAINED (a build synchronises before it returns; hipFree on an earlier return waits for the device itself).
//   ScratchArena   (scratcharena.h) the temporaries of a call carved from ONE block of its DeviceScratch, dev_slot<T>(n) bytes each;
//                  zeroed_words() carves the counter words of a call and zeroes them on the stream.
//   CubWorkspace   hipcub's temporary storage behind the four operations the builds use: each call asks hipcub for the size, makes
//                  the workspace large enough and runs.  Fed from a DeviceScratch it grows by taking a new block (the old one
//                  is freed with the scope, so nothing in flight loses its buffer).  Without one it is a handle's own: sized by
//                  its first call, fixed from then on (a larger need is SURFD_ERR_STATE), so later calls allocate nothing.
//   dev_bytes, dev_grid, dev_tid, scan_total    sizes of max(n, 1) elements, 256-wide grids, the 64-bit thread index, and the
//                  total of an exclusive sum.  SURFD_TRY passes a SURFD_* refusal on (the callee has set the message).
//   DEV_LAUNCH     a kernel over n items on the stream `st` of the scope: one item per lane, 256 lanes per block, no LDS, then
//                  LAUNCH_CHECK.  Launches of another block size, grid shape or LDS size are written out.
//   read_words     THE host read of a call: a few counter words, then the stream is drained (the scratch may be freed after it).
//   mesh_sizes     the refusal of F < 0, V < 0 and 3 F >= 2^31 that every entry point over faces starts with.
// A build returns from wherever it is refused: besides the scratch it holds the handle it has not finished in a std::unique_ptr
// with the handle's free function, declared before the scratch, and release()s it at the end.
#pragma once
#include <algorithm>
#include <climits>
#include <hipcub/hipcub.hpp>
#include <memory>

#include "scratcharena.h"

#define SURFD_TRY(expr)                                             \
    do {                                                            \
        if (const int _rc = (expr); _rc != SURFD_OK) return _rc;    \
    } while (0)

#define DEV_LAUNCH(kernel, n, ...)                                                             \
    do {                                                                                       \
        hipLaunchKernelGGL(kernel, dim3(dev_grid(n)), dim3(256), 0, st, __VA_ARGS__);          \
        LAUNCH_CHECK();                                                                        \
    } while (0)

namespace surfd {

template <class T>
static inline size_t dev_bytes(long n) { return (size_t)std::max<long>(n, 1) * sizeof(T); }
static inline unsigned dev_grid(long n) { return (unsigned)std::max<long>(1, ceil_div<long>(n, 256)); }
// the thread's index in 64 bits: a grid over close to 2^31 items overflows an int before the guard sees it
__device__ __forceinline__ long dev_tid() { return blockIdx.x * (long)blockDim.x + threadIdx.x; }

// *out = the number of flags set, from the flags and their exclusive sum (static: every code object that includes this has its own)
static __global__ void scan_total_kernel(const int *__restrict__ flag, const int *__restrict__ excl, int n, int *__restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = n > 0 ? excl[n - 1] + flag[n - 1] : 0;
}
static inline int scan_total(const int *flag, const int *excl, int n, int *out, hipStream_t st) {
    hipLaunchKernelGGL(scan_total_kernel, dim3(1), dim3(64), 0, st, flag, excl, n, out);
    LAUNCH_CHECK();
    return SURFD_OK;
}

// the one host read of a call; the scratch may be freed after it
static inline int read_words(const int *dev, int *host, int n, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(host, dev, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SURFD_OK;
}

// too_many: what 3 F >= 2^31 returns (V is an int: below 2^31)
static inline int mesh_sizes(const char *who, int F, int V, int too_many = SURFD_ERR_ARG) {
    if (F < 0 || V < 0) SURFD_FAIL(SURFD_ERR_ARG, "%s: F = %d, V = %d must not be negative", who, F, V);
    if ((long)F * 3 > (long)INT_MAX) SURFD_FAIL(too_many, "%s: 3 F must stay below 2^31, F = %d", who, F);
    return SURFD_OK;
}

class DeviceScratch {
    std::vector<void *> blocks;
  public:
    DeviceScratch() = default;
    DeviceScratch(const DeviceScratch &) = delete;
    DeviceScratch &operator=(const DeviceScratch &) = delete;
    ~DeviceScratch() { for (void *p : blocks) (void)hipFree(p); }

    // max(n, 1) elements; *ptr stays null on failure
    template <class T>
    int get(T **ptr, long n) {
        void *p = *ptr = nullptr;
        HIP_TRY(hipMalloc(&p, dev_bytes<T>(n)));
        blocks.push_back(p);
        *ptr = (T *)p;
        return SURFD_OK;
    }
};

// the counter words of a call, zeroed on the stream
static inline int zeroed_words(ScratchArena &arena, int **words, int n, hipStream_t st) {
    SURFD_TRY(arena.get(words, n));
    HIP_TRY(hipMemsetAsync(*words, 0, (size_t)n * sizeof(int), st));
    return SURFD_OK;
}

struct CubWorkspace {
    DeviceScratch *scratch = nullptr;        // null: the handle's own block (its owner frees ptr)
    char *ptr = nullptr;
    size_t bytes = 0;

    // op(storage, bytes) is one hipcub call: asked for its size first, then run (reserve_only: room is made, nothing runs)
    template <class Op>
    int run(Op op, bool reserve_only = false) {
        size_t need = 0;
        HIP_TRY(op((void *)nullptr, need));
        if (!ptr || need > bytes) {
            if (ptr && !scratch) SURFD_FAIL(SURFD_ERR_STATE, "the hipcub workspace of the handle is too small (%zu > %zu bytes)", need, bytes);
            need = std::max<size_t>(need, 16);
            if (scratch) SURFD_TRY(scratch->get(&ptr, (long)need));
            else HIP_TRY(hipMalloc((void **)&ptr, need));
            bytes = need;
        }
        need = bytes;
        if (!reserve_only) HIP_TRY(op((void *)ptr, need));
        return SURFD_OK;
    }
    // stable, over the key bits [0, end_bit).  reserve_only: for a build whose first sort is not its largest
    template <class K, class V>
    int sort_pairs(const K *kin, K *kout, const V *vin, V *vout, int n, int end_bit, hipStream_t st, bool reserve_only = false) {
        return run([&](void *tmp, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(tmp, b, kin, kout, vin, vout, n, 0, end_bit, st); }, reserve_only);
    }
    int exclusive_sum(const int *in, int *out, int n, hipStream_t st) {
        return run([&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, in, out, n, st); });
    }
    int inclusive_max(const int *in, int *out, int n, hipStream_t st) {
        return run([&](void *tmp, size_t &b) { return hipcub::DeviceScan::InclusiveScan(tmp, b, in, out, hipcub::Max(), n, st); });
    }
    int reduce_sum(const int *in, int *out, int n, hipStream_t st) {
        return run([&](void *tmp, size_t &b) { return hipcub::DeviceReduce::Sum(tmp, b, in, out, n, st); });
    }
};

}  // namespace surfd
