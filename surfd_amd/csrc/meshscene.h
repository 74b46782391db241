// Host scaffold of the mesh handles (raycast.hip, meshdist.hip, meshintersect.hip, winding.hip, raster.hip), included after
// common.h.  Host code only: what a kernel computes, and with it every result, is each file's own.  The handles' grow-only
// workspace, DeviceArena, is in common.h: the network handles use it too.
//   split_units    how many workgroups share a call's triangle range, so that a small call still fills the chip.
//   CreateFlags    the flag words a create's kernels raise; mesh_create_args / mesh_bad_index: the refusals every create makes.
//   read_counter   a device counter and the host total that goes with it (the *_skipped entry points).
#pragma once
#include <algorithm>
#include <climits>

namespace surfd {

// `units` (chunks, groups) are shared by S workgroups per block of `block` items (rays, queries, triangles), `span` whole units
// each: about `target` workgroups over the chip (2048 = 8 per CU), at most max_splits (the kernel's grid.y).  target = 1: S = 1.
struct Split {
    int S, span;
};

static inline Split split_units(long items, int block, int units, int max_splits, long target = 2048) {
    long s = std::max<long>(1, ceil_div<long>(target, ceil_div<long>(items, block)));
    s = std::min<long>({s, (long)max_splits, (long)units});
    const int span = (int)ceil_div<long>(units, s);
    return {ceil_div(units, span), span};
}

// n ints on the device, zero from init() on; a create's kernels add to them or set them, read() brings them back once the
// stream has drained.  Freed with the scope.
struct CreateFlags {
    int *dev = nullptr;
    const int n;

    explicit CreateFlags(int count) : n(count) {}
    CreateFlags(const CreateFlags &) = delete;
    ~CreateFlags() { (void)hipFree(dev); }

    int init(hipStream_t st) {
        HIP_TRY(hipMalloc(&dev, n * sizeof(int)));
        HIP_TRY(hipMemsetAsync(dev, 0, n * sizeof(int), st));
        return SURFD_OK;
    }
    int read(int *host, hipStream_t st) {
        HIP_TRY(hipMemcpyAsync(host, dev, n * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return SURFD_OK;
    }
};

// what every create refuses before it allocates; *out is null from here on.  max_F: the largest F the caller's 32-bit indices hold
// (INT_MAX where the caller has a test of its own).
template <class Handle>
static inline int mesh_create_args(const char *who, const float *vertices, int V, const int32_t *triangles, int F, Handle **out, int max_F) {
    if (!out) SURFD_FAIL(SURFD_ERR_ARG, "%s: null out", who);
    *out = nullptr;
    if (!vertices || !triangles) SURFD_FAIL(SURFD_ERR_ARG, "%s: null vertices or triangles", who);
    if (V < 1 || F < 1) SURFD_FAIL(SURFD_ERR_ARG, "%s: V = %d, F = %d must be positive", who, V, F);
    if (F > max_F) SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "%s: F = %d is beyond the supported size", who, F);
    return SURFD_OK;
}

// the refusal behind a gather kernel's flag
static inline int mesh_bad_index(const char *who, int V) {
    SURFD_FAIL(SURFD_ERR_ARG, "%s: a triangle names a vertex outside [0, %d)", who, V);
}

// syncs the stream
static inline int read_counter(const unsigned long long *dev, long long host_total, int64_t *value, int64_t *total, hipStream_t st) {
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, dev, sizeof(v), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *value = (int64_t)v;
    *total = (int64_t)host_total;
    return SURFD_OK;
}

}  // namespace surfd
