// Device pieces that two or more of the mesh-editing builds use (meshtopo.hip, meshclean.hip, meshsimplify.hip), included after
// devscratch.h.  Every __global__ here is static or a template: a kernel in a header is compiled into every code object that
// includes it.  What merely looks alike stays with its file: the half-edge key packings order their sorts differently, the face
// compactions map through different tables, and a heads test that compares anything but sorted keys is its file's own.
#pragma once
#include "devscratch.h"

namespace surfd {

// 1 where the fp64 vertex v holds a NaN or an Inf (a coordinate is loaded only where those before it are finite)
__device__ __forceinline__ int vertex_nonfinite(const double *__restrict__ vertices, long v) {
    return (isfinite(vertices[3 * v]) && isfinite(vertices[3 * v + 1]) && isfinite(vertices[3 * v + 2])) ? 0 : 1;
}

// The kernel that sees the caller's indices: a face with one outside [0, V) raises *bad and is not looked at further.  keep[f]: no
// vertex of the face is non-finite; used[v]: a kept face names v.
static __global__ void face_mark_kernel(const int32_t *__restrict__ faces, int F, int V, const int *__restrict__ nonfinite, int *__restrict__ keep,
                                        int *__restrict__ used, int *__restrict__ bad) {
    if (dev_tid() >= F) return;
    const long f = dev_tid();
    const int t0 = faces[3 * f], t1 = faces[3 * f + 1], t2 = faces[3 * f + 2];
    if (t0 < 0 || t0 >= V || t1 < 0 || t1 >= V || t2 < 0 || t2 >= V) { *bad = 1; keep[f] = 0; return; }
    const int k = (nonfinite[t0] | nonfinite[t1] | nonfinite[t2]) ? 0 : 1;
    keep[f] = k;
    if (k) { used[t0] = 1; used[t1] = 1; used[t2] = 1; }      // every writer stores the same 1
}

// head[i] = 1 where sorted position i opens a run of equal keys; the key NONE opens none
template <unsigned long long NONE>
__global__ void run_heads_kernel(const unsigned long long *__restrict__ skeys, int n, int *__restrict__ head) {
    if (dev_tid() >= n) return;
    const long i = dev_tid();
    const unsigned long long k = skeys[i];
    head[i] = (k != NONE && (i == 0 || skeys[i - 1] != k)) ? 1 : 0;
}

// idx: the vertices in sorted order; headpos[i]: the position that opens the run of position i.  The sorts are stable over an
// ascending start, so the head of a run is its lowest index.  used (nullable): a vertex outside the mask does not survive.
static __global__ void group_rep_kernel(int V, const int *__restrict__ idx, const int *__restrict__ headpos, const int *__restrict__ used, int *__restrict__ rep,
                                        int *__restrict__ survives) {
    if (dev_tid() >= V) return;
    const int i = (int)dev_tid();
    const int v = idx[i], r = idx[headpos[i]];
    rep[v] = r;
    survives[v] = ((!used || used[v]) && v == r) ? 1 : 0;
}

// heads[i] = i at the head of a run and 0 elsewhere -> rep, survives, newidx (the exclusive sum of survives) and *total survivors.
// hp is scratch of V words.
static inline int group_representatives(CubWorkspace &cub, int V, const int *idx, const int *heads, int *hp, const int *used, int *rep, int *survives,
                                        int *newidx, int *total, hipStream_t st) {
    SURFD_TRY(cub.inclusive_max(heads, hp, V, st));
    DEV_LAUNCH(group_rep_kernel, V, V, idx, (const int *)hp, used, rep, survives);
    SURFD_TRY(cub.exclusive_sum(survives, newidx, V, st));
    return scan_total(survives, newidx, V, total, st);
}

}  // namespace surfd
