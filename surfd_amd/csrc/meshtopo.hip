// Combinatorial questions about a triangle mesh, answered on the device from the index array alone: edges with their valences
// and incident half-edges, face neighbours, connected components (by vertex, by edge, by manifold edge), border loops, a
// consistent orientation of every manifold patch, and exact welding of coincident vertices.  Everything here is integer work;
// every output is a function of the input alone: not of the launch geometry, not of the order in which atomics arrive, not of
// the other handles of the process.
//
// Contract (restated sequentially in tests/meshtopo_ref.py):
//   half-edge   h = 3 f + c runs from t[f, c] to t[f, (c + 1) % 3].
//   degenerate  a face with two equal indices: listed in a mask, rows of face_edges / face_neighbors -1, labels -1, flip 0; it
//               takes part in nothing else (it makes no edge, joins nothing, references no vertex).
//   edges       the distinct unordered pairs (lo < hi), ascending in (lo, hi); valence = number of half-edges on it; the
//               half-edges of edge e are edge_halfedges[edge_offsets[e] .. edge_offsets[e + 1]), ascending in h.
//   neighbours  face_neighbors[f, c]: the other face across a valence-2 edge, -1 across a border edge, -2 across valence >= 3.
//   components  "vertex": faces that share a vertex; "edge": an edge of any valence; "manifold": a valence-2 edge.  Labels
//               number the components in ascending order of their lowest face.
//   orientation two faces across a valence-2 edge agree when their half-edges on it run in opposite directions.  flip[f] is the
//               one assignment under which every such edge agrees and the lowest face of every manifold component (patch)
//               keeps its winding; a patch that has none (a Moebius band) is not orientable and its flips are 0.
//   outward     with vertices given: every orientable patch all of whose faces have three valence-2 edges is turned as a whole
//               so that its signed volume (below) is positive; a volume of 0 leaves it.  Patches are treated one by one, no
//               nesting analysis: the shell of a cavity ends up outward too.
//   border loop a connected component of the valence-1 edges under "share a vertex"; numbered in ascending order of the lowest
//               edge; a loop is simple when every vertex it touches lies on exactly two border edges.
//   weld        vertices with equal fp32 coordinates become one (-0 == +0, a vertex that holds a NaN equals nothing); the
//               survivor is the lowest index of its class and survivors keep their relative order.  No tolerance.
//
// Build (mt_create): one 64-bit key lo << 32 | hi per half-edge (all ones for the half-edges of a degenerate face, which sort
// behind every real key), hipcub::DeviceRadixSort::SortPairs of (key, h) over all 64 bits: stable, so the half-edges of an edge
// stay ascending in h.  A head flag per sorted position and its exclusive sum give the edge of every position; E is read back.
//
// One connected-components routine (cc_run) serves every partition.  It works on an explicit list of node pairs, (-1, -1)
// meaning "no pair here":
//   vertex      nodes = vertices; a face joins (v0, v1) and (v1, v2).
//   edge        nodes = faces; sorted positions i - 1 and i of one edge join their faces.   manifold: only where valence == 2.
//   border      nodes = edges; vfirst[v] = the lowest border edge at v (atomicMin: the minimum does not depend on the order);
//               border edge e joins (e, vfirst[lo]) and (e, vfirst[hi]).  vdeg[v] counts the border edges at v (integer adds).
//   orientation nodes = the double cover (f, s) -> 2 f + s.  A valence-2 edge between f and g with relation r (0: the half-edges
//               run in opposite directions, 1: in the same) joins (f, 0)-(g, r) and (f, 1)-(g, 1 - r).  Walking an edge with
//               r = 1 changes the sheet, so (f, 0) and (f, 1) meet exactly when some cycle of the patch has an odd number of
//               disagreeing edges: the patch is not orientable.  Otherwise the cover of a patch splits into two components,
//               each holding one of (g, 0), (g, 1) for every face g; the one with (fmin, 0) has the smallest node 2 fmin, the
//               other 2 fmin + 1.  Roots are smallest nodes (below), so with r0 = root(2 f): flip[f] = r0 & 1, the patch's
//               lowest face is r0 >> 1, and the patch is not orientable where root(2 f) == root(2 f + 1).
//
// cc_run: parent[i] = i; cc_hook_kernel, one thread per pair; cc_compress_kernel, one thread per node.
//   invariant   parent[x] <= x always, a node that stopped being a root never becomes one again, and the parent of a non-root
//               only ever moves to one of its ancestors (fetch_min of two ancestors: the ancestors of x form a chain).
//   hook        find both roots (cc_find halves the path with fetch_min as it goes), order them a > b, and
//               compare-and-swap parent[a] from a to b.  A failed swap means parent[a] had already been lowered by another
//               thread; the thread looks again.  The larger root always goes under the smaller, so the final root of a
//               component is its smallest node: that is what makes the labels canonical without a second pass.
//   progress    no loop waits for another workgroup: there is no spin on a flag, no barrier between workgroups, no lock.
//               Every write lowers one parent entry strictly (a successful swap, a fetch_min that changes its word) and the
//               entries are bounded below by 0, so the number of writes is finite.  cc_find follows strictly decreasing
//               indices.  A hook iteration that does not return has either seen its swap fail, which is paid for by another
//               thread's strict decrease of that very word since this thread read it, or nothing: so every thread's loop
//               ends after finitely many steps whatever the scheduling, even if only one wave ever runs at a time.
//   visibility  inside cc_hook_kernel every access to parent[] is an agent-scope atomic (relaxed load, fetch_min,
//               compare-and-swap): none is served from a CU's L1 or depends on another XCD's L2, so a retry sees the word that
//               made its swap fail.  A stale value would still be an ancestor (safe), but could be re-read for ever.
//   compress    runs after the hooks are complete (kernel boundary): the forest is fixed, every thread chases to the root
//               read-only and stores it; concurrent stores only replace an ancestor by the root.
// Labels: rootface[i] = the lowest face (edge, for loops) of i's component; a node with rootface[i] == i opens a component, the
// exclusive sum of those flags numbers them in ascending order of their lowest member; C is read back.
//
// Signed volume (outward): M = the power of two >= max |coordinate| over the finite coordinates (1 if there is none, or if it
// is 0).  Per face det = (x0 cx + y0 cy) + z0 cz with c = v1 x v2 = (y1 z2 - z1 y2, z1 x2 - x1 z2, x1 y2 - y1 x2), fp64 from the
// fp32 coordinates, every operation rounded once (-ffp-contract=off); turning a face negates det exactly.  The term is
// q = llrint(det * 2^k / M^3), 0 where det is not finite, and the terms are added as 64-bit integers with atomics: integer
// addition is associative, so the sum has no order (a wave whose faces lie in one patch adds its lanes first and issues one
// atomic: the same total).  k and the face limit: by Hadamard |det| <= (sqrt 3 M)^3 < 5.2 M^3, and fp64
// rounding adds less than 2^-48 of that, so |q| < 5.2 * 2^k + 1 < 2^(k + 3).  F faces sum to less than F 2^(k + 3); create
// bounds 3 F < 2^31, so F < 2^30 and the sum stays below 2^(k + 33).  k = 30 keeps it below 2^63 for every mesh the handle
// accepts; a face then resolves 2^-30 M^3 / 6 of volume.
//
// Limits, all return codes: F >= 0 (F = 0 gives empty outputs), V >= 0, 3 F < 2^31 (so 2 F and 3 F fit an int32), every index in
// [0, V) (checked on the device, reported with the first offending face, never a fault).
// Host syncs: mt_create reads E and the counters back once; components and border_loops read their count back once.  Nothing
// else syncs: read and orient only enqueue.  All workspaces are allocated in create, so no later call allocates or frees.
// Bounds: every kernel guards its thread index against the count it is launched for; vertex-indexed arrays are indexed only
// by indices that create validated; edge ids come from the exclusive sum and lie in [0, E); pair nodes lie in [0, n).
#include "common.h"
#include "devscratch.h"
#include "meshedit.h"
#include <climits>
#include <cmath>

namespace surfd {

typedef unsigned long long u64;
constexpr u64 MT_KEY_NONE = ~0ull;
constexpr int MT_VOLUME_K = 30;
enum { MT_CNT_BAD = 0, MT_CNT_FIRST_BAD = 1, MT_CNT_DEGENERATE = 2, MT_CNT_REFERENCED = 3, MT_CNT_E = 4, MT_CNT_WORDS = 8 };

#define MT_LD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// ---- the connected-components routine ------------------------------------------------------------------------------------
__global__ void mt_iota_kernel(int *__restrict__ a, int n) {
    if (dev_tid() < n) a[dev_tid()] = (int)dev_tid();
}

__device__ __forceinline__ int cc_find(int *parent, int x) {
    for (;;) {
        const int p = MT_LD(parent + x);
        if (p == x) return x;
        const int g = MT_LD(parent + p);
        if (g == p) return p;
        (void)__hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // g < p < x
        x = g;
    }
}

__global__ void cc_hook_kernel(int *parent, const int2 *__restrict__ pairs, int n_pairs) {
    if (dev_tid() >= n_pairs) return;
    const int i = (int)dev_tid();
    int a = pairs[i].x, b = pairs[i].y;
    if (a < 0) return;
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        int expected = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
    }
}

__global__ void cc_compress_kernel(int *parent, int n) {
    if (dev_tid() >= n) return;
    const int i = (int)dev_tid();
    int r = i;
    for (;;) {
        const int p = MT_LD(parent + r);
        if (p == r) break;
        r = p;
    }
    __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static int cc_run(int *parent, int n, const int2 *pairs, int n_pairs, hipStream_t st) {
    if (n <= 0) return SURFD_OK;
    DEV_LAUNCH(mt_iota_kernel, n, parent, n);
    if (n_pairs > 0) DEV_LAUNCH(cc_hook_kernel, n_pairs, parent, pairs, n_pairs);
    DEV_LAUNCH(cc_compress_kernel, n, parent, n);
    return SURFD_OK;
}

// ---- edges ---------------------------------------------------------------------------------------------------------------
__global__ void mt_keys_kernel(const int32_t *__restrict__ tri, int F, int V, u64 *__restrict__ keys, int *__restrict__ hidx,
                               unsigned char *__restrict__ degenerate, int *used, int *cnt) {
    if (dev_tid() >= F) return;
    const int f = (int)dev_tid();
    const int t[3] = {tri[3 * (long)f], tri[3 * (long)f + 1], tri[3 * (long)f + 2]};
    const bool bad = t[0] < 0 || t[0] >= V || t[1] < 0 || t[1] >= V || t[2] < 0 || t[2] >= V;
    const bool deg = !bad && (t[0] == t[1] || t[1] == t[2] || t[0] == t[2]);
    degenerate[f] = deg ? 1 : 0;
    if (bad) { atomicAdd(cnt + MT_CNT_BAD, 1); atomicMin(cnt + MT_CNT_FIRST_BAD, f); }
    if (deg) atomicAdd(cnt + MT_CNT_DEGENERATE, 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int a = t[c], b = t[(c + 1) % 3];
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        const long h = 3 * (long)f + c;
        keys[h] = (bad || deg) ? MT_KEY_NONE : ((u64)(unsigned)lo << 32) | (u64)(unsigned)hi;
        hidx[h] = (int)h;
        if (!bad && !deg && atomicExch(used + a, 1) == 0) atomicAdd(cnt + MT_CNT_REFERENCED, 1);
    }
}

__global__ void mt_fill_kernel(const u64 *__restrict__ skeys, const int *__restrict__ shidx, const int *__restrict__ head,
                               const int *__restrict__ excl, int H, int E, int32_t *__restrict__ edges, int32_t *__restrict__ edge_offsets,
                               int32_t *__restrict__ edge_halfedges, int32_t *__restrict__ face_edges) {
    if (dev_tid() >= H) return;
    const int i = (int)dev_tid();
    const int e = excl[i] + head[i] - 1;
    const int h = shidx[i];
    face_edges[h] = e;
    edge_halfedges[i] = h;
    if (head[i]) {
        const u64 k = skeys[i];
        edges[2 * (long)e] = (int32_t)(k >> 32);
        edges[2 * (long)e + 1] = (int32_t)(k & 0xFFFFFFFFull);
        edge_offsets[e] = i;
    }
    if (i == H - 1) edge_offsets[E] = H;
}

__global__ void mt_neighbors_kernel(int H, int E, const int32_t *__restrict__ edge_offsets, const int32_t *__restrict__ edge_halfedges,
                                    const int32_t *__restrict__ face_edges, int32_t *__restrict__ valence, int32_t *__restrict__ face_neighbors) {
    if (dev_tid() >= H) return;
    const int i = (int)dev_tid();
    const int h = edge_halfedges[i];
    const int e = face_edges[h];
    const int s = edge_offsets[e], val = edge_offsets[e + 1] - s;
    if (i == s) valence[e] = val;
    face_neighbors[h] = val == 1 ? -1 : val == 2 ? edge_halfedges[i == s ? s + 1 : s] / 3 : -2;
}

// ---- pair lists ----------------------------------------------------------------------------------------------------------
__global__ void mt_pairs_vertex_kernel(const int32_t *__restrict__ tri, const unsigned char *__restrict__ degenerate, int F, int2 *__restrict__ pairs) {
    if (dev_tid() >= F) return;
    const int f = (int)dev_tid();
    const bool deg = degenerate[f] != 0;
    const int a = tri[3 * (long)f], b = tri[3 * (long)f + 1], c = tri[3 * (long)f + 2];
    pairs[2 * (long)f] = deg ? make_int2(-1, -1) : make_int2(a, b);
    pairs[2 * (long)f + 1] = deg ? make_int2(-1, -1) : make_int2(b, c);
}

__global__ void mt_pairs_faces_kernel(int H, const int32_t *__restrict__ edge_offsets, const int32_t *__restrict__ edge_halfedges,
                                      const int32_t *__restrict__ face_edges, int manifold_only, int2 *__restrict__ pairs) {
    if (dev_tid() >= H) return;
    const int i = (int)dev_tid();
    const int h = edge_halfedges[i];
    const int e = face_edges[h];
    const int s = edge_offsets[e], val = edge_offsets[e + 1] - s;
    pairs[i] = (i == s || (manifold_only && val != 2)) ? make_int2(-1, -1) : make_int2(edge_halfedges[i - 1] / 3, h / 3);
}

__global__ void mt_pairs_orient_kernel(int E, const int32_t *__restrict__ edges, const int32_t *__restrict__ edge_offsets,
                                       const int32_t *__restrict__ edge_halfedges, const int32_t *__restrict__ tri, int2 *__restrict__ pairs) {
    if (dev_tid() >= E) return;
    const int e = (int)dev_tid();
    const int s = edge_offsets[e], val = edge_offsets[e + 1] - s;
    int2 p0 = make_int2(-1, -1), p1 = make_int2(-1, -1);
    if (val == 2) {
        const int h1 = edge_halfedges[s], h2 = edge_halfedges[s + 1];
        const int lo = edges[2 * (long)e];
        const int r = ((tri[h1] == lo) == (tri[h2] == lo)) ? 1 : 0;      // tri[h] is where half-edge h starts
        const int f = h1 / 3, g = h2 / 3;
        p0 = make_int2(2 * f, 2 * g + r);
        p1 = make_int2(2 * f + 1, 2 * g + 1 - r);
    }
    pairs[2 * (long)e] = p0;
    pairs[2 * (long)e + 1] = p1;
}

__global__ void mt_border_vertices_kernel(int E, const int32_t *__restrict__ edges, const int32_t *__restrict__ valence, int *vfirst, int *vdeg) {
    if (dev_tid() >= E || valence[dev_tid()] != 1) return;
    const int e = (int)dev_tid();
    const int lo = edges[2 * (long)e], hi = edges[2 * (long)e + 1];
    atomicMin(vfirst + lo, e); atomicMin(vfirst + hi, e);
    atomicAdd(vdeg + lo, 1); atomicAdd(vdeg + hi, 1);
}

__global__ void mt_pairs_border_kernel(int E, const int32_t *__restrict__ edges, const int32_t *__restrict__ valence, const int *__restrict__ vfirst,
                                       const int *__restrict__ vdeg, int2 *__restrict__ pairs, unsigned char *__restrict__ irregular) {
    if (dev_tid() >= E) return;
    const int e = (int)dev_tid();
    int2 p0 = make_int2(-1, -1), p1 = make_int2(-1, -1);
    unsigned char irr = 0;
    if (valence[e] == 1) {
        const int lo = edges[2 * (long)e], hi = edges[2 * (long)e + 1];
        p0 = make_int2(e, vfirst[lo]);
        p1 = make_int2(e, vfirst[hi]);
        irr = (vdeg[lo] != 2 || vdeg[hi] != 2) ? 1 : 0;
    }
    pairs[2 * (long)e] = p0;
    pairs[2 * (long)e + 1] = p1;
    if (irregular) irregular[e] = irr;
}

// ---- labels --------------------------------------------------------------------------------------------------------------
__global__ void mt_minface_kernel(const int32_t *__restrict__ tri, const unsigned char *__restrict__ degenerate, int F, const int *__restrict__ parent, int *minface) {
    if (dev_tid() >= F || degenerate[dev_tid()]) return;
    const int f = (int)dev_tid();
    int *slot = minface + parent[tri[3 * (long)f]];
    if (f < MT_LD(slot)) atomicMin(slot, f);      // the word only falls, so a face that is not below it cannot be the minimum: one
                                                  // large component would otherwise send every face's atomic to one address
}

__global__ void mt_rootface_vertex_kernel(const int32_t *__restrict__ tri, const unsigned char *__restrict__ degenerate, int F, const int *__restrict__ parent,
                                          const int *__restrict__ minface, int *__restrict__ rootface) {
    if (dev_tid() >= F) return;
    const int f = (int)dev_tid();
    rootface[f] = degenerate[f] ? -1 : minface[parent[tri[3 * (long)f]]];
}

__global__ void mt_rootface_faces_kernel(const unsigned char *__restrict__ degenerate, int F, const int *__restrict__ parent, int *__restrict__ rootface) {
    if (dev_tid() >= F) return;
    const int f = (int)dev_tid();
    rootface[f] = degenerate[f] ? -1 : parent[f];
}

__global__ void mt_rootface_border_kernel(const int32_t *__restrict__ valence, int E, const int *__restrict__ parent, int *__restrict__ rootface) {
    if (dev_tid() >= E) return;
    const int e = (int)dev_tid();
    rootface[e] = valence[e] == 1 ? parent[e] : -1;
}

__global__ void mt_isroot_kernel(const int *__restrict__ rootface, int n, int *__restrict__ isroot) {
    const int i = (int)dev_tid();
    if (dev_tid() < n) isroot[i] = rootface[i] == i ? 1 : 0;
}

__global__ void mt_labels_kernel(const int *__restrict__ rootface, const int *__restrict__ rank, int n, int32_t *__restrict__ labels) {
    if (dev_tid() >= n) return;
    const int i = (int)dev_tid();
    const int r = rootface[i];
    labels[i] = r < 0 ? -1 : rank[r];
}

// ---- orientation ---------------------------------------------------------------------------------------------------------
__global__ void mt_flip_kernel(const unsigned char *__restrict__ degenerate, int F, const int *__restrict__ parent, unsigned char *__restrict__ flip,
                               unsigned char *__restrict__ orientable, int32_t *__restrict__ patch_face) {
    if (dev_tid() >= F) return;
    const int f = (int)dev_tid();
    const int r0 = parent[2 * (long)f], r1 = parent[2 * (long)f + 1];
    const bool deg = degenerate[f] != 0, ok = r0 != r1;
    flip[f] = (!deg && ok) ? (unsigned char)(r0 & 1) : 0;
    orientable[f] = (deg || ok) ? 1 : 0;
    patch_face[f] = deg ? -1 : (r0 >> 1);
}

__global__ void mt_maxabs_kernel(const float *__restrict__ vertices, long n, unsigned *maxbits) {
    const long i = dev_tid();
    if (i >= n) return;
    const float a = fabsf(vertices[i]);
    if (a <= 3.4028234663852886e38f) atomicMax(maxbits, __float_as_uint(a));      // false for a NaN and for +inf; bits of a >= 0 order as a does
}

__global__ void mt_volume_kernel(const int32_t *__restrict__ tri, const float *__restrict__ vertices, int F, const int32_t *__restrict__ face_edges,
                                 const int32_t *__restrict__ valence, const unsigned char *__restrict__ flip, const int32_t *__restrict__ patch_face,
                                 const unsigned *__restrict__ maxbits, u64 *volume, int *open_patch) {
    const int f = (int)dev_tid();                                  // no early return: every lane of a wave takes part in the shuffles
    const int root = dev_tid() < F ? patch_face[f] : -1;
    long long q = 0;
    int open = 0;
    if (root >= 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) open |= valence[face_edges[3 * (long)f + c]] != 2;
        const float m = __uint_as_float(*maxbits);
        int ex = 0;
        double scale = ldexp(1.0, MT_VOLUME_K);
        if (m > 0.f) {
            const double fr = frexp((double)m, &ex);              // m = fr 2^ex, fr in [1/2, 1): M = m where fr == 1/2, else 2^ex
            if (fr == 0.5) ex -= 1;
            scale = ldexp(1.0, MT_VOLUME_K - 3 * ex);
        }
        double v[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 3; ++j) v[c][j] = (double)vertices[3 * (long)tri[3 * (long)f + c] + j];
        const double cx = v[1][1] * v[2][2] - v[1][2] * v[2][1];
        const double cy = v[1][2] * v[2][0] - v[1][0] * v[2][2];
        const double cz = v[1][0] * v[2][1] - v[1][1] * v[2][0];
        double det = (v[0][0] * cx + v[0][1] * cy) + v[0][2] * cz;
        if (flip[f]) det = -det;
        const double scaled = det * scale;
        q = (scaled == scaled && fabs(scaled) < 9.0e18) ? llrint(scaled) : 0ll;
    }
    // a wave whose faces all lie in one patch adds once: integer sums are associative, so the total is the same either way
    int rmax = root;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) rmax = max(rmax, __shfl_xor(rmax, d));
    if (rmax < 0) return;                                          // wave-uniform
    if (__all(root < 0 || root == rmax)) {
        long long sum = q;
        int any_open = open;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { sum += __shfl_xor(sum, d); any_open |= __shfl_xor(any_open, d); }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(volume + rmax, (u64)sum);
            if (any_open) open_patch[rmax] = 1;                   // every writer stores the same 1
        }
    } else if (root >= 0) {
        atomicAdd(volume + root, (u64)q);
        if (open) open_patch[root] = 1;
    }
}

__global__ void mt_turn_kernel(int F, const int32_t *__restrict__ patch_face, const unsigned char *__restrict__ orientable, const u64 *__restrict__ volume,
                               const int *__restrict__ open_patch, unsigned char *__restrict__ flip) {
    if (dev_tid() >= F) return;
    const int f = (int)dev_tid();
    const int root = patch_face[f];
    if (root < 0 || !orientable[f] || open_patch[root]) return;
    if ((long long)volume[root] < 0) flip[f] ^= 1;
}

// ---- weld ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned mt_coord_bits(float x) { return x == 0.f ? 0u : __float_as_uint(x); }      // -0 -> +0

__global__ void mt_weld_key_z_kernel(const float *__restrict__ vertices, int V, unsigned *__restrict__ key, int *__restrict__ idx) {
    if (dev_tid() >= V) return;
    const int i = (int)dev_tid();
    key[i] = mt_coord_bits(vertices[3 * (long)i + 2]);
    idx[i] = i;
}

__global__ void mt_weld_key_xy_kernel(const float *__restrict__ vertices, int V, const int *__restrict__ idx, u64 *__restrict__ key) {
    if (dev_tid() >= V) return;
    const int i = (int)dev_tid();
    const long v = idx[i];
    key[i] = ((u64)mt_coord_bits(vertices[3 * v]) << 32) | (u64)mt_coord_bits(vertices[3 * v + 1]);
}

__global__ void mt_weld_heads_kernel(const float *__restrict__ vertices, int V, const int *__restrict__ idx, int *__restrict__ headpos) {
    if (dev_tid() >= V) return;
    const int i = (int)dev_tid();
    bool same = i > 0;
    if (same) {
        const long a = idx[i], b = idx[i - 1];
#pragma unroll
        for (int j = 0; j < 3; ++j) same = same && vertices[3 * a + j] == vertices[3 * b + j];      // false with a NaN on either side
    }
    headpos[i] = same ? 0 : i;
}

__global__ void mt_weld_map_kernel(int V, const int *__restrict__ rep, const int *__restrict__ survives, const int *__restrict__ newidx,
                                   int32_t *__restrict__ vertex_map, unsigned char *__restrict__ survivor) {
    if (dev_tid() >= V) return;
    const int i = (int)dev_tid();
    vertex_map[i] = newidx[rep[i]];
    survivor[i] = (unsigned char)survives[i];
}

}  // namespace surfd

using namespace surfd;

struct surfd_meshtopo {
    int F = 0, V = 0, E = 0, H = 0;          // H = 3 (F - degenerate): the half-edges that lie on an edge
    int n_degenerate = 0, n_referenced = 0;
    int32_t *tri = nullptr, *edges = nullptr, *valence = nullptr, *edge_offsets = nullptr, *edge_halfedges = nullptr;
    int32_t *face_edges = nullptr, *face_neighbors = nullptr;
    unsigned char *degenerate = nullptr;
    // workspaces of the calls (one stream and one host thread at a time)
    int *parent = nullptr;                   // max(2 F, V, E) nodes
    int2 *pairs = nullptr;                   // max(3 F, 2 E) pairs
    int *rootface = nullptr, *isroot = nullptr, *rank = nullptr;      // max(F, E)
    int *vaux = nullptr;                     // 2 V: vfirst / minface, vdeg
    int32_t *patch_face = nullptr;           // F
    unsigned char *orientable = nullptr;     // F
    u64 *volume = nullptr;                   // F
    int *open_patch = nullptr;               // F
    int *scalars = nullptr;                  // [0] a count, [1] the bits of max |coordinate|
    CubWorkspace scan;                       // the handle's own: sized by create's scan over 3 F >= max(F, E) items, the longest
};

static void mt_free(surfd_meshtopo *m) {
    (void)hipFree(m->tri); (void)hipFree(m->edges); (void)hipFree(m->valence); (void)hipFree(m->edge_offsets); (void)hipFree(m->edge_halfedges);
    (void)hipFree(m->face_edges); (void)hipFree(m->face_neighbors); (void)hipFree(m->degenerate); (void)hipFree(m->parent); (void)hipFree(m->pairs);
    (void)hipFree(m->rootface); (void)hipFree(m->isroot); (void)hipFree(m->rank); (void)hipFree(m->vaux); (void)hipFree(m->patch_face);
    (void)hipFree(m->orientable); (void)hipFree(m->volume); (void)hipFree(m->open_patch); (void)hipFree(m->scalars); (void)hipFree(m->scan.ptr);
    delete m;
}

extern "C" int surfd_meshtopo_create(const int32_t *triangles, int F, int V, surfd_stream s, surfd_meshtopo **out) {
    if (!out) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_create: null argument");
    *out = nullptr;
    SURFD_TRY(mesh_sizes("surfd_meshtopo_create", F, V));
    if (F > 0 && !triangles) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_create: null argument");
    hipStream_t st = as_stream(s);
    std::unique_ptr<surfd_meshtopo, void (*)(surfd_meshtopo *)> owner(new surfd_meshtopo(), mt_free);      // freed on every early return
    surfd_meshtopo *m = owner.get();
    m->F = F; m->V = V;
    const int n3 = 3 * F;
    HIP_TRY(hipMalloc(&m->tri, dev_bytes<int32_t>(n3)));
    HIP_TRY(hipMalloc(&m->degenerate, dev_bytes<unsigned char>(F)));
    HIP_TRY(hipMalloc(&m->face_edges, dev_bytes<int32_t>(n3)));
    HIP_TRY(hipMalloc(&m->face_neighbors, dev_bytes<int32_t>(n3)));
    HIP_TRY(hipMalloc(&m->scalars, 16));
    if (F == 0) {
        HIP_TRY(hipMalloc(&m->edge_offsets, sizeof(int32_t)));
        HIP_TRY(hipMemsetAsync(m->edge_offsets, 0, sizeof(int32_t), st));
        HIP_TRY(hipStreamSynchronize(st));
        *out = owner.release();
        return SURFD_OK;
    }
    DeviceScratch scratch;
    CubWorkspace cub{&scratch};
    u64 *keys, *skeys;
    int *hidx, *shidx, *head, *excl, *used, *cnt;
    SURFD_TRY(scratch.get(&keys, n3)); SURFD_TRY(scratch.get(&skeys, n3)); SURFD_TRY(scratch.get(&hidx, n3)); SURFD_TRY(scratch.get(&shidx, n3));
    SURFD_TRY(scratch.get(&head, n3)); SURFD_TRY(scratch.get(&excl, n3)); SURFD_TRY(scratch.get(&used, V)); SURFD_TRY(scratch.get(&cnt, MT_CNT_WORDS));
    HIP_TRY(hipMemcpyAsync(m->tri, triangles, (size_t)n3 * sizeof(int32_t), hipMemcpyDefault, st));
    HIP_TRY(hipMemsetAsync(used, 0, dev_bytes<int>(V), st));
    const int cnt0[MT_CNT_WORDS] = {0, INT_MAX, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, cnt0, sizeof(cnt0), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(m->face_edges, 0xFF, dev_bytes<int32_t>(n3), st));
    HIP_TRY(hipMemsetAsync(m->face_neighbors, 0xFF, dev_bytes<int32_t>(n3), st));
    DEV_LAUNCH(mt_keys_kernel, F, (const int32_t *)m->tri, F, V, keys, hidx, m->degenerate, used, cnt);
    SURFD_TRY(cub.sort_pairs(keys, skeys, hidx, shidx, n3, 64, st));
    DEV_LAUNCH(run_heads_kernel<MT_KEY_NONE>, n3, (const u64 *)skeys, n3, head);
    SURFD_TRY(m->scan.exclusive_sum(head, excl, n3, st));     // sizes the handle's workspace: every later scan is shorter
    SURFD_TRY(scan_total(head, excl, n3, cnt + MT_CNT_E, st));
    int hc[MT_CNT_WORDS];
    SURFD_TRY(read_words(cnt, hc, MT_CNT_WORDS, st));
    if (hc[MT_CNT_BAD] > 0)
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_create: %d faces name vertices outside [0, %d), the first is face %d", hc[MT_CNT_BAD], V, hc[MT_CNT_FIRST_BAD]);
    m->n_degenerate = hc[MT_CNT_DEGENERATE];
    m->n_referenced = hc[MT_CNT_REFERENCED];
    m->E = hc[MT_CNT_E];
    m->H = 3 * (F - m->n_degenerate);
    const int E = m->E, H = m->H;
    HIP_TRY(hipMalloc(&m->edges, dev_bytes<int32_t>(2L * E)));
    HIP_TRY(hipMalloc(&m->valence, dev_bytes<int32_t>(E)));
    HIP_TRY(hipMalloc(&m->edge_offsets, dev_bytes<int32_t>(E + 1L)));
    HIP_TRY(hipMalloc(&m->edge_halfedges, dev_bytes<int32_t>(H)));
    HIP_TRY(hipMemsetAsync(m->edge_offsets, 0, dev_bytes<int32_t>(E + 1L), st));
    if (H > 0) {
        DEV_LAUNCH(mt_fill_kernel, H, (const u64 *)skeys, (const int *)shidx, (const int *)head, (const int *)excl, H, E, m->edges, m->edge_offsets,
                   m->edge_halfedges, m->face_edges);
        DEV_LAUNCH(mt_neighbors_kernel, H, H, E, (const int32_t *)m->edge_offsets, (const int32_t *)m->edge_halfedges, (const int32_t *)m->face_edges, m->valence,
                   m->face_neighbors);
    }
    const long n_nodes = std::max(std::max(2L * F, (long)V), (long)E), n_pairs = std::max(3L * F, 2L * E), n_fe = std::max(F, E);
    HIP_TRY(hipMalloc(&m->parent, dev_bytes<int>(n_nodes)));
    HIP_TRY(hipMalloc(&m->pairs, dev_bytes<int2>(n_pairs)));
    HIP_TRY(hipMalloc(&m->rootface, dev_bytes<int>(n_fe)));
    HIP_TRY(hipMalloc(&m->isroot, dev_bytes<int>(n_fe)));
    HIP_TRY(hipMalloc(&m->rank, dev_bytes<int>(n_fe)));
    HIP_TRY(hipMalloc(&m->vaux, dev_bytes<int>(2L * V)));
    HIP_TRY(hipMalloc(&m->patch_face, dev_bytes<int32_t>(F)));
    HIP_TRY(hipMalloc(&m->orientable, dev_bytes<unsigned char>(F)));
    HIP_TRY(hipMalloc(&m->volume, dev_bytes<u64>(F)));
    HIP_TRY(hipMalloc(&m->open_patch, dev_bytes<int>(F)));
    HIP_TRY(hipStreamSynchronize(st));                        // the scratch is freed next
    *out = owner.release();
    return SURFD_OK;
}

extern "C" void surfd_meshtopo_destroy(surfd_meshtopo *m) {
    if (m) mt_free(m);
}

extern "C" int surfd_meshtopo_counts(const surfd_meshtopo *m, int64_t *faces, int64_t *edges, int64_t *degenerate, int64_t *referenced) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_counts: null handle");
    if (faces) *faces = m->F;
    if (edges) *edges = m->E;
    if (degenerate) *degenerate = m->n_degenerate;
    if (referenced) *referenced = m->n_referenced;
    return SURFD_OK;
}

extern "C" int surfd_meshtopo_read(const surfd_meshtopo *m, int32_t *edges, int32_t *valence, int32_t *edge_offsets, int32_t *edge_halfedges,
                                   int32_t *face_edges, int32_t *face_neighbors, unsigned char *degenerate, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_read: null handle");
    hipStream_t st = as_stream(s);
    const size_t i4 = sizeof(int32_t);
    if (edges && m->E > 0) HIP_TRY(hipMemcpyAsync(edges, m->edges, 2 * (size_t)m->E * i4, hipMemcpyDeviceToDevice, st));
    if (valence && m->E > 0) HIP_TRY(hipMemcpyAsync(valence, m->valence, (size_t)m->E * i4, hipMemcpyDeviceToDevice, st));
    if (edge_offsets) HIP_TRY(hipMemcpyAsync(edge_offsets, m->edge_offsets, ((size_t)m->E + 1) * i4, hipMemcpyDeviceToDevice, st));
    if (edge_halfedges && m->H > 0) HIP_TRY(hipMemcpyAsync(edge_halfedges, m->edge_halfedges, (size_t)m->H * i4, hipMemcpyDeviceToDevice, st));
    if (face_edges && m->F > 0) HIP_TRY(hipMemcpyAsync(face_edges, m->face_edges, 3 * (size_t)m->F * i4, hipMemcpyDeviceToDevice, st));
    if (face_neighbors && m->F > 0) HIP_TRY(hipMemcpyAsync(face_neighbors, m->face_neighbors, 3 * (size_t)m->F * i4, hipMemcpyDeviceToDevice, st));
    if (degenerate && m->F > 0) HIP_TRY(hipMemcpyAsync(degenerate, m->degenerate, (size_t)m->F, hipMemcpyDeviceToDevice, st));
    return SURFD_OK;
}

// rootface[0 .. n) -> labels and the number of components (read back: the one sync of the call)
static int mt_number(surfd_meshtopo *m, int n, int32_t *labels, int64_t *count, hipStream_t st) {
    DEV_LAUNCH(mt_isroot_kernel, n, (const int *)m->rootface, n, m->isroot);
    SURFD_TRY(m->scan.exclusive_sum(m->isroot, m->rank, n, st));      // allocates nothing: SURFD_ERR_STATE if create's size did not do
    DEV_LAUNCH(mt_labels_kernel, n, (const int *)m->rootface, (const int *)m->rank, n, labels);
    SURFD_TRY(scan_total(m->isroot, m->rank, n, m->scalars, st));
    int c = 0;
    SURFD_TRY(read_words(m->scalars, &c, 1, st));
    *count = c;
    return SURFD_OK;
}

extern "C" int surfd_meshtopo_components(surfd_meshtopo *m, int connectivity, int32_t *labels, int64_t *count, surfd_stream s) {
    if (!m || !count) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_components: null argument");
    if (connectivity != SURFD_MESHTOPO_VERTEX && connectivity != SURFD_MESHTOPO_EDGE && connectivity != SURFD_MESHTOPO_MANIFOLD)
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_components: connectivity %d is none of vertex (0), edge (1), manifold (2)", connectivity);
    *count = 0;
    const int F = m->F, V = m->V, H = m->H;
    if (F == 0) return SURFD_OK;
    if (!labels) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_components: null argument");
    hipStream_t st = as_stream(s);
    int rc;
    if (connectivity == SURFD_MESHTOPO_VERTEX) {
        DEV_LAUNCH(mt_pairs_vertex_kernel, F, (const int32_t *)m->tri, (const unsigned char *)m->degenerate, F, m->pairs);
        if ((rc = cc_run(m->parent, V, m->pairs, 2 * F, st)) != SURFD_OK) return rc;
        HIP_TRY(hipMemsetAsync(m->vaux, 0x7F, dev_bytes<int>(V), st));         // 0x7F7F7F7F: above every face index
        DEV_LAUNCH(mt_minface_kernel, F, (const int32_t *)m->tri, (const unsigned char *)m->degenerate, F, (const int *)m->parent, m->vaux);
        DEV_LAUNCH(mt_rootface_vertex_kernel, F, (const int32_t *)m->tri, (const unsigned char *)m->degenerate, F, (const int *)m->parent, (const int *)m->vaux, m->rootface);
    } else {
        if (H > 0) {
            DEV_LAUNCH(mt_pairs_faces_kernel, H, H, (const int32_t *)m->edge_offsets, (const int32_t *)m->edge_halfedges, (const int32_t *)m->face_edges,
                       connectivity == SURFD_MESHTOPO_MANIFOLD ? 1 : 0, m->pairs);
        }
        if ((rc = cc_run(m->parent, F, m->pairs, H, st)) != SURFD_OK) return rc;
        DEV_LAUNCH(mt_rootface_faces_kernel, F, (const unsigned char *)m->degenerate, F, (const int *)m->parent, m->rootface);
    }
    return mt_number(m, F, labels, count, st);
}

extern "C" int surfd_meshtopo_border_loops(surfd_meshtopo *m, int32_t *labels, unsigned char *irregular, int64_t *count, surfd_stream s) {
    if (!m || !count) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_border_loops: null argument");
    *count = 0;
    const int E = m->E, V = m->V;
    if (E == 0) return SURFD_OK;
    if (!labels) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_border_loops: null argument");
    hipStream_t st = as_stream(s);
    int *vfirst = m->vaux, *vdeg = m->vaux + V;
    HIP_TRY(hipMemsetAsync(vfirst, 0x7F, dev_bytes<int>(V), st));
    HIP_TRY(hipMemsetAsync(vdeg, 0, dev_bytes<int>(V), st));
    DEV_LAUNCH(mt_border_vertices_kernel, E, E, (const int32_t *)m->edges, (const int32_t *)m->valence, vfirst, vdeg);
    DEV_LAUNCH(mt_pairs_border_kernel, E, E, (const int32_t *)m->edges, (const int32_t *)m->valence, (const int *)vfirst, (const int *)vdeg, m->pairs, irregular);
    int rc;
    if ((rc = cc_run(m->parent, E, m->pairs, 2 * E, st)) != SURFD_OK) return rc;
    DEV_LAUNCH(mt_rootface_border_kernel, E, (const int32_t *)m->valence, E, (const int *)m->parent, m->rootface);
    return mt_number(m, E, labels, count, st);
}

extern "C" int surfd_meshtopo_orient(surfd_meshtopo *m, const float *vertices, unsigned char *flip, unsigned char *orientable, int32_t *patch_face,
                                     surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_orient: null handle");
    const int F = m->F, E = m->E;
    if (F == 0) return SURFD_OK;
    if (!flip) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_orient: null argument");
    hipStream_t st = as_stream(s);
    if (E > 0) {
        DEV_LAUNCH(mt_pairs_orient_kernel, E, E, (const int32_t *)m->edges, (const int32_t *)m->edge_offsets, (const int32_t *)m->edge_halfedges,
                   (const int32_t *)m->tri, m->pairs);
    }
    int rc;
    if ((rc = cc_run(m->parent, 2 * F, m->pairs, 2 * E, st)) != SURFD_OK) return rc;
    DEV_LAUNCH(mt_flip_kernel, F, (const unsigned char *)m->degenerate, F, (const int *)m->parent, flip, m->orientable, m->patch_face);
    if (vertices && m->V > 0) {
        unsigned *maxbits = (unsigned *)(m->scalars + 1);
        HIP_TRY(hipMemsetAsync(maxbits, 0, sizeof(unsigned), st));
        HIP_TRY(hipMemsetAsync(m->volume, 0, dev_bytes<u64>(F), st));
        HIP_TRY(hipMemsetAsync(m->open_patch, 0, dev_bytes<int>(F), st));
        DEV_LAUNCH(mt_maxabs_kernel, 3L * m->V, vertices, 3L * m->V, maxbits);
        DEV_LAUNCH(mt_volume_kernel, F, (const int32_t *)m->tri, vertices, F, (const int32_t *)m->face_edges, (const int32_t *)m->valence,
                   (const unsigned char *)flip, (const int32_t *)m->patch_face, (const unsigned *)maxbits, m->volume, m->open_patch);
        DEV_LAUNCH(mt_turn_kernel, F, F, (const int32_t *)m->patch_face, (const unsigned char *)m->orientable, (const u64 *)m->volume, (const int *)m->open_patch, flip);
    }
    if (orientable) HIP_TRY(hipMemcpyAsync(orientable, m->orientable, (size_t)F, hipMemcpyDeviceToDevice, st));
    if (patch_face) HIP_TRY(hipMemcpyAsync(patch_face, m->patch_face, (size_t)F * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return SURFD_OK;
}

extern "C" int surfd_meshtopo_weld(const float *vertices, int V, int32_t *vertex_map, unsigned char *survivor, int64_t *count, surfd_stream s) {
    if (!count) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_weld: null argument");
    *count = 0;
    if (V < 0) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_weld: V = %d must not be negative", V);
    if (V == 0) return SURFD_OK;
    if (!vertices || !vertex_map || !survivor) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_weld: null argument");
    if ((long)V * 3 > (long)INT_MAX) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshtopo_weld: 3 V must stay below 2^31, V = %d", V);
    hipStream_t st = as_stream(s);
    DeviceScratch scratch;
    CubWorkspace cub{&scratch};
    unsigned *kz, *kz2;
    u64 *kxy, *kxy2;
    int *idx0, *idx1, *idx2, *headpos, *hp, *rep, *survives, *newidx, *total;
    SURFD_TRY(scratch.get(&kz, V)); SURFD_TRY(scratch.get(&kz2, V)); SURFD_TRY(scratch.get(&kxy, V)); SURFD_TRY(scratch.get(&kxy2, V));
    SURFD_TRY(scratch.get(&idx0, V)); SURFD_TRY(scratch.get(&idx1, V)); SURFD_TRY(scratch.get(&idx2, V)); SURFD_TRY(scratch.get(&headpos, V));
    SURFD_TRY(scratch.get(&hp, V)); SURFD_TRY(scratch.get(&rep, V)); SURFD_TRY(scratch.get(&survives, V)); SURFD_TRY(scratch.get(&newidx, V));
    SURFD_TRY(scratch.get(&total, 1));
    SURFD_TRY(cub.sort_pairs(kxy, kxy2, idx1, idx2, V, 64, st, true));      // the second sort is the larger: one workspace allocation
    // least significant key first; both sorts are stable, so equal vertices end up adjacent and ascending in index
    DEV_LAUNCH(mt_weld_key_z_kernel, V, vertices, V, kz, idx0);
    SURFD_TRY(cub.sort_pairs(kz, kz2, idx0, idx1, V, 32, st));
    DEV_LAUNCH(mt_weld_key_xy_kernel, V, vertices, V, (const int *)idx1, kxy);
    SURFD_TRY(cub.sort_pairs(kxy, kxy2, idx1, idx2, V, 64, st));
    DEV_LAUNCH(mt_weld_heads_kernel, V, vertices, V, (const int *)idx2, headpos);
    SURFD_TRY(group_representatives(cub, V, idx2, headpos, hp, nullptr, rep, survives, newidx, total, st));      // every vertex takes part
    DEV_LAUNCH(mt_weld_map_kernel, V, V, (const int *)rep, (const int *)survives, (const int *)newidx, vertex_map, survivor);
    int c = 0;
    SURFD_TRY(read_words(total, &c, 1, st));                  // the scratch is freed next
    *count = c;
    return SURFD_OK;
}
