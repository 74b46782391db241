// The scaffold of ROUNDS OF INDEPENDENT EDGE OPERATIONS, which the edge-collapse decimation (meshdecimate.hip) and the isotropic
// remeshing (meshremesh.hip) share, included after meshedit.h by those two and by nothing else: the integer mix of the priorities,
// the normal and the side test of rule (e), the structure of a round (edges, corners and rings of every vertex, as keys, stable
// sorts and run bounds), the rules (a) (b) (c) (d) and (e) of a collapse, the selection by least priority over a vertex's ring
// (meshdecimate.hip, step 5, has the argument), the renaming and compaction of the faces, and the naming of the output.  Every
// __global__ here is static: a kernel in a header is compiled into every code object that includes it.  As in meshedit.h, what
// merely looks alike stays with its file: the placement, rule (n) and the cost key are the decimation's, the length gate, the
// collapse point and rule (f) the remeshing's, and each file keeps its own select and apply kernels and its output of vertices.
#pragma once
#include "meshedit.h"

namespace surfd {

typedef unsigned long long er_u64;

// splitmix64's finaliser
__host__ __device__ __forceinline__ er_u64 er_fin(er_u64 x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
// the salt of a round, made on the host; mix64(seed, round, lo, hi) = er_mix(er_salt(seed, round), lo, hi)
static inline er_u64 er_salt(uint64_t seed, uint64_t round) { return er_fin(seed + 0x9e3779b97f4a7c15ull * (er_u64)(round + 1)); }
__device__ __forceinline__ er_u64 er_mix(er_u64 salt, int lo, int hi) { return er_fin(salt ^ (((er_u64)(unsigned)lo << 32) | (er_u64)(unsigned)hi)); }

// the normal of a face
struct er_v3 { double x, y, z; };
__device__ __forceinline__ er_v3 er_load(const double *__restrict__ P, long v) { return {P[3 * v], P[3 * v + 1], P[3 * v + 2]}; }
__device__ __forceinline__ er_v3 er_normal(const er_v3 &q0, const er_v3 &q1, const er_v3 &q2) {
    const double ax = q1.x - q0.x, ay = q1.y - q0.y, az = q1.z - q0.z, bx = q2.x - q0.x, by = q2.y - q0.y, bz = q2.z - q0.z;
    return {ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx};
}
__device__ __forceinline__ double er_dot(const er_v3 &a, const er_v3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// the two comparisons of rule (e): does the new normal w keep the side of n?
__device__ __forceinline__ bool er_keeps(const er_v3 &n, const er_v3 &w, double ww, double flip2) {
    const double g = er_dot(n, w);
    return g > 0.0 && g * g > flip2 * (er_dot(n, n) * ww);
}
// does moving corner k of the face t to p keep its side, against its standing normal and against n0?  (rule (e))
__device__ __forceinline__ bool er_keeps_side(const double *__restrict__ P, const int t[3], int k, const er_v3 &p, const er_v3 &n0, double flip2) {
    const er_v3 q0 = er_load(P, t[0]), q1 = er_load(P, t[1]), q2 = er_load(P, t[2]);
    const er_v3 n = er_normal(q0, q1, q2);
    const er_v3 w = er_normal(k == 0 ? p : q0, k == 1 ? p : q1, k == 2 ? p : q2);
    const double ww = er_dot(w, w);
    return er_keeps(n, w, ww, flip2) && er_keeps(n0, w, ww, flip2);
}

// the ascending neighbours and incident edges of a vertex: the edges that name it as hi (lower neighbours), then those that name
// it as lo, a run of the edge list itself
struct er_ring {
    const int *elo, *ehi, *hie;
    int h0, nh, l0, n;
    __device__ __forceinline__ int edge(int j) const { return j < nh ? hie[h0 + j] : l0 + (j - nh); }
    __device__ __forceinline__ int other(int j) const { return j < nh ? elo[hie[h0 + j]] : ehi[l0 + (j - nh)]; }
};
struct er_rings {
    const int *elo, *ehi, *hie, *hfirst, *hlast, *lfirst, *llast;
    __device__ __forceinline__ er_ring at(long v) const {
        const int h0 = hfirst[v], nh = hlast[v] - h0, l0 = lfirst[v], nl = llast[v] - l0;
        return {elo, ehi, hie, h0, nh, l0, nh + nl};
    }
    __device__ __forceinline__ int degree(long v) const { return (hlast[v] - hfirst[v]) + (llast[v] - lfirst[v]); }
};

__device__ __forceinline__ bool er_before(const er_u64 *__restrict__ ehash, int a, int b) {      // b may be -1: nothing yet
    return b < 0 || ehash[a] < ehash[b] || (ehash[a] == ehash[b] && a < b);
}

// ---- the rules of a collapse that both files ask ------------------------------------------------------------------------------------
// The first of the rules (a) (b) (c) (d) that refuses the collapse of edge e = (lo, hi) of valence val, as 0..3, or -1:
// (a) valence 1 or 2;  (b) |N(lo) & N(hi)| == valence;  (c) not (valence 2 and lo and hi both border vertices);
// (d) every opposite vertex o: deg(o) >= 4, or >= 3 at a border vertex.
__device__ __forceinline__ int er_refused_abcd(const er_rings &rings, const int32_t *__restrict__ fa, const int *__restrict__ estart, const int *__restrict__ sh,
                                               const int *__restrict__ vborder, long e, int lo, int hi, int val) {
    int refused = -1;
    if (val != 1 && val != 2) refused = 0;
    if (refused < 0) {
        const er_ring a = rings.at(lo), b = rings.at(hi);
        int i = 0, j = 0, common = 0;
        while (i < a.n && j < b.n) {                          // at most a.n + b.n steps
            const int x = a.other(i), y = b.other(j);
            if (x == y) { ++common; ++i; ++j; }
            else if (x < y) ++i;
            else ++j;
        }
        if (common != val) refused = 1;
    }
    if (refused < 0 && val == 2 && vborder[lo] && vborder[hi]) refused = 2;
    if (refused < 0) {
        for (int i = estart[e]; i < estart[e + 1]; ++i) {     // val <= 2 half-edges
            const long h = sh[i], f = h / 3;
            const int o = fa[3 * f + ((int)(h - 3 * f) + 2) % 3];
            if (rings.degree(o) < (vborder[o] ? 3 : 4)) refused = 3;
        }
    }
    return refused;
}

// rule (e) over both fans: every face at lo or at hi that does not hold both keeps its side with its moved corner at p
__device__ __forceinline__ bool er_fans_keep_side(const double *__restrict__ P, const int32_t *__restrict__ fa, const int *__restrict__ vfirst,
                                                  const int *__restrict__ vlast, const int *__restrict__ vf, const double *__restrict__ nref, int lo, int hi,
                                                  const er_v3 &p, double flip2) {
    bool keeps = true;
#pragma unroll 1
    for (int side = 0; side < 2 && keeps; ++side) {
        const int end = side ? hi : lo, other = side ? lo : hi;
        for (int i = vfirst[end]; i < vlast[end]; ++i) {
            const long h = vf[i], f = h / 3;
            const int t[3] = {fa[3 * f], fa[3 * f + 1], fa[3 * f + 2]};
            if (t[0] == other || t[1] == other || t[2] == other) continue;
            if (!er_keeps_side(P, t, (int)(h - 3 * f), p, {nref[3 * f], nref[3 * f + 1], nref[3 * f + 2]}, flip2)) { keeps = false; break; }
        }
    }
    return keeps;
}

// ---- kept faces ---------------------------------------------------------------------------------------------------------------------
// The kernel that sees the caller's indices: a face with one outside [0, V) raises *bad and is not looked at further.  keep[f]: no
// vertex of the face is non-finite and none is named twice; part[v] (nullable): a kept face names v.
static __global__ void er_face_mark_kernel(const int32_t *__restrict__ faces, int F, int V, const int *__restrict__ nonfinite, int *__restrict__ keep,
                                           int *__restrict__ part, int *__restrict__ bad) {
    if (dev_tid() >= F) return;
    const long f = dev_tid();
    const int t0 = faces[3 * f], t1 = faces[3 * f + 1], t2 = faces[3 * f + 2];
    if (t0 < 0 || t0 >= V || t1 < 0 || t1 >= V || t2 < 0 || t2 >= V) { *bad = 1; keep[f] = 0; return; }
    const int k = (nonfinite[t0] | nonfinite[t1] | nonfinite[t2] || t0 == t1 || t1 == t2 || t0 == t2) ? 0 : 1;
    keep[f] = k;
    if (part && k) { part[t0] = 1; part[t1] = 1; part[t2] = 1; }      // every writer stores the same 1
}

static __global__ void er_compact_kept_kernel(const int32_t *__restrict__ faces, int F, const int *__restrict__ keep, const int *__restrict__ kpos,
                                              int32_t *__restrict__ out) {
    if (dev_tid() >= F || !keep[dev_tid()]) return;
    const long f = dev_tid(), n = kpos[f];                     // n <= f
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * n + c] = faces[3 * f + c];
}

// n0 of every kept face
static __global__ void er_face_normals_kernel(const double *__restrict__ P, const int32_t *__restrict__ fa, int F, double *__restrict__ nref) {
    if (dev_tid() >= F) return;
    const long f = dev_tid();
    const er_v3 n = er_normal(er_load(P, fa[3 * f]), er_load(P, fa[3 * f + 1]), er_load(P, fa[3 * f + 2]));
    nref[3 * f] = n.x; nref[3 * f + 1] = n.y; nref[3 * f + 2] = n.z;
}

static __global__ void er_iota_kernel(int *__restrict__ iota, long n) {
    if (dev_tid() < n) iota[dev_tid()] = (int)dev_tid();
}

// the kept faces of the caller's F faces, in their order, into fa; *kept their number, *bad set by an index outside [0, V).  The
// caller reads both words and refuses the bad index.
static inline int er_kept_faces(CubWorkspace &cub, const int32_t *faces, int F, int V, const int *nonfinite, int *keep, int *kpos, int *part, int *bad,
                                int *kept, int32_t *fa, hipStream_t st) {
    DEV_LAUNCH(er_face_mark_kernel, F, faces, F, V, nonfinite, keep, part, bad);
    SURFD_TRY(cub.exclusive_sum(keep, kpos, F, st));
    SURFD_TRY(scan_total(keep, kpos, F, kept, st));
    DEV_LAUNCH(er_compact_kept_kernel, F, faces, F, (const int *)keep, (const int *)kpos, fa);
    return SURFD_OK;
}

// ---- the structure of a round ---------------------------------------------------------------------------------------------------------
// one lane per corner h = 3 f + k: the key of its half-edge and the vertex it names
static __global__ void er_half_keys_kernel(const int32_t *__restrict__ fa, long n, er_u64 *__restrict__ hkey, unsigned *__restrict__ vkey) {
    if (dev_tid() >= n) return;
    const long h = dev_tid(), f = h / 3;
    const int k = (int)(h - 3 * f);
    const int a = fa[h], b = fa[3 * f + (k + 1) % 3];
    hkey[h] = ((er_u64)(unsigned)(a < b ? a : b) << 32) | (er_u64)(unsigned)(a < b ? b : a);
    vkey[h] = (unsigned)a;
}

// sorted position i -> the edge of its half-edge; at the head of a run the edge's start and names; the last lane closes the starts
static __global__ void er_edge_fill_kernel(const er_u64 *__restrict__ skey, const int *__restrict__ sh, const int *__restrict__ head, const int *__restrict__ hpos,
                                           long n, int *__restrict__ eoh, int *__restrict__ estart, int *__restrict__ elo, int *__restrict__ ehi) {
    if (dev_tid() >= n) return;
    const long i = dev_tid();
    const int e = hpos[i] + head[i] - 1;
    eoh[sh[i]] = e;
    if (head[i]) { estart[e] = (int)i; elo[e] = (int)(skey[i] >> 32); ehi[e] = (int)(skey[i] & 0xffffffffull); }
    if (i == n - 1) estart[e + 1] = (int)n;                   // e + 1 <= n: estart has one entry more than there are corners
}

// first[k], last[k]: the run of the key k in the sorted keys (both preset to 0: an empty run)
static __global__ void er_run_bounds_kernel(const unsigned *__restrict__ skey, long n, int *__restrict__ first, int *__restrict__ last) {
    if (dev_tid() >= n) return;
    const long i = dev_tid();
    const unsigned k = skey[i];
    if (i == 0 || skey[i - 1] != k) first[k] = (int)i;
    if (i == n - 1 || skey[i + 1] != k) last[k] = (int)(i + 1);
}

// the valence of every edge, the key of its hi end, the border vertices and (vheavy nullable) the vertices at an edge of valence >= 3
static __global__ void er_edge_info_kernel(const int *__restrict__ estart, const int *__restrict__ elo, const int *__restrict__ ehi, int E, int *__restrict__ eval,
                                           int *__restrict__ vborder, int *__restrict__ vheavy, unsigned *__restrict__ hikey) {
    if (dev_tid() >= E) return;
    const long e = dev_tid();
    const int val = estart[e + 1] - estart[e];
    eval[e] = val;
    hikey[e] = (unsigned)ehi[e];
    if (val == 1) { vborder[elo[e]] = 1; vborder[ehi[e]] = 1; }      // every writer stores the same 1
    if (vheavy && val >= 3) { vheavy[elo[e]] = 1; vheavy[ehi[e]] = 1; }
}

// The structure of a round over the current faces a.fa (Fn > 0, their names below V): the edges (a.eoh, a.estart, a.elo, a.ehi,
// a.eval), the flags a.vborder and a.vheavy (where it is not null), and with `rings` the corners (a.vf, a.vfirst, a.vlast) and
// the rings (a.hie, a.lfirst .. a.hlast) of every vertex.  A is anything with these members: the remeshing's rm_arrays as they
// are at the call (its faces are swapped every round, so no copy of them is kept), the decimation's arrays of the call.  The
// caller has zeroed a.vborder .. a.hlast.  The ONE host read of the structure takes `words` counter words of cnt into hc; the
// edges are counted in cnt[e_word] and returned in *E.  a.iota holds 0, 1, ...; a.hkey, a.hkeys, a.vkey, a.vkeys, a.head and
// a.hpos are spent when it returns.
template <class A>
static inline int er_structure(const A &a, CubWorkspace &cub, int V, int Fn, bool rings, int *cnt, int words, int e_word, int *hc, int *E, hipStream_t st) {
    const long n = 3L * Fn;
    int vbits = 1;                                           // of a vertex index below V; never a sort over zero bits
    while ((1L << vbits) < V) ++vbits;
    DEV_LAUNCH(er_half_keys_kernel, n, (const int32_t *)a.fa, n, a.hkey, a.vkey);
    SURFD_TRY(cub.sort_pairs(a.hkey, a.hkeys, a.iota, a.sh, (int)n, 32 + vbits, st));
    DEV_LAUNCH(run_heads_kernel<~0ull>, n, (const er_u64 *)a.hkeys, (int)n, a.head);
    SURFD_TRY(cub.exclusive_sum(a.head, a.hpos, (int)n, st));
    SURFD_TRY(scan_total(a.head, a.hpos, (int)n, cnt + e_word, st));
    DEV_LAUNCH(er_edge_fill_kernel, n, (const er_u64 *)a.hkeys, (const int *)a.sh, (const int *)a.head, (const int *)a.hpos, n, a.eoh, a.estart, a.elo, a.ehi);
    if (rings) {
        SURFD_TRY(cub.sort_pairs(a.vkey, a.vkeys, a.iota, a.vf, (int)n, vbits, st));
        DEV_LAUNCH(er_run_bounds_kernel, n, (const unsigned *)a.vkeys, n, a.vfirst, a.vlast);
    }
    SURFD_TRY(read_words(cnt, hc, words, st));
    *E = hc[e_word];
    unsigned *hikey = a.vkey, *hikeys = a.vkeys;             // the corner keys are spent
    DEV_LAUNCH(er_edge_info_kernel, *E, (const int *)a.estart, (const int *)a.elo, (const int *)a.ehi, *E, a.eval, a.vborder, a.vheavy, hikey);
    if (rings) {
        DEV_LAUNCH(er_run_bounds_kernel, *E, (const unsigned *)a.elo, (long)*E, a.lfirst, a.llast);
        SURFD_TRY(cub.sort_pairs(hikey, hikeys, a.iota, a.hie, *E, vbits, st));
        DEV_LAUNCH(er_run_bounds_kernel, *E, (const unsigned *)hikeys, (long)*E, a.hfirst, a.hlast);
    }
    return SURFD_OK;
}

// ---- selection ------------------------------------------------------------------------------------------------------------------------
// m(v): the candidate of least priority at v, or -1
static __global__ void er_vertex_min_kernel(er_rings rings, int V, const int *__restrict__ cand, const er_u64 *__restrict__ ehash, int *__restrict__ mbest) {
    if (dev_tid() >= V) return;
    const er_ring r = rings.at(dev_tid());
    int best = -1;
    for (int j = 0; j < r.n; ++j) {
        const int e = r.edge(j);
        if (cand[e] && er_before(ehash, e, best)) best = e;
    }
    mbest[dev_tid()] = best;
}

// M(v): the least m over v and its neighbours
static __global__ void er_ring_min_kernel(er_rings rings, int V, const int *__restrict__ mbest, const er_u64 *__restrict__ ehash, int *__restrict__ Mbest) {
    if (dev_tid() >= V) return;
    const er_ring r = rings.at(dev_tid());
    int best = mbest[dev_tid()];
    for (int j = 0; j < r.n; ++j) {
        const int e = mbest[r.other(j)];
        if (e >= 0 && er_before(ehash, e, best)) best = e;
    }
    Mbest[dev_tid()] = best;
}

// ---- the faces after the collapses of a round -----------------------------------------------------------------------------------------
static __global__ void er_rename_faces_kernel(int32_t *__restrict__ fa, int F, const int *__restrict__ rename, int *__restrict__ live) {
    if (dev_tid() >= F) return;
    const long f = dev_tid();
    const int a = rename[fa[3 * f]], b = rename[fa[3 * f + 1]], c = rename[fa[3 * f + 2]];
    fa[3 * f] = a; fa[3 * f + 1] = b; fa[3 * f + 2] = c;
    live[f] = (a != b && b != c && a != c) ? 1 : 0;
}

static __global__ void er_compact_live_kernel(const int32_t *__restrict__ fa, const double *__restrict__ nref, int F, const int *__restrict__ live,
                                              const int *__restrict__ lpos, int32_t *__restrict__ out, double *__restrict__ nout) {
    if (dev_tid() >= F || !live[dev_tid()]) return;
    const long f = dev_tid(), n = lpos[f];
#pragma unroll
    for (int c = 0; c < 3; ++c) { out[3 * n + c] = fa[3 * f + c]; nout[3 * n + c] = nref[3 * f + c]; }
}

// ---- output ---------------------------------------------------------------------------------------------------------------------------
static __global__ void er_mark_named_kernel(const int32_t *__restrict__ fa, long n, int *__restrict__ stays) {
    if (dev_tid() < n) stays[fa[dev_tid()]] = 1;              // every writer stores the same 1
}

static __global__ void er_out_faces_kernel(const int32_t *__restrict__ fa, long n, const int *__restrict__ newid, int32_t *__restrict__ out) {
    if (dev_tid() < n) out[dev_tid()] = newid[fa[dev_tid()]];
}

// the number of vertices the Fn faces name -> *total; stays is left set, and with Fn > 0 newid is its exclusive sum
static inline int er_count_named(CubWorkspace &cub, const int32_t *fa, int Fn, int V, int *stays, int *newid, int *total, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(stays, 0, dev_bytes<int>(V), st));
    HIP_TRY(hipMemsetAsync(total, 0, sizeof(int), st));
    if (Fn > 0) {
        DEV_LAUNCH(er_mark_named_kernel, 3L * Fn, fa, 3L * Fn, stays);
        SURFD_TRY(cub.exclusive_sum(stays, newid, V, st));
        SURFD_TRY(scan_total(stays, newid, V, total, st));
    }
    return SURFD_OK;
}

}  // namespace surfd
