// Mesh cleaning on the device: the counterpart of meshproc.cull_and_merge / drop_duplicate_faces / drop_degenerate_faces /
// fill_small_holes, the four steps meshproc.clean_until_stable is made of.  meshproc is the contract: every output equals its
// output bit for bit and in the same order (vertex order, face order, every double).  tests/meshclean_ref.py restates the
// order-free form built here sequentially and tests/test_meshclean_cpu.py pins that restatement to meshproc.
//
// Contract.  Vertices are fp64 [V, 3], faces int32 [F, 3], both on the device; outputs go to buffers the caller sized for the
// largest result, the counts come back on the host.
//   cull_and_merge   a face that names a non-finite vertex goes.  The vertices that TAKE PART are those a remaining face names.
//                    Each takes the key (rint(x s), rint(y s), rint(z s)) as three int64, s = 1 / tolerance worked out by the
//                    caller (1e8 exactly for 1e-8); rint rounds ties to even, -0.0 and 0.0 share a key.  Vertices with equal keys
//                    become one: the survivor is the lowest index of the class and keeps its own bits, survivors keep their
//                    relative order, faces keep theirs and are re-indexed.  This is surfd_meshtopo_weld's rule with a quantised
//                    key and a participation mask.  A finite coordinate with |x s| >= 2^62 (of any vertex, as numpy converts all
//                    of them) is outside the conversion numpy defines: SURFD_ERR_ARG, never wrapped.
//   duplicates       two faces are the same when their sorted index triples are; the survivor of a class is its lowest face, with
//                    its own winding; THE OUTPUT IS ORDERED by ascending (largest, middle, smallest index), whether or not anything
//                    was removed (np.unique over meshproc._pack_rows; its wide fallback at indices >= 2^20 - 1 gives the same
//                    order, and nothing here changes at that boundary).
//   degenerate       a = p1 - p0, b = p2 - p0, c = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), |x| = sqrt((x0 x0 + x1 x1) + x2 x2),
//                    area = |c| * 0.5, la = |a|, lb = |b|, ha = (2.0 * area) / la where la > 1e-8 else 0, hb likewise; the face stays
//                    iff ha > height and hb > height (false with a NaN).  fp64, every operation rounded once (-ffp-contract=off).
//                    Face order is kept.
//   small holes      half-edge h = 3 f + c runs from t[f, c] to t[f, (c + 1) % 3] and is a BORDER half-edge iff its unordered vertex
//                    pair occurs exactly once among all 3 F half-edges (faces with repeated indices take part: meshproc.
//                    border_edge_rows, the rule of surfd_meshsmooth_create).  out(u) = the number of border half-edges leaving u;
//                    nxt(u) = where the one leads, where out(u) == 1.  A LOOP is a cycle u0 -> nxt(u0) -> ... -> u0 whose first
//                    return comes after exactly 3 or 4 steps, every vertex of which has out == 1, listed from its smallest vertex
//                    u0.  Vertices with out == 1 form a functional graph, so such loops are disjoint and every vertex tests its own
//                    cycle: one lane per vertex, at most four dependent loads.  With r the reversed listing a 3-loop gives the cap
//                    r and a 4-loop gives (r0, r1, r2) and (r2, r3, r0).  meshproc appends the caps in a stable sort by their
//                    smallest vertex.  NO TWO CAPS SHARE THEIR SMALLEST VERTEX: a vertex lies on at most one loop, it is the
//                    smallest vertex of the 3-cap or of (r2, r3, r0) only as u0, and of (r0, r1, r2) only as another vertex of that
//                    loop.  So a cap is stored at the slot of its smallest vertex and the slots in ascending order ARE that sort:
//                    a scan over V, no sort and no count of the caps on the host.  Fewer than 3 faces: no caps (meshproc returns).
//
// Passes (256-wide grids, one item per lane; sorts and scans are hipcub's through CubWorkspace):
//   cull    mc_vertex_flags (finite, range) -> face_mark (keep flag per face, used flag per vertex: every writer stores the
//           same 1) -> three stable 64-bit radix sorts of (key of one coordinate, vertex), z then y then x, the key re-read
//           through the permutation before each; a vertex that takes no part gets the key 2^63, which no quantised coordinate has,
//           so those gather in one run and split no class -> mc_heads (head of a run of equal keys) -> inclusive max of the head
//           positions -> group_rep (stable sorts of an ascending start: the head of a run is its lowest index) -> exclusive sums of the
//           survivor and keep flags -> mc_out_vertices, mc_out_faces.  face_mark and everything from the inclusive max to the
//           survivor count (group_representatives, shared with surfd_meshtopo_weld) are in meshedit.h.
//   dup     mc_dup_key0 (smallest index, 31 bits) -> sort -> mc_dup_key1 (largest << 32 | middle, 63 bits) -> sort -> mc_dup_heads
//           -> exclusive sum -> mc_dup_out (the head of every run, at its rank).
//   degen   mc_degenerate_flags -> exclusive sum -> mc_compact_faces.
//   holes   mc_edge_keys (hi << b | lo per half-edge, b the bits of an index below V: 2 b key bits to sort, not 64) -> sort ->
//           mc_border_next (out by integer atomicAdd: a count has no order; nxt by a plain store, read only where out == 1, that
//           is where one lane wrote it) -> mc_loops -> exclusive sum of the slot flags -> mc_caps_out.  The number of loops is a
//           reduction of the start flags: 3-loops = 2 loops - caps, 4-loops = caps - loops.
// Scratch (freed when the call returns): cull 52 V + 8 F bytes, dup 36 F, degen 8 F, holes 72 F + 32 V, carved from ONE
// DeviceScratch block per call (ScratchArena; it, the launch macro, the counter words and their one read-back are devscratch.h's),
// plus hipcub's workspace in a block of its own.  Nothing is kept between calls.
//
// Limits, all return codes: F >= 0, V >= 0, 3 F < 2^31, V < 2^31 (F = 0 or V = 0 give empty outputs).  An index outside [0, V)
// (negative, for the duplicate pass, which has no V) is SURFD_ERR_ARG.  The kernels that see caller indices compare them first
// and index nothing by one that fails; the flag they raise is read back with the counts at the end of the call.
// Host syncs: every call reads its counts and flags back ONCE, at its end (the scratch is freed behind that sync); none of the
// four reads anything back in between.  surfd_amd.meshclean.clean_until_stable therefore syncs 4 times on the fast return and
// 5 + (2 or 3 per round) times otherwise.  Calls run on the caller's stream.
// Bounds: every kernel guards its thread index against the count it is launched for; arrays of V entries are indexed only by
// indices compared against V in the same kernel or produced by the library (permutations of [0, V), survivors, cycle vertices
// taken from nxt, which holds validated destinations); output rows come from exclusive sums of flags over the input, so they
// stay below the input's length; caps are also compared against the caller's row count.
#include "common.h"
#include "devscratch.h"
#include "meshedit.h"
#include "meshscene.h"
#include <cmath>

namespace surfd {

typedef unsigned long long mc_u64;
constexpr mc_u64 MC_KEY_NONE = 0x8000000000000000ull;        // LLONG_MIN: |rint(x s)| < 2^62 for every vertex that takes part
enum { MC_BAD = 0, MC_RANGE = 1, MC_N0 = 2, MC_N1 = 3, MC_N2 = 4, MC_N3 = 5, MC_WORDS = 8 };

__device__ __forceinline__ bool mc_in(int t, int V) { return t >= 0 && t < V; }

__device__ __forceinline__ long long mc_quantise(double x, double scale) { return (long long)rint(x * scale); }      // ties to even; -0.0 -> 0

__device__ __forceinline__ void mc_sort3(int &a, int &b, int &c) {
    int t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
}

// ---- cull_and_merge -----------------------------------------------------------------------------------------------------------
__global__ void mc_vertex_flags_kernel(const double *__restrict__ vertices, int V, double scale, int *__restrict__ nonfinite, int *__restrict__ cnt) {
    if (dev_tid() >= V) return;
    const long v = dev_tid();
    const double x = vertices[3 * v], y = vertices[3 * v + 1], z = vertices[3 * v + 2];
    const int nf = vertex_nonfinite(vertices, v);
    nonfinite[v] = nf;
    if (!nf && !(fabs(x * scale) < 0x1p62 && fabs(y * scale) < 0x1p62 && fabs(z * scale) < 0x1p62)) cnt[MC_RANGE] = 1;      // every writer stores the same 1
}

// key[i] = the quantised coordinate c of vertex idx[i] (of vertex i without idx, which also starts the permutation in iota)
__global__ void mc_coord_key_kernel(const double *__restrict__ vertices, int V, double scale, const int *__restrict__ used, const int *__restrict__ idx, int c,
                                    mc_u64 *__restrict__ key, int *__restrict__ iota) {
    if (dev_tid() >= V) return;
    const int i = (int)dev_tid();
    const long v = idx ? idx[i] : i;
    key[i] = used[v] ? (mc_u64)mc_quantise(vertices[3 * v + c], scale) : MC_KEY_NONE;
    if (iota) iota[i] = i;
}

__global__ void mc_heads_kernel(const double *__restrict__ vertices, int V, double scale, const int *__restrict__ used, const int *__restrict__ idx,
                                int *__restrict__ headpos) {
    if (dev_tid() >= V) return;
    const int i = (int)dev_tid();
    bool same = i > 0;
    if (same) {
        const long a = idx[i], b = idx[i - 1];
        same = used[a] && used[b];
#pragma unroll
        for (int j = 0; j < 3; ++j) same = same && mc_quantise(vertices[3 * a + j], scale) == mc_quantise(vertices[3 * b + j], scale);
    }
    headpos[i] = same ? 0 : i;
}

__global__ void mc_out_vertices_kernel(const double *__restrict__ vertices, int V, const int *__restrict__ survives, const int *__restrict__ newidx,
                                       double *__restrict__ out) {
    if (dev_tid() >= V || !survives[dev_tid()]) return;
    const long v = dev_tid(), n = newidx[v];                   // n <= v
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * n + j] = vertices[3 * v + j];
}

__global__ void mc_out_faces_kernel(const int32_t *__restrict__ faces, int F, const int *__restrict__ keep, const int *__restrict__ pos, const int *__restrict__ rep,
                                    const int *__restrict__ newidx, int32_t *__restrict__ out) {
    if (dev_tid() >= F || !keep[dev_tid()]) return;            // a kept face names validated, finite, used vertices
    const long f = dev_tid(), n = pos[f];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * n + c] = newidx[rep[faces[3 * f + c]]];
}

// ---- drop_duplicate_faces -------------------------------------------------------------------------------------------------------
// indices are compared and packed here, never used as addresses
__global__ void mc_dup_key0_kernel(const int32_t *__restrict__ faces, int F, unsigned *__restrict__ key, int *__restrict__ iota, int *__restrict__ cnt) {
    if (dev_tid() >= F) return;
    const long f = dev_tid();
    int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || b < 0 || c < 0) cnt[MC_BAD] = 1;
    mc_sort3(a, b, c);
    key[f] = (unsigned)a;
    iota[f] = (int)f;
}

__global__ void mc_dup_key1_kernel(const int32_t *__restrict__ faces, int F, const int *__restrict__ idx, mc_u64 *__restrict__ key) {
    if (dev_tid() >= F) return;
    const long f = idx[dev_tid()];
    int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    mc_sort3(a, b, c);
    key[dev_tid()] = ((mc_u64)(unsigned)c << 32) | (mc_u64)(unsigned)b;
}

__global__ void mc_dup_heads_kernel(const int32_t *__restrict__ faces, int F, const int *__restrict__ idx, int *__restrict__ head) {
    if (dev_tid() >= F) return;
    const int i = (int)dev_tid();
    int same = 0;
    if (i > 0) {
        const long f = idx[i], g = idx[i - 1];
        int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        int p = faces[3 * g], q = faces[3 * g + 1], r = faces[3 * g + 2];
        mc_sort3(a, b, c); mc_sort3(p, q, r);
        same = a == p && b == q && c == r;
    }
    head[i] = same ? 0 : 1;
}

__global__ void mc_dup_out_kernel(const int32_t *__restrict__ faces, int F, const int *__restrict__ idx, const int *__restrict__ head, const int *__restrict__ rank,
                                  int32_t *__restrict__ out) {
    if (dev_tid() >= F || !head[dev_tid()]) return;
    const long f = idx[dev_tid()], n = rank[dev_tid()];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * n + c] = faces[3 * f + c];
}

// ---- drop_degenerate_faces ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double mc_norm(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

__global__ void __launch_bounds__(256) mc_degenerate_flags_kernel(const double *__restrict__ vertices, int V, const int32_t *__restrict__ faces, int F, double height,
                                                                  int *__restrict__ keep, int *__restrict__ cnt) {
    if (dev_tid() >= F) return;
    const long f = dev_tid();
    const long t0 = faces[3 * f], t1 = faces[3 * f + 1], t2 = faces[3 * f + 2];
    if (!mc_in((int)t0, V) || !mc_in((int)t1, V) || !mc_in((int)t2, V)) { cnt[MC_BAD] = 1; keep[f] = 0; return; }
    const double p0x = vertices[3 * t0], p0y = vertices[3 * t0 + 1], p0z = vertices[3 * t0 + 2];
    const double ax = vertices[3 * t1] - p0x, ay = vertices[3 * t1 + 1] - p0y, az = vertices[3 * t1 + 2] - p0z;
    const double bx = vertices[3 * t2] - p0x, by = vertices[3 * t2 + 1] - p0y, bz = vertices[3 * t2 + 2] - p0z;
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const double area = mc_norm(cx, cy, cz) * 0.5, la = mc_norm(ax, ay, az), lb = mc_norm(bx, by, bz);
    const double ha = la > 1e-8 ? (2.0 * area) / la : 0.0, hb = lb > 1e-8 ? (2.0 * area) / lb : 0.0;
    keep[f] = (ha > height && hb > height) ? 1 : 0;
}

__global__ void mc_compact_faces_kernel(const int32_t *__restrict__ faces, int F, const int *__restrict__ keep, const int *__restrict__ pos, int32_t *__restrict__ out) {
    if (dev_tid() >= F || !keep[dev_tid()]) return;
    const long f = dev_tid(), n = pos[f];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * n + c] = faces[3 * f + c];
}

// ---- fill_small_holes -----------------------------------------------------------------------------------------------------------
// indices are compared and packed here, never used as addresses
__global__ void mc_edge_keys_kernel(const int32_t *__restrict__ faces, int F, int V, int bits, mc_u64 *__restrict__ key, int *__restrict__ eh, int *__restrict__ cnt) {
    if (dev_tid() >= F) return;
    const long f = dev_tid();
    const int t[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    if (!mc_in(t[0], V) || !mc_in(t[1], V) || !mc_in(t[2], V)) cnt[MC_BAD] = 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int a = t[c], b = t[(c + 1) % 3];
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        key[3 * f + c] = ((mc_u64)(unsigned)hi << bits) | (mc_u64)(unsigned)lo;      // both below 2^bits where the flag stays down
        eh[3 * f + c] = (int)(3 * f + c);
    }
}

// per sorted position: a key that neither neighbour shares is a border half-edge u -> w; it counts at u and records w
__global__ void mc_border_next_kernel(const mc_u64 *__restrict__ skey, const int *__restrict__ sh, const int32_t *__restrict__ faces, int n, int V,
                                      int *outcnt, int *__restrict__ nxt) {
    if (dev_tid() >= n) return;
    const int i = (int)dev_tid();
    const mc_u64 k = skey[i];
    if ((i > 0 && skey[i - 1] == k) || (i < n - 1 && skey[i + 1] == k)) return;
    const int h = sh[i], f = h / 3, c = h - 3 * f;
    const int u = faces[h], w = faces[3 * (long)f + (c + 1) % 3];
    if (!mc_in(u, V) || !mc_in(w, V)) return;                   // the flag is up already (mc_edge_keys_kernel)
    atomicAdd(outcnt + u, 1);
    nxt[u] = w;                                                 // read only where outcnt[u] == 1: this lane was the only writer
}

// one lane per vertex u0: is it the smallest vertex of a loop of 3 or 4 border half-edges?  The caps go to the slots of their smallest vertices.
__global__ void mc_loops_kernel(int V, const int *__restrict__ outcnt, const int *__restrict__ nxt, int *__restrict__ start, int *__restrict__ capflag,
                                int32_t *__restrict__ captri) {
    if (dev_tid() >= V) return;
    const int u0 = (int)dev_tid();
    if (outcnt[u0] != 1) return;
    const int u1 = nxt[u0];
    if (u1 <= u0 || outcnt[u1] != 1) return;                   // u1 == u0: back after one step; u1 < u0: u0 is not the smallest
    const int u2 = nxt[u1];
    if (u2 <= u0 || outcnt[u2] != 1) return;                   // u2 == u0: back after two steps
    const int u3 = nxt[u2];
    if (u3 == u0) {                                            // r = (u2, u1, u0)
        start[u0] = 1;
        capflag[u0] = 1;
        captri[3 * (long)u0] = u2; captri[3 * (long)u0 + 1] = u1; captri[3 * (long)u0 + 2] = u0;
        return;
    }
    if (u3 < u0 || outcnt[u3] != 1 || nxt[u3] != u0) return;
    start[u0] = 1;                                             // r = (u3, u2, u1, u0): (u3, u2, u1) and (u1, u0, u3)
    const int m = min(u1, min(u2, u3));                        // > u0, and on this loop alone
    capflag[m] = 1;
    captri[3 * (long)m] = u3; captri[3 * (long)m + 1] = u2; captri[3 * (long)m + 2] = u1;
    capflag[u0] = 1;
    captri[3 * (long)u0] = u1; captri[3 * (long)u0 + 1] = u0; captri[3 * (long)u0 + 2] = u3;
}

__global__ void mc_caps_out_kernel(int V, const int *__restrict__ capflag, const int *__restrict__ pos, const int32_t *__restrict__ captri, long rows,
                                   int32_t *__restrict__ caps) {
    if (dev_tid() >= V || !capflag[dev_tid()]) return;
    const long m = dev_tid(), n = pos[m];
    if (n >= rows) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) caps[3 * n + c] = captri[3 * m + c];
}

}  // namespace surfd

using namespace surfd;

extern "C" int surfd_meshclean_cull_and_merge(const double *vertices, int V, const int32_t *faces, int F, double scale, double *out_vertices,
                                              int32_t *out_faces, int64_t *counts, surfd_stream s) {
    const char *who = "surfd_meshclean_cull_and_merge";
    if (!counts) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    for (int i = 0; i < 5; ++i) counts[i] = 0;
    SURFD_TRY(mesh_sizes(who, F, V));
    if (!(scale > 0.0) || !std::isfinite(scale)) SURFD_FAIL(SURFD_ERR_ARG, "%s: scale = %g must be positive and finite", who, scale);
    if (F == 0 || V == 0) return SURFD_OK;
    if (!vertices || !faces || !out_vertices || !out_faces) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    hipStream_t st = as_stream(s);
    DeviceScratch scratch;
    CubWorkspace cub{&scratch};
    int *cnt, *nonfinite, *used, *idxa, *idxb, *headpos, *hp, *rep, *survives, *newidx, *keep, *fpos;
    mc_u64 *key, *key2;
    ScratchArena arena("meshclean");
    SURFD_TRY(arena.open(scratch, dev_slot<int>(MC_WORDS) + 9 * dev_slot<int>(V) + 2 * dev_slot<mc_u64>(V) + 2 * dev_slot<int>(F)));
    SURFD_TRY(zeroed_words(arena, &cnt, MC_WORDS, st));
    SURFD_TRY(arena.get(&nonfinite, V)); SURFD_TRY(arena.get(&used, V)); SURFD_TRY(arena.get(&idxa, V)); SURFD_TRY(arena.get(&idxb, V));
    SURFD_TRY(arena.get(&headpos, V)); SURFD_TRY(arena.get(&hp, V)); SURFD_TRY(arena.get(&rep, V)); SURFD_TRY(arena.get(&survives, V));
    SURFD_TRY(arena.get(&newidx, V)); SURFD_TRY(arena.get(&key, V)); SURFD_TRY(arena.get(&key2, V));
    SURFD_TRY(arena.get(&keep, F)); SURFD_TRY(arena.get(&fpos, F));
    HIP_TRY(hipMemsetAsync(used, 0, dev_bytes<int>(V), st));
    DEV_LAUNCH(mc_vertex_flags_kernel, V, vertices, V, scale, nonfinite, cnt);
    DEV_LAUNCH(face_mark_kernel, F, faces, F, V, (const int *)nonfinite, keep, used, cnt + MC_BAD);
    // least significant coordinate first; the sorts are stable, so equal keys end up adjacent and ascending in the vertex index
    DEV_LAUNCH(mc_coord_key_kernel, V, vertices, V, scale, (const int *)used, (const int *)nullptr, 2, key, idxa);
    SURFD_TRY(cub.sort_pairs(key, key2, idxa, idxb, V, 64, st));
    DEV_LAUNCH(mc_coord_key_kernel, V, vertices, V, scale, (const int *)used, (const int *)idxb, 1, key, (int *)nullptr);
    SURFD_TRY(cub.sort_pairs(key, key2, idxb, idxa, V, 64, st));
    DEV_LAUNCH(mc_coord_key_kernel, V, vertices, V, scale, (const int *)used, (const int *)idxa, 0, key, (int *)nullptr);
    SURFD_TRY(cub.sort_pairs(key, key2, idxa, idxb, V, 64, st));
    DEV_LAUNCH(mc_heads_kernel, V, vertices, V, scale, (const int *)used, (const int *)idxb, headpos);
    SURFD_TRY(group_representatives(cub, V, idxb, headpos, hp, used, rep, survives, newidx, cnt + MC_N0, st));
    SURFD_TRY(cub.exclusive_sum(keep, fpos, F, st));
    SURFD_TRY(scan_total(keep, fpos, F, cnt + MC_N1, st));
    SURFD_TRY(cub.reduce_sum(nonfinite, cnt + MC_N2, V, st));
    SURFD_TRY(cub.reduce_sum(used, cnt + MC_N3, V, st));
    DEV_LAUNCH(mc_out_vertices_kernel, V, vertices, V, (const int *)survives, (const int *)newidx, out_vertices);
    DEV_LAUNCH(mc_out_faces_kernel, F, faces, F, (const int *)keep, (const int *)fpos, (const int *)rep, (const int *)newidx, out_faces);
    int hc[MC_WORDS];
    SURFD_TRY(read_words(cnt, hc, MC_WORDS, st));
    if (hc[MC_BAD]) return mesh_bad_index(who, V);
    if (hc[MC_RANGE]) SURFD_FAIL(SURFD_ERR_ARG, "%s: a finite coordinate times the scale %g reaches 2^62: beyond the range of the 64-bit keys", who, scale);
    counts[0] = hc[MC_N0];                                   // vertices that stay
    counts[1] = hc[MC_N1];                                   // faces that stay
    counts[2] = hc[MC_N2];                                   // non-finite vertices
    counts[3] = (int64_t)V - hc[MC_N2] - hc[MC_N3];          // finite vertices that no remaining face names
    counts[4] = (int64_t)hc[MC_N3] - hc[MC_N0];              // vertices merged into a lower one
    return SURFD_OK;
}

extern "C" int surfd_meshclean_drop_duplicate_faces(const int32_t *faces, int F, int32_t *out_faces, int64_t *count, surfd_stream s) {
    const char *who = "surfd_meshclean_drop_duplicate_faces";
    if (!count) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    *count = 0;
    SURFD_TRY(mesh_sizes(who, F, 0));
    if (F == 0) return SURFD_OK;
    if (!faces || !out_faces) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    hipStream_t st = as_stream(s);
    DeviceScratch scratch;
    CubWorkspace cub{&scratch};
    int *cnt, *idxa, *idxb, *head, *rank;
    unsigned *k0, *k0s;
    mc_u64 *k1, *k1s;
    ScratchArena arena("meshclean");
    SURFD_TRY(arena.open(scratch, dev_slot<int>(MC_WORDS) + 4 * dev_slot<int>(F) + dev_slot<unsigned>(F) + 2 * dev_slot<mc_u64>(F)));
    SURFD_TRY(zeroed_words(arena, &cnt, MC_WORDS, st));
    SURFD_TRY(arena.get(&idxa, F)); SURFD_TRY(arena.get(&idxb, F)); SURFD_TRY(arena.get(&head, F)); SURFD_TRY(arena.get(&rank, F));
    SURFD_TRY(arena.get(&k0, F)); SURFD_TRY(arena.get(&k1, F)); SURFD_TRY(arena.get(&k1s, F));
    k0s = (unsigned *)k1;                                    // 4 F of the 8 F bytes that the second sort's keys overwrite after the first sort is done
    SURFD_TRY(cub.sort_pairs(k1, k1s, idxb, idxa, F, 63, st, true));        // the second sort is the larger: one workspace allocation
    DEV_LAUNCH(mc_dup_key0_kernel, F, faces, F, k0, idxa, cnt);
    SURFD_TRY(cub.sort_pairs(k0, k0s, idxa, idxb, F, 31, st));
    DEV_LAUNCH(mc_dup_key1_kernel, F, faces, F, (const int *)idxb, k1);
    SURFD_TRY(cub.sort_pairs(k1, k1s, idxb, idxa, F, 63, st));
    DEV_LAUNCH(mc_dup_heads_kernel, F, faces, F, (const int *)idxa, head);
    SURFD_TRY(cub.exclusive_sum(head, rank, F, st));
    SURFD_TRY(scan_total(head, rank, F, cnt + MC_N0, st));
    DEV_LAUNCH(mc_dup_out_kernel, F, faces, F, (const int *)idxa, (const int *)head, (const int *)rank, out_faces);
    int hc[MC_WORDS];
    SURFD_TRY(read_words(cnt, hc, MC_WORDS, st));
    if (hc[MC_BAD]) SURFD_FAIL(SURFD_ERR_ARG, "%s: a face names a negative vertex index", who);
    *count = hc[MC_N0];
    return SURFD_OK;
}

extern "C" int surfd_meshclean_drop_degenerate_faces(const double *vertices, int V, const int32_t *faces, int F, double height, int32_t *out_faces,
                                                     int64_t *count, surfd_stream s) {
    const char *who = "surfd_meshclean_drop_degenerate_faces";
    if (!count) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    *count = 0;
    SURFD_TRY(mesh_sizes(who, F, V));
    if (F == 0) return SURFD_OK;
    if (!faces || !out_faces || (V > 0 && !vertices)) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    hipStream_t st = as_stream(s);
    DeviceScratch scratch;
    CubWorkspace cub{&scratch};
    int *cnt, *keep, *pos;
    ScratchArena arena("meshclean");
    SURFD_TRY(arena.open(scratch, dev_slot<int>(MC_WORDS) + 2 * dev_slot<int>(F)));
    SURFD_TRY(zeroed_words(arena, &cnt, MC_WORDS, st));
    SURFD_TRY(arena.get(&keep, F)); SURFD_TRY(arena.get(&pos, F));
    DEV_LAUNCH(mc_degenerate_flags_kernel, F, vertices, V, faces, F, height, keep, cnt);
    SURFD_TRY(cub.exclusive_sum(keep, pos, F, st));
    SURFD_TRY(scan_total(keep, pos, F, cnt + MC_N0, st));
    DEV_LAUNCH(mc_compact_faces_kernel, F, faces, F, (const int *)keep, (const int *)pos, out_faces);
    int hc[MC_WORDS];
    SURFD_TRY(read_words(cnt, hc, MC_WORDS, st));
    if (hc[MC_BAD]) return mesh_bad_index(who, V);
    *count = hc[MC_N0];
    return SURFD_OK;
}

extern "C" int surfd_meshclean_fill_small_holes(const int32_t *faces, int F, int V, int32_t *caps, int64_t cap_rows, int64_t *counts, surfd_stream s) {
    const char *who = "surfd_meshclean_fill_small_holes";
    if (!counts) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    counts[0] = counts[1] = counts[2] = 0;
    SURFD_TRY(mesh_sizes(who, F, V));
    if (F < 3) return SURFD_OK;                              // meshproc returns its input
    const int64_t most = std::min<int64_t>(V, 3L * F / 2);   // a cap has its own smallest vertex, and uses up at least two border half-edges
    if (!faces || cap_rows < most || (most > 0 && !caps))
        SURFD_FAIL(SURFD_ERR_ARG, "%s: caps must have room for min(V, 3 F / 2) = %lld rows, got %lld", who, (long long)most, (long long)cap_rows);
    hipStream_t st = as_stream(s);
    DeviceScratch scratch;
    CubWorkspace cub{&scratch};
    const int H = 3 * F;
    int *cnt, *eh, *sh, *outcnt, *nxt, *start, *capflag, *cpos;
    int32_t *captri;
    mc_u64 *key, *skey;
    ScratchArena arena("meshclean");
    SURFD_TRY(arena.open(scratch, dev_slot<int>(MC_WORDS) + 2 * dev_slot<mc_u64>(H) + 2 * dev_slot<int>(H) + 5 * dev_slot<int>(V) + dev_slot<int32_t>(3L * V)));
    SURFD_TRY(zeroed_words(arena, &cnt, MC_WORDS, st));
    SURFD_TRY(arena.get(&key, H)); SURFD_TRY(arena.get(&skey, H)); SURFD_TRY(arena.get(&eh, H)); SURFD_TRY(arena.get(&sh, H));
    SURFD_TRY(arena.get(&outcnt, V)); SURFD_TRY(arena.get(&start, V)); SURFD_TRY(arena.get(&capflag, V)); SURFD_TRY(arena.get(&nxt, V));
    SURFD_TRY(arena.get(&cpos, V)); SURFD_TRY(arena.get(&captri, 3L * V));
    HIP_TRY(hipMemsetAsync(outcnt, 0, 3 * dev_slot<int>(V), st));      // outcnt, start, capflag: three slots in a row
    int bits = 1;                                            // of an index below V: the keys take 2 bits of the radix sort, not 64
    while (bits < 31 && (1L << bits) < V) ++bits;
    DEV_LAUNCH(mc_edge_keys_kernel, F, faces, F, V, bits, key, eh, cnt);
    SURFD_TRY(cub.sort_pairs(key, skey, eh, sh, H, 2 * bits, st));
    DEV_LAUNCH(mc_border_next_kernel, H, (const mc_u64 *)skey, (const int *)sh, faces, H, V, outcnt, nxt);
    if (V > 0) {
        DEV_LAUNCH(mc_loops_kernel, V, V, (const int *)outcnt, (const int *)nxt, start, capflag, captri);
        SURFD_TRY(cub.exclusive_sum(capflag, cpos, V, st));
        SURFD_TRY(scan_total(capflag, cpos, V, cnt + MC_N0, st));
        SURFD_TRY(cub.reduce_sum(start, cnt + MC_N1, V, st));
        DEV_LAUNCH(mc_caps_out_kernel, V, V, (const int *)capflag, (const int *)cpos, (const int32_t *)captri, (long)cap_rows, caps);
    }
    int hc[MC_WORDS];
    SURFD_TRY(read_words(cnt, hc, MC_WORDS, st));
    if (hc[MC_BAD]) return mesh_bad_index(who, V);
    const int64_t n_caps = hc[MC_N0], n_loops = hc[MC_N1];
    counts[0] = n_caps;                                      // a 3-loop gives one cap, a 4-loop two
    counts[1] = 2 * n_loops - n_caps;                        // 3-loops
    counts[2] = n_caps - n_loops;                            // 4-loops
    return SURFD_OK;
}
