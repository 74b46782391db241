// Vertex-moving work on a triangle mesh that stays on the device: Laplacian smoothing (uniform or cotangent weights, with
// MeshLab's border rule), the uniform umbrella operator (over all edges: Taubin's lambda | mu; over the border polyline only:
// the border smoothing of get_mesh_from_udf), and vertex normals (corner-angle or area weighted).  The host counterparts are
// meshproc.laplacian_smooth / smooth_borders / vertex_normals_by_angle; tests/meshsmooth_ref.py restates the arithmetic below
// sequentially, and the device results equal that restatement bit for bit (the one exception is acos, see normals).
//
// Contract.
//   arithmetic  fp64 throughout on the caller's positions ([V, 3] fp32 or fp64, converted exactly); outputs are fp64.  Only
//               + - * / sqrt, every operation rounded once (-ffp-contract=off), plus the one acos of the "angle" normals.
//               No atomics anywhere: every output is a function of the input arrays alone, not of the launch geometry.
//   half-edge   h = 3 f + c runs from t[f, c] (origin) to t[f, (c + 1) % 3] (destination); its opposite corner is t[f, (c + 2) % 3].
//   border      a half-edge whose unordered vertex pair occurs exactly once among ALL 3 F half-edges.  Every face takes part in
//               the count, a face with repeated indices too (meshproc.border_edge_rows); meshtopo.hip sets such faces aside,
//               so its classification is NOT this one.  A vertex is a border vertex when it ends a border half-edge.
//   OUT(v)      the half-edges that leave v, ascending in h;  IN(v): those that arrive at v, ascending in h.
//   BN(v)       the border neighbours of v: the other ends u of the border half-edges at v, first those with u >= v ascending,
//               then those with u <= v ascending (a border half-edge from v to v, which a face (v, v, w) can make, is listed
//               in both runs): the order in which np.add.at meets them in meshproc.smooth_borders.
//   corners(v)  the corners (f, c) with t[f, c] == v, ascending in (c, f): all corners 0 by face, then corners 1, then corners 2.
//   sweeps      Jacobi: a sweep reads the previous positions and writes another buffer; one launch per sweep, one vertex per lane.
//               The order of summation inside a vertex is part of the contract (it is the order np.add.at gives the host code):
//
//   laplacian   w(h) = dot / cr where cr > 0, else 0, with a = p[dest] - p[opp], b = p[origin] - p[opp],
//               c = a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), cr = sqrt((cx cx + cy cy) + cz cz),
//               dot = (a0 b0 + a1 b1) + a2 b2; w = 1 without `cotangent`.
//               A vertex that is not a border vertex (every vertex with boundary = 0): acc = 0, cnt = 0; for h in OUT(v):
//               acc += p[dest] * w, cnt += w; then for h in IN(v): acc += p[origin] * w, cnt += w.
//               A border vertex (boundary = 1): acc = p, cnt = 1; for the border h in OUT(v): acc += p[dest], cnt += 1; then
//               for the border h in IN(v): acc += p[origin], cnt += 1.  Its inner half-edges are not read.
//               new p = (p + acc) / (cnt + 1) where cnt > 0, else p.
//   umbrella    acc = 0, deg = 0; set = all: for h in OUT(v): acc += p[dest]; for h in IN(v): acc += p[origin]; set = border:
//               for u in BN(v): acc += p[u]; deg counts the terms.  new p = p + k * (acc / deg - p) where deg > 0, else p.
//               Sweep s uses k0 when s is even and k1 when it is odd (Taubin: k0 = lambda, k1 = mu, two sweeps per step).
//   normals     per corner, with (P0, P1, P2) the positions of the face in ITS order: n = (P1 - P0) x (P2 - P0), and with
//               a = P[c + 1] - P[c], b = P[c + 2] - P[c]:
//               angle: term = (n / |n|, 0 where |n| == 0) * acos(clamp(dot(a, b) / max(|a| |b|, 1e-300), -1, 1));
//               area:  term = n.   |x| = sqrt((x0 x0 + x1 x1) + x2 x2), dot as above, NaNs pass through clamp and max.
//               raw[v] = the sum of the terms over corners(v) in their order, from 0; unit[v] = raw / |raw|, 0 where |raw| == 0.
//               acos is the device library's: "area" is bit-exact against the restatement, "angle" is so up to acos.
//
// Build (create, once per connectivity; sizes H = 3 F):
//   keys      one 64-bit key hi << 32 | lo per half-edge (the order of meshproc._pack_rows), hipcub radix sort of (key, h), stable;
//             a sorted position is a border half-edge iff both neighbours hold other keys; the exclusive sum of those flags ranks
//             the border edges in key order; B (their number) is read back.
//   BN        2 B records (lo -> hi for rank r at r, hi -> lo at B + r), stable sort by the first vertex: per vertex the order above.
//   OUT, IN   stable sorts of (origin(h), h) and (destination(h), h): ascending in h inside a vertex.
//   corners   stable sort of (t[f, c], c F + f).
//   offsets   per list a binary search per vertex in the sorted keys (V + 1 entries).
// Kept per handle: the triangles, per OUT / IN record 8 bytes (neighbour, opposite corner | border bit), per corner 4, per border
// record 4, four offset arrays of V + 1 words, one byte per vertex: 72 F + 17 V + 8 B bytes, plus the arena (two position buffers).
// The cotangents are worked out in the gather: writing them per half-edge first and reading them back gave the same bits and was
// slower at every size measured, so that variant is not kept.
//
// Limits, all return codes: F >= 0, V >= 0, 3 F < 2^31, V < 2^31; an index outside [0, V) is refused in create (checked by the
// first kernel, which uses indices only as values; nothing indexed by them runs before the flag has been read).
// Host reads: create only (the bad-index flag, B, the number of border vertices).  laplacian, umbrella and vertex_normals only
// enqueue; the arena grows in the first call that needs it.  ONE STREAM AT A TIME PER HANDLE.
// Bounds: every kernel guards its thread index; lists are walked between offsets that the binary search puts in [0, n]; the
// neighbour / opposite / corner records hold indices that create validated.
#include "common.h"
#include "devscratch.h"
#include "meshscene.h"

namespace surfd {

typedef unsigned long long ms_u64;
constexpr int MS_BORDER_BIT = (int)0x80000000u;

// ---- create ----------------------------------------------------------------------------------------------------------------
// the only kernel that sees unvalidated indices: they are compared and packed, never used as addresses
__global__ void ms_keys_kernel(const int32_t *__restrict__ tri, int F, int V, ms_u64 *__restrict__ ekey, int *__restrict__ eh, unsigned *__restrict__ okey,
                               unsigned *__restrict__ ikey, unsigned *__restrict__ ckey, int *__restrict__ cpay, int *__restrict__ bad) {
    if (dev_tid() >= F) return;
    const int f = (int)dev_tid();
    const int t[3] = {tri[3 * (long)f], tri[3 * (long)f + 1], tri[3 * (long)f + 2]};
    if (t[0] < 0 || t[0] >= V || t[1] < 0 || t[1] >= V || t[2] < 0 || t[2] >= V) *bad = 1;      // every writer stores the same 1
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int a = t[c], b = t[(c + 1) % 3];
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        const long h = 3 * (long)f + c;
        ekey[h] = ((ms_u64)(unsigned)hi << 32) | (ms_u64)(unsigned)lo;
        eh[h] = (int)h;
        okey[h] = (unsigned)a;
        ikey[h] = (unsigned)b;
        ckey[(long)c * F + f] = (unsigned)a;
        cpay[(long)c * F + f] = (int)h;
    }
}

__global__ void ms_border_flags_kernel(const ms_u64 *__restrict__ skey, int n, int *__restrict__ flag) {
    if (dev_tid() >= n) return;
    const int i = (int)dev_tid();
    const ms_u64 k = skey[i];
    flag[i] = ((i == 0 || skey[i - 1] != k) && (i == n - 1 || skey[i + 1] != k)) ? 1 : 0;
}

// per sorted position: the border byte of its half-edge and, for a border edge of rank r, the two records of BN
__global__ void ms_border_records_kernel(const ms_u64 *__restrict__ skey, const int *__restrict__ sh, const int *__restrict__ flag, const int *__restrict__ rank,
                                         int n, int B, unsigned char *__restrict__ hborder, unsigned *__restrict__ bsrc, int *__restrict__ bdst) {
    if (dev_tid() >= n) return;
    const int i = (int)dev_tid();
    hborder[sh[i]] = (unsigned char)flag[i];
    if (!flag[i]) return;
    const ms_u64 k = skey[i];
    const int lo = (int)(k & 0xFFFFFFFFull), hi = (int)(k >> 32), r = rank[i];      // r < B
    bsrc[r] = (unsigned)lo; bdst[r] = hi;
    bsrc[(long)B + r] = (unsigned)hi; bdst[(long)B + r] = lo;
}

// off[v] = the first position of sorted[0 .. n) that holds a key >= v, + base; v = 0 .. V
__global__ void ms_offsets_kernel(const unsigned *__restrict__ sorted, unsigned n, int V, unsigned base, unsigned *__restrict__ off) {
    const long v = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (v > V) return;
    unsigned lo = 0, hi = n;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (sorted[mid] < (unsigned)v) lo = mid + 1; else hi = mid;
    }
    off[v] = base + lo;
}

// the records of OUT (arriving = 0) or IN (arriving = 1) in their sorted order
__global__ void ms_adjacency_kernel(const int32_t *__restrict__ tri, const int *__restrict__ sh, const unsigned char *__restrict__ hborder, int n, int arriving,
                                    int *__restrict__ nbr, int *__restrict__ opp) {
    if (dev_tid() >= n) return;
    const int i = (int)dev_tid();
    const int h = sh[i], f = h / 3, c = h - 3 * f;
    nbr[i] = arriving ? tri[h] : tri[3 * (long)f + (c + 1) % 3];
    opp[i] = tri[3 * (long)f + (c + 2) % 3] | (hborder[h] ? MS_BORDER_BIT : 0);
}

__global__ void ms_vertex_border_kernel(const unsigned *__restrict__ boff, int V, unsigned char *__restrict__ vborder, int *__restrict__ vflag) {
    if (dev_tid() >= V) return;
    const int v = (int)dev_tid();
    const int on = boff[v + 1] > boff[v] ? 1 : 0;
    vborder[v] = (unsigned char)on;
    vflag[v] = on;
}

// ---- positions -------------------------------------------------------------------------------------------------------------
template <class T>
__global__ void ms_convert_kernel(const T *__restrict__ in, long n, double *__restrict__ out) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}

struct ms_d3 { double x, y, z; };
template <class T>
__device__ __forceinline__ ms_d3 ms_load(const T *__restrict__ p, int v) {
    return {(double)p[3 * (long)v], (double)p[3 * (long)v + 1], (double)p[3 * (long)v + 2]};
}
__device__ __forceinline__ ms_d3 ms_sub(ms_d3 a, ms_d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ ms_d3 ms_cross(ms_d3 a, ms_d3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double ms_dot(ms_d3 a, ms_d3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ double ms_len(ms_d3 a) { return sqrt((a.x * a.x + a.y * a.y) + a.z * a.z); }

__device__ __forceinline__ double ms_cot(ms_d3 pdest, ms_d3 porigin, ms_d3 popp) {
    const ms_d3 a = ms_sub(pdest, popp), b = ms_sub(porigin, popp);
    const double cr = ms_len(ms_cross(a, b)), dot = ms_dot(a, b);
    return cr > 0.0 ? dot / cr : 0.0;
}

// COT 0: w = 1; 1: the cotangent of the angle opposite the half-edge
template <int COT>
__global__ void __launch_bounds__(256) ms_laplacian_kernel(const double *__restrict__ p, double *__restrict__ q, int V, const unsigned *__restrict__ ooff,
                                                           const unsigned *__restrict__ ioff, const int *__restrict__ nbr, const int *__restrict__ opp,
                                                           const unsigned char *__restrict__ vborder) {
    if (dev_tid() >= V) return;
    const int v = (int)dev_tid();
    const ms_d3 pv = ms_load(p, v);
    const bool onb = vborder != nullptr && vborder[v] != 0;        // vborder == nullptr: boundary = 0, no half-edge is a border half-edge
    ms_d3 acc = onb ? pv : ms_d3{0.0, 0.0, 0.0};
    double cnt = onb ? 1.0 : 0.0;
#pragma unroll
    for (int arriving = 0; arriving < 2; ++arriving) {
        const unsigned *off = arriving ? ioff : ooff;
        const unsigned e = off[v + 1];
        for (unsigned i = off[v]; i < e; ++i) {
            const int o = opp[i];
            if (onb) {
                if (o >= 0) continue;
                const ms_d3 pn = ms_load(p, nbr[i]);
                acc.x += pn.x; acc.y += pn.y; acc.z += pn.z;
                cnt += 1.0;
            } else {
                const ms_d3 pn = ms_load(p, nbr[i]);
                double wt = 1.0;
                if (COT) {
                    const ms_d3 po = ms_load(p, o & ~MS_BORDER_BIT);
                    wt = arriving ? ms_cot(pv, pn, po) : ms_cot(pn, pv, po);
                }
                acc.x += pn.x * wt; acc.y += pn.y * wt; acc.z += pn.z * wt;
                cnt += wt;
            }
        }
    }
    ms_d3 r = pv;
    if (cnt > 0.0) {
        const double d = cnt + 1.0;
        r = {(pv.x + acc.x) / d, (pv.y + acc.y) / d, (pv.z + acc.z) / d};
    }
    q[3 * (long)v] = r.x; q[3 * (long)v + 1] = r.y; q[3 * (long)v + 2] = r.z;
}

// off1 (nullable): a second list walked after the first, over the same nbr array
__global__ void __launch_bounds__(256) ms_umbrella_kernel(const double *__restrict__ p, double *__restrict__ q, int V, const unsigned *__restrict__ off0,
                                                          const unsigned *__restrict__ off1, const int *__restrict__ nbr, double k) {
    if (dev_tid() >= V) return;
    const int v = (int)dev_tid();
    const ms_d3 pv = ms_load(p, v);
    ms_d3 acc = {0.0, 0.0, 0.0};
    unsigned deg = 0;
    for (int l = 0; l < 2; ++l) {
        const unsigned *off = l ? off1 : off0;
        if (!off) break;
        const unsigned e = off[v + 1];
        for (unsigned i = off[v]; i < e; ++i) {
            const ms_d3 pn = ms_load(p, nbr[i]);
            acc.x += pn.x; acc.y += pn.y; acc.z += pn.z;
            ++deg;
        }
    }
    ms_d3 r = pv;
    if (deg > 0) {
        const double d = (double)deg;
        r = {pv.x + k * (acc.x / d - pv.x), pv.y + k * (acc.y / d - pv.y), pv.z + k * (acc.z / d - pv.z)};
    }
    q[3 * (long)v] = r.x; q[3 * (long)v + 1] = r.y; q[3 * (long)v + 2] = r.z;
}

template <class T, int ANGLE>
__global__ void __launch_bounds__(256) ms_normals_kernel(const T *__restrict__ p, const int32_t *__restrict__ tri, int V, const unsigned *__restrict__ coff,
                                                         const int *__restrict__ ch, double *__restrict__ unit, double *__restrict__ raw) {
    if (dev_tid() >= V) return;
    const int v = (int)dev_tid();
    ms_d3 acc = {0.0, 0.0, 0.0};
    const unsigned e = coff[v + 1];
    for (unsigned i = coff[v]; i < e; ++i) {
        const int h = ch[i], f = h / 3, c = h - 3 * f;
        const ms_d3 pc = ms_load(p, tri[h]);                                        // tri[h] == v
        const ms_d3 pn = ms_load(p, tri[3 * (long)f + (c + 1) % 3]);
        const ms_d3 pp = ms_load(p, tri[3 * (long)f + (c + 2) % 3]);
        // the face's own order (P0, P1, P2): a rotation has the same cross product, but not the same bits
        const ms_d3 p0 = c == 0 ? pc : (c == 1 ? pp : pn);
        const ms_d3 p1 = c == 0 ? pn : (c == 1 ? pc : pp);
        const ms_d3 p2 = c == 0 ? pp : (c == 1 ? pn : pc);
        ms_d3 n = ms_cross(ms_sub(p1, p0), ms_sub(p2, p0));
        if (ANGLE) {
            const double ln = ms_len(n);
            n = ln > 0.0 ? ms_d3{n.x / ln, n.y / ln, n.z / ln} : ms_d3{0.0, 0.0, 0.0};
            const ms_d3 a = ms_sub(pn, pc), b = ms_sub(pp, pc);
            const double ll = ms_len(a) * ms_len(b);
            const double den = ll < 1e-300 ? 1e-300 : ll;                           // a NaN passes, as through np.maximum
            double cs = ms_dot(a, b) / den;
            cs = cs < -1.0 ? -1.0 : (cs > 1.0 ? 1.0 : cs);                          // and through np.clip
            const double ang = acos(cs);
            n = {n.x * ang, n.y * ang, n.z * ang};
        }
        acc.x += n.x; acc.y += n.y; acc.z += n.z;
    }
    if (raw) { raw[3 * (long)v] = acc.x; raw[3 * (long)v + 1] = acc.y; raw[3 * (long)v + 2] = acc.z; }
    if (unit) {
        const double ln = ms_len(acc);
        const ms_d3 u = ln > 0.0 ? ms_d3{acc.x / ln, acc.y / ln, acc.z / ln} : ms_d3{0.0, 0.0, 0.0};
        unit[3 * (long)v] = u.x; unit[3 * (long)v + 1] = u.y; unit[3 * (long)v + 2] = u.z;
    }
}

}  // namespace surfd

using namespace surfd;

struct surfd_meshsmooth {
    int F = 0, V = 0, B = 0, n_border_vertices = 0;
    int32_t *tri = nullptr;
    unsigned *ooff = nullptr, *ioff = nullptr, *coff = nullptr, *boff = nullptr;      // V + 1 each; ioff counts from 3 F (IN follows OUT)
    int *nbr = nullptr, *opp = nullptr;                                               // 6 F each: OUT records, then IN records
    int *ch = nullptr;                                                                // 3 F: the half-edge 3 f + c of every corner
    int *bnbr = nullptr;                                                              // 2 B
    unsigned char *vborder = nullptr;                                                 // V
    DeviceArena arena;                                                                // positions A, positions B
};

static void ms_free(surfd_meshsmooth *m) {
    (void)hipFree(m->tri); (void)hipFree(m->ooff); (void)hipFree(m->ioff); (void)hipFree(m->coff); (void)hipFree(m->boff);
    (void)hipFree(m->nbr); (void)hipFree(m->opp); (void)hipFree(m->ch); (void)hipFree(m->bnbr); (void)hipFree(m->vborder);
    m->arena.release();
    delete m;
}

extern "C" int surfd_meshsmooth_create(const int32_t *triangles, int F, int V, surfd_stream s, surfd_meshsmooth **out) {
    if (!out) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshsmooth_create: null argument");
    *out = nullptr;
    SURFD_TRY(mesh_sizes("surfd_meshsmooth_create", F, V));
    if (F > 0 && !triangles) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshsmooth_create: null argument");
    hipStream_t st = as_stream(s);
    std::unique_ptr<surfd_meshsmooth, void (*)(surfd_meshsmooth *)> owner(new surfd_meshsmooth(), ms_free);      // freed on every early return
    surfd_meshsmooth *m = owner.get();
    m->F = F; m->V = V;
    if (F == 0) {
        *out = owner.release();
        return SURFD_OK;
    }
    const int H = 3 * F;
    HIP_TRY(hipMalloc(&m->tri, dev_bytes<int32_t>(H)));
    HIP_TRY(hipMalloc(&m->ooff, dev_bytes<unsigned>(V + 1L))); HIP_TRY(hipMalloc(&m->ioff, dev_bytes<unsigned>(V + 1L)));
    HIP_TRY(hipMalloc(&m->coff, dev_bytes<unsigned>(V + 1L))); HIP_TRY(hipMalloc(&m->boff, dev_bytes<unsigned>(V + 1L)));
    HIP_TRY(hipMalloc(&m->nbr, dev_bytes<int>(2L * H))); HIP_TRY(hipMalloc(&m->opp, dev_bytes<int>(2L * H)));
    HIP_TRY(hipMalloc(&m->ch, dev_bytes<int>(H)));
    HIP_TRY(hipMalloc(&m->vborder, dev_bytes<unsigned char>(V)));
    DeviceScratch scratch;
    CubWorkspace cub{&scratch};                             // one workspace for every sort, scan and reduction below
    ms_u64 *ekey, *ekey2;
    int *eh, *eh2, *cpay, *flag, *rank, *bdst, *sh, *scal, *vflag;
    unsigned *okey, *ikey, *ckey, *skey, *bsrc;
    unsigned char *hborder;
    SURFD_TRY(scratch.get(&ekey, H)); SURFD_TRY(scratch.get(&ekey2, H)); SURFD_TRY(scratch.get(&eh, H)); SURFD_TRY(scratch.get(&eh2, H));
    SURFD_TRY(scratch.get(&cpay, H)); SURFD_TRY(scratch.get(&flag, H)); SURFD_TRY(scratch.get(&rank, H)); SURFD_TRY(scratch.get(&sh, H));
    SURFD_TRY(scratch.get(&okey, H)); SURFD_TRY(scratch.get(&ikey, H)); SURFD_TRY(scratch.get(&ckey, H)); SURFD_TRY(scratch.get(&skey, H));
    SURFD_TRY(scratch.get(&hborder, H)); SURFD_TRY(scratch.get(&vflag, V)); SURFD_TRY(scratch.get(&scal, 4));
    HIP_TRY(hipMemsetAsync(scal, 0, 4 * sizeof(int), st));
    HIP_TRY(hipMemcpyAsync(m->tri, triangles, (size_t)H * sizeof(int32_t), hipMemcpyDefault, st));
    DEV_LAUNCH(ms_keys_kernel, F, (const int32_t *)m->tri, F, V, ekey, eh, okey, ikey, ckey, cpay, scal);
    SURFD_TRY(cub.sort_pairs(ekey, ekey2, eh, eh2, H, 64, st));
    DEV_LAUNCH(ms_border_flags_kernel, H, (const ms_u64 *)ekey2, H, flag);
    SURFD_TRY(cub.exclusive_sum(flag, rank, H, st));
    SURFD_TRY(scan_total(flag, rank, H, scal + 1, st));
    int hs[4];
    SURFD_TRY(read_words(scal, hs, 4, st));
    if (hs[0]) return mesh_bad_index("surfd_meshsmooth_create", V);        // nothing below this line sees an unvalidated index
    const int B = m->B = hs[1];
    HIP_TRY(hipMalloc(&m->bnbr, dev_bytes<int>(2L * B)));
    SURFD_TRY(scratch.get(&bsrc, 2L * B));
    SURFD_TRY(scratch.get(&bdst, 2L * B));
    DEV_LAUNCH(ms_border_records_kernel, H, (const ms_u64 *)ekey2, (const int *)eh2, (const int *)flag, (const int *)rank, H, B, hborder, bsrc, bdst);
    // BN: the sorted keys (2 B <= 2 H words) go to ekey (8 H bytes), which the first sort has read and nothing needs any more
    unsigned *bsorted = (unsigned *)ekey;
    if (B > 0) SURFD_TRY(cub.sort_pairs(bsrc, bsorted, bdst, m->bnbr, 2 * B, 32, st));
    DEV_LAUNCH(ms_offsets_kernel, V + 1L, (const unsigned *)bsorted, 2u * (unsigned)B, V, 0u, m->boff);
    DEV_LAUNCH(ms_vertex_border_kernel, V, (const unsigned *)m->boff, V, m->vborder, vflag);
    if (V > 0) SURFD_TRY(cub.reduce_sum(vflag, scal + 2, V, st));
    // OUT, IN
    for (int arriving = 0; arriving < 2; ++arriving) {
        SURFD_TRY(cub.sort_pairs(arriving ? ikey : okey, skey, eh, sh, H, 32, st));
        const long base = arriving ? H : 0;
        DEV_LAUNCH(ms_offsets_kernel, V + 1L, (const unsigned *)skey, (unsigned)H, V, (unsigned)base, arriving ? m->ioff : m->ooff);
        DEV_LAUNCH(ms_adjacency_kernel, H, (const int32_t *)m->tri, (const int *)sh, (const unsigned char *)hborder, H, arriving, m->nbr + base, m->opp + base);
    }
    // corners, ascending in (c, f) inside a vertex
    SURFD_TRY(cub.sort_pairs(ckey, skey, cpay, m->ch, H, 32, st));
    DEV_LAUNCH(ms_offsets_kernel, V + 1L, (const unsigned *)skey, (unsigned)H, V, 0u, m->coff);
    SURFD_TRY(read_words(scal, hs, 4, st));                   // the scratch is freed next
    m->n_border_vertices = hs[2];
    *out = owner.release();
    return SURFD_OK;
}

extern "C" void surfd_meshsmooth_destroy(surfd_meshsmooth *m) {
    if (m) ms_free(m);
}

extern "C" int surfd_meshsmooth_counts(const surfd_meshsmooth *m, int64_t *faces, int64_t *vertices, int64_t *border_halfedges, int64_t *border_vertices) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshsmooth_counts: null handle");
    if (faces) *faces = m->F;
    if (vertices) *vertices = m->V;
    if (border_halfedges) *border_halfedges = m->B;
    if (border_vertices) *border_vertices = m->n_border_vertices;
    return SURFD_OK;
}

namespace {

struct Buffers { double *a, *b; };

// the arena: positions A | positions B
int ms_buffers(surfd_meshsmooth *m, hipStream_t st, Buffers *out) {
    const size_t pos = ((size_t)m->V * 3 * sizeof(double) + 255) & ~(size_t)255;
    int rc = m->arena.reserve(std::max<size_t>(2 * pos, 256), st);
    if (rc != SURFD_OK) return rc;
    out->a = (double *)m->arena.ptr;
    out->b = (double *)((char *)m->arena.ptr + pos);
    return SURFD_OK;
}

// the caller's positions as fp64 in dst (exact)
int ms_import(const void *vertices, int dtype, long n, double *dst, hipStream_t st) {
    if (n == 0) return SURFD_OK;
    if (dtype == SURFD_MESHSMOOTH_F64) {
        if (vertices != (const void *)dst) HIP_TRY(hipMemcpyAsync(dst, vertices, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    } else {
        DEV_LAUNCH(ms_convert_kernel<float>, n, (const float *)vertices, n, dst);
    }
    return SURFD_OK;
}

int ms_sweep_args(const char *who, const surfd_meshsmooth *m, const void *vertices, int dtype, int steps, const double *out) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "%s: null handle", who);
    if (dtype != SURFD_MESHSMOOTH_F32 && dtype != SURFD_MESHSMOOTH_F64) SURFD_FAIL(SURFD_ERR_ARG, "%s: dtype %d is neither fp32 (0) nor fp64 (1)", who, dtype);
    if (steps < 0) SURFD_FAIL(SURFD_ERR_ARG, "%s: steps = %d must not be negative", who, steps);
    if (m->V > 0 && (!vertices || !out)) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    return SURFD_OK;
}

}  // namespace

extern "C" int surfd_meshsmooth_laplacian(surfd_meshsmooth *m, const void *vertices, int dtype, int steps, int cotangent, int boundary, double *out,
                                          surfd_stream s) {
    int rc = ms_sweep_args("surfd_meshsmooth_laplacian", m, vertices, dtype, steps, out);
    if (rc != SURFD_OK) return rc;
    const int V = m->V, H = 3 * m->F;
    if (V == 0) return SURFD_OK;
    hipStream_t st = as_stream(s);
    if (steps == 0 || H == 0) return ms_import(vertices, dtype, 3L * V, out, st);
    Buffers buf;
    if ((rc = ms_buffers(m, st, &buf)) != SURFD_OK) return rc;
    if ((rc = ms_import(vertices, dtype, 3L * V, buf.a, st)) != SURFD_OK) return rc;
    const unsigned char *vb = boundary ? m->vborder : nullptr;
    const double *src = buf.a;
    for (int i = 0; i < steps; ++i) {
        double *dst = i == steps - 1 ? out : (src == buf.a ? buf.b : buf.a);
        auto kernel = cotangent ? ms_laplacian_kernel<1> : ms_laplacian_kernel<0>;
        DEV_LAUNCH(kernel, V, src, dst, V, (const unsigned *)m->ooff, (const unsigned *)m->ioff, (const int *)m->nbr, (const int *)m->opp, vb);
        src = dst;
    }
    return SURFD_OK;
}

extern "C" int surfd_meshsmooth_umbrella(surfd_meshsmooth *m, const void *vertices, int dtype, double k0, double k1, int sweeps, int set, double *out,
                                         surfd_stream s) {
    int rc = ms_sweep_args("surfd_meshsmooth_umbrella", m, vertices, dtype, sweeps, out);
    if (rc != SURFD_OK) return rc;
    if (set != SURFD_MESHSMOOTH_ALL && set != SURFD_MESHSMOOTH_BORDER)
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshsmooth_umbrella: set %d is neither all (0) nor border (1)", set);
    const int V = m->V;
    if (V == 0) return SURFD_OK;
    hipStream_t st = as_stream(s);
    if (sweeps == 0 || m->F == 0 || (set == SURFD_MESHSMOOTH_BORDER && m->B == 0)) return ms_import(vertices, dtype, 3L * V, out, st);
    Buffers buf;
    if ((rc = ms_buffers(m, st, &buf)) != SURFD_OK) return rc;
    if ((rc = ms_import(vertices, dtype, 3L * V, buf.a, st)) != SURFD_OK) return rc;
    const bool border = set == SURFD_MESHSMOOTH_BORDER;
    const double *src = buf.a;
    for (int i = 0; i < sweeps; ++i) {
        double *dst = i == sweeps - 1 ? out : (src == buf.a ? buf.b : buf.a);
        DEV_LAUNCH(ms_umbrella_kernel, V, src, dst, V, (const unsigned *)(border ? m->boff : m->ooff), (const unsigned *)(border ? nullptr : m->ioff),
                   (const int *)(border ? m->bnbr : m->nbr), (i & 1) ? k1 : k0);
        src = dst;
    }
    return SURFD_OK;
}

extern "C" int surfd_meshsmooth_vertex_normals(surfd_meshsmooth *m, const void *vertices, int dtype, int weight, double *unit, double *raw, surfd_stream s) {
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshsmooth_vertex_normals: null handle");
    if (dtype != SURFD_MESHSMOOTH_F32 && dtype != SURFD_MESHSMOOTH_F64)
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshsmooth_vertex_normals: dtype %d is neither fp32 (0) nor fp64 (1)", dtype);
    if (weight != SURFD_MESHSMOOTH_ANGLE && weight != SURFD_MESHSMOOTH_AREA)
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshsmooth_vertex_normals: weight %d is neither angle (0) nor area (1)", weight);
    const int V = m->V;
    if (V == 0 || (!unit && !raw)) return SURFD_OK;
    if (!vertices) SURFD_FAIL(SURFD_ERR_ARG, "surfd_meshsmooth_vertex_normals: null argument");
    hipStream_t st = as_stream(s);
    if (m->F == 0) {
        if (unit) HIP_TRY(hipMemsetAsync(unit, 0, (size_t)V * 3 * sizeof(double), st));
        if (raw) HIP_TRY(hipMemsetAsync(raw, 0, (size_t)V * 3 * sizeof(double), st));
        return SURFD_OK;
    }
    const unsigned *coff = m->coff;
    const int *ch = m->ch;
    const int32_t *tri = m->tri;
    if (dtype == SURFD_MESHSMOOTH_F32) {
        if (weight == SURFD_MESHSMOOTH_ANGLE) DEV_LAUNCH((ms_normals_kernel<float, 1>), V, (const float *)vertices, tri, V, coff, ch, unit, raw);
        else DEV_LAUNCH((ms_normals_kernel<float, 0>), V, (const float *)vertices, tri, V, coff, ch, unit, raw);
    } else {
        if (weight == SURFD_MESHSMOOTH_ANGLE) DEV_LAUNCH((ms_normals_kernel<double, 1>), V, (const double *)vertices, tri, V, coff, ch, unit, raw);
        else DEV_LAUNCH((ms_normals_kernel<double, 0>), V, (const double *)vertices, tri, V, coff, ch, unit, raw);
    }
    return SURFD_OK;
}
