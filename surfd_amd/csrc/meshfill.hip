// Hole filling on the device: every border loop of up to max_edges edges is closed by its minimum-total-area triangulation
// (Barequet and Sharir 1995; the area term of Liepa 2003 without the dihedral one).  tests/meshfill_ref.py restates the contract
// sequentially in numpy; caps, their order, cap_loop and every count equal it bit for bit.  DESIGN.md section 8.20.
//
// Contract.  Vertices are fp64 [V, 3], faces int32 [F, 3], both on the device.
//   border   as meshclean.hip: half-edge 3 f + c runs t[f, c] -> t[f, (c + 1) % 3] and is a BORDER half-edge iff its unordered pair
//            occurs once among all 3 F half-edges (faces with repeated indices take part).  out(u) / in(u) count those leaving /
//            entering u; nxt(u) is where the one leads where out(u) == 1.
//   loops    u is REGULAR iff out(u) == 1 and in(u) == 1.  A loop is a cycle u0 -> nxt(u0) -> ... -> u0 of n >= 3 regular vertices,
//            listed from its smallest vertex u0; loops are numbered in ascending u0, those that stay open included.  Regular vertices
//            have one regular predecessor at most, so walks over them are disjoint chains and cycles.  A border half-edge on no loop
//            is irregular and stays open (bow-ties, borders of colliding directions).  n > max_edges: the loop stays open.
//   listing  r_m = u_((n - m) mod n), the border reversed (meshclean's rule): caps take the orientation of the faces round them.
//   DP       W[i][i+1] = 0; W[i][j] = min over i < k < j of S = (W[i][k] + W[k][j]) + A(i, k, j), a = P_k - P_i, b = P_j - P_i,
//            c = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), A = sqrt((c0 c0 + c1 c1) + c2 c2) * 0.5, fp64, every operation rounded
//            once (-ffp-contract=off).  The winner is the least (S, k) in the TOTAL order: a number before a NaN, the smaller S, the
//            smaller k.  The minimum under a total order is associative, so the split of the candidates over lanes changes no bit.
//            W[0][n-1] not finite: the loop stays open and is counted.
//   caps     n - 2 rows (r_i, r_k, r_j) in PREORDER: the triangle of (i, j), everything of (i, k), everything of (k, j); the row of a
//            node at slot s has its left child at s + 1 and its right child at s + 1 + (k - i - 1).  Filled loops in ascending number.
//
// Passes.
//   plan   mf_edge_keys -> sort -> mf_border_next (meshclean.hip's border pass with the in count) -> mf_init -> R rounds of mf_double (pointer
//          doubling over nxt between regular vertices, a non-regular vertex is a sink, the minimum vertex of the span rides along:
//          a vertex that has met no sink after 2^R >= V steps is on a cycle, and the minimum is the cycle's u0) -> mf_rank_init ->
//          R rounds of mf_rank (list ranking with the cycle cut at u0: d(u) = steps from u to u0, which is u's place m in the
//          reversed listing, and d(u0) = n) -> mf_flags -> five exclusive sums over V (loop number, filled-loop index, point base,
//          place in the short and the medium class) -> mf_scatter (per-loop records, the class lists in ascending loop order) ->
//          mf_gather (the listing's vertices and points, contiguous per loop: run needs no vertex array).  R = ceil(log2 V) and not
//          ceil(log2 max_edges) + 1: a loop longer than max_edges must be told from an open chain of that length to be counted.
//   run    mf_triangulate_kernel<NMAX, LANES, TableInLds> per class (short n <= 32: a wave per loop, four loops per workgroup;
//          medium n <= 128: a workgroup per loop; both with W and the splits in LDS; long n <= 1024: a workgroup per loop, W and the
//          splits in global scratch, in batches of ascending loops whose tables fit MF_TABLE_BUDGET) -> mf_ok_caps -> exclusive sum
//          -> mf_emit (rows staged at their planned place move up over the loops that turned out non-finite).
//          In the kernel spans d = 2 .. n - 1 are sequential, two workgroup barriers each.  The table is indexed (d, i) so that a
//          span is contiguous: lanes take consecutive i at one k - i, so both W reads of a wave are consecutive 8-byte words (no bank
//          conflict).  A span of fewer entries than lanes splits every entry's candidates over up to 32 lanes, reduced through LDS
//          in a fixed order.  Preorder slots are found by a stack walk of one lane per loop.
// Scratch: plan 72 F + 72 V bytes and hipcub's, freed when it returns; the handle keeps 28 V + 20 (V / 3 + 1) bytes; run 20 bytes per
// planned cap and 12 per loop, and for the long class min(loops, budget / table) tables of 10 n (n - 1) / 2 bytes, n the longest
// planned loop.  Host syncs: plan one, run one (none with nothing to fill).  No float atomics; integer ones only for counts.
// Bounds: arrays of V entries are indexed by the thread index below V, by destinations mf_border_next validated, and by positions
// from exclusive sums over V; the listing has at most V entries (loops are disjoint); per-loop arrays have V / 3 + 1 entries (a
// loop has three vertices at least); a class kernel sees only loops with n <= NMAX (the class flags) and drops any other; table
// indices are below n (n - 1) / 2; a cap row is compared against the caller's row count.  An index outside [0, V) is found in
// mf_edge_keys before anything is indexed by it: SURFD_ERR_ARG.
#include "common.h"
#include "devscratch.h"
#include "meshscene.h"
#include <cmath>
#include <type_traits>

namespace surfd {

constexpr int MF_MAX_EDGES = 1024, MF_SHORT = 32, MF_MEDIUM = 128, MF_PARTS = 32;
constexpr size_t MF_TABLE_BUDGET = (size_t)256 << 20;         // bytes of global tables of the long class in flight
enum { MF_BAD = 0, MF_BORDER, MF_LOOP_EDGES, MF_LOOPS, MF_TOO_LONG, MF_FILL, MF_POINTS, MF_N0, MF_N1, MF_LONGEST, MF_NONFINITE, MF_CAPS, MF_BROKEN, MF_WORDS = 16 };

// ---- plan -----------------------------------------------------------------------------------------------------------------------
// The border pass is meshclean.hip's (mc_edge_keys, mc_border_next) with the count of the half-edges that ENTER a vertex beside it.
// Indices are compared and packed here, never used as addresses.
__global__ void mf_edge_keys_kernel(const int32_t *__restrict__ faces, int F, int V, int bits, unsigned long long *__restrict__ key, int *__restrict__ eh,
                                    int *__restrict__ cnt) {
    if (dev_tid() >= F) return;
    const long f = dev_tid();
    const int t[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    if (t[0] < 0 || t[0] >= V || t[1] < 0 || t[1] >= V || t[2] < 0 || t[2] >= V) cnt[MF_BAD] = 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int a = t[c], b = t[(c + 1) % 3];
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        key[3 * f + c] = ((unsigned long long)(unsigned)hi << bits) | (unsigned long long)(unsigned)lo;      // both below 2^bits where the flag stays down
        eh[3 * f + c] = (int)(3 * f + c);
    }
}

// per sorted position: a key that neither neighbour shares is a border half-edge u -> w; it counts at u and at w and records w
__global__ void mf_border_next_kernel(const unsigned long long *__restrict__ skey, const int *__restrict__ sh, const int32_t *__restrict__ faces, int n, int V,
                                      int *outcnt, int *incnt, int *__restrict__ nxt) {
    if (dev_tid() >= n) return;
    const int i = (int)dev_tid();
    const unsigned long long k = skey[i];
    if ((i > 0 && skey[i - 1] == k) || (i < n - 1 && skey[i + 1] == k)) return;
    const int h = sh[i], f = h / 3, c = h - 3 * f;
    const int u = faces[h], w = faces[3 * (long)f + (c + 1) % 3];
    if (u < 0 || u >= V || w < 0 || w >= V) return;             // the flag is up already (mf_edge_keys_kernel)
    atomicAdd(outcnt + u, 1);                                   // integer counts have no order
    atomicAdd(incnt + w, 1);
    nxt[u] = w;                                                 // read only where outcnt[u] == 1: this lane was the only writer
}

__global__ void mf_init_kernel(int V, const int *__restrict__ outcnt, const int *__restrict__ incnt, const int *__restrict__ nxt, int *__restrict__ ptr,
                               int *__restrict__ mn) {
    if (dev_tid() >= V) return;
    const int u = (int)dev_tid();
    int p = -1;
    if (outcnt[u] == 1 && incnt[u] == 1) {
        const int w = nxt[u];                                  // a validated destination: this vertex's one border half-edge wrote it
        if (outcnt[w] == 1 && incnt[w] == 1) p = w;
    }
    ptr[u] = p;                                                // -1: the walk from u has left the regular vertices
    mn[u] = u;
}

__global__ void mf_double_kernel(int V, const int *__restrict__ ptr, const int *__restrict__ mn, int *__restrict__ ptr2, int *__restrict__ mn2) {
    if (dev_tid() >= V) return;
    const int u = (int)dev_tid(), p = ptr[u];
    ptr2[u] = p < 0 ? -1 : ptr[p];
    mn2[u] = p < 0 ? mn[u] : min(mn[u], mn[p]);
}

// in place: (ptr, mn) of the last doubling round become (q, d) of the ranking; head[u] = u0 of u's cycle, -1 off the cycles
__global__ void mf_rank_init_kernel(int V, const int *__restrict__ nxt, int *__restrict__ q, int *__restrict__ d, int *__restrict__ head) {
    if (dev_tid() >= V) return;
    const int u = (int)dev_tid();
    if (q[u] < 0) { head[u] = -1; d[u] = 0; return; }
    const int h = d[u], w = nxt[u];
    head[u] = h;
    q[u] = w == h ? -1 : w;                                    // the cycle is cut in front of its head
    d[u] = 1;
}

__global__ void mf_rank_kernel(int V, const int *__restrict__ q, const int *__restrict__ d, int *__restrict__ q2, int *__restrict__ d2) {
    if (dev_tid() >= V) return;
    const int u = (int)dev_tid(), p = q[u];
    q2[u] = p < 0 ? -1 : q[p];
    d2[u] = p < 0 ? d[u] : d[u] + d[p];
}

// per vertex: the flags of a loop's head (all others 0), and the counts that have no order
__global__ void mf_flags_kernel(int V, const int *__restrict__ head, const int *__restrict__ d, int max_edges, int *__restrict__ isloop, int *__restrict__ fill,
                                int *__restrict__ nfill, int *__restrict__ c0, int *__restrict__ c1, int *cnt) {
    if (dev_tid() >= V) return;
    const int u = (int)dev_tid();
    const int n = head[u] == u ? d[u] : 0;
    const int loop = n >= 3, f = loop && n <= max_edges;
    isloop[u] = loop;
    fill[u] = f;
    nfill[u] = f ? n : 0;
    c0[u] = f && n <= MF_SHORT;
    c1[u] = f && n > MF_SHORT && n <= MF_MEDIUM;
    if (loop) {
        atomicAdd(cnt + MF_LOOP_EDGES, n);
        if (f) atomicMax(cnt + MF_LONGEST, n); else atomicAdd(cnt + MF_TOO_LONG, 1);
    }
}

__global__ void mf_scatter_kernel(int V, const int *__restrict__ head, const int *__restrict__ d, const int *__restrict__ fill, const int *__restrict__ loopnum,
                                  const int *__restrict__ jidx, const int *__restrict__ base, const int *__restrict__ c0, const int *__restrict__ c1,
                                  const int *__restrict__ p0, const int *__restrict__ p1, const int *__restrict__ cnt, int *__restrict__ all_n,
                                  int *__restrict__ fl_n, int *__restrict__ fl_base, int *__restrict__ fl_num, int *__restrict__ list) {
    if (dev_tid() >= V) return;
    const int u = (int)dev_tid();
    if (head[u] != u || d[u] < 3) return;
    const int n = d[u], num = loopnum[u];
    all_n[num] = n;
    if (!fill[u]) return;
    const int j = jidx[u];
    fl_n[j] = n; fl_base[j] = base[u]; fl_num[j] = num;
    const int n0 = cnt[MF_N0], n1 = cnt[MF_N1];               // written by the scans in front of this launch
    list[c0[u] ? p0[u] : c1[u] ? n0 + p1[u] : n0 + n1 + (j - p0[u] - p1[u])] = j;
}

__global__ void mf_gather_kernel(int V, const double *__restrict__ vertices, const int *__restrict__ head, const int *__restrict__ d, const int *__restrict__ fill,
                                 const int *__restrict__ base, int *__restrict__ rvert, double *__restrict__ pts) {
    if (dev_tid() >= V) return;
    const long u = dev_tid();
    const int h = head[u];
    if (h < 0 || !fill[h]) return;
    const long slot = (long)base[h] + (u == h ? 0 : d[u]);     // d(u) = steps to the head = the place in the reversed listing
    rvert[slot] = (int)u;
#pragma unroll
    for (int c = 0; c < 3; ++c) pts[3 * slot + c] = vertices[3 * u + c];
}

// ---- run ------------------------------------------------------------------------------------------------------------------------
// (s, k) before (bs, bk): a number before a NaN, the smaller sum, the smaller k
__device__ __forceinline__ bool mf_better(double s, int k, double bs, int bk) {
    const bool ns = s != s, nb = bs != bs;
    if (ns != nb) return nb;
    if (!ns && s != bs) return s < bs;
    return k < bk;
}

template <int NMAX>
using mf_split_t = typename std::conditional<(NMAX <= 256), unsigned char, unsigned short>::type;

template <int NMAX, int LANES, bool TableInLds>
constexpr size_t mf_group_bytes() {
    const size_t tri = (size_t)NMAX * (NMAX - 1) / 2;
    const size_t b = (TableInLds ? tri * 8 : 0) + (size_t)LANES * 8 + 3 * (size_t)NMAX * 8 + (size_t)LANES * 4 + (size_t)NMAX * 4 +
                     (TableInLds ? tri * sizeof(mf_split_t<NMAX>) : 0);
    return (b + 7) & ~(size_t)7;
}

// list[begin .. end): the loops of this launch, one per group of LANES lanes.  gT / gK (TableInLds = false): one table of
// table_entries entries per workgroup of the launch.
template <int NMAX, int LANES, bool TableInLds>
__global__ void __launch_bounds__(256) mf_triangulate_kernel(const int *__restrict__ list, int begin, int end, const int *__restrict__ fl_n,
                                                             const int *__restrict__ fl_base, const double *__restrict__ pts, const int *__restrict__ rvert,
                                                             double *gT, mf_split_t<NMAX> *gK, long table_entries, int32_t *__restrict__ stage,
                                                             int *__restrict__ stage_j, int *__restrict__ ok, int *cnt) {
    typedef mf_split_t<NMAX> split_t;
    constexpr int GROUPS = 256 / LANES, TRI = NMAX * (NMAX - 1) / 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char mf_lds[];
    const int grp = threadIdx.x / LANES, g = threadIdx.x - grp * LANES;
    unsigned char *mine = mf_lds + (size_t)grp * mf_group_bytes<NMAX, LANES, TableInLds>();
    double *T = (double *)mine;
    double *redS = T + (TableInLds ? TRI : 0);
    double *P = redS + LANES;
    int *redK = (int *)(P + 3 * NMAX);
    unsigned *stack = (unsigned *)(redK + LANES);
    split_t *K = (split_t *)(stack + NMAX);
    if (!TableInLds) {
        T = gT + (long)blockIdx.x * table_entries;
        K = gK + (long)blockIdx.x * table_entries;
    }
    const int item = begin + (int)blockIdx.x * GROUPS + grp;
    const int j = item < end ? list[item] : -1;
    int n = j >= 0 ? fl_n[j] : 0;
    if (n > NMAX) n = 0;                                       // the class flags admit none
    const int base = j >= 0 ? fl_base[j] : 0;
    int nmax = n;                                              // of the workgroup: every wave meets every barrier
    if (GROUPS > 1) {
        nmax = 0;
        for (int t = 0; t < GROUPS; ++t) {
            const int it = begin + (int)blockIdx.x * GROUPS + t;
            const int nt = it < end ? fl_n[list[it]] : 0;
            nmax = max(nmax, nt <= NMAX ? nt : 0);
        }
    }
    for (int t = g; t < 3 * n; t += LANES) P[t] = pts[3 * (long)base + t];
    for (int t = g; t < n - 1; t += LANES) T[t] = 0.0;         // the span d = 1
    __syncthreads();
    auto off = [n](int d) { return (d - 1) * n - (d - 1) * d / 2; };      // where span d starts: spans 1 .. d - 1 have n - 1 .. n - d + 1 entries
    // the least (S, k) of entry (i, i + d) over the candidates e = e0, e0 + step, ... (k = i + e)
    auto entry = [&](int i, int d, int e0, int step, double &bs, int &bk) {
        const int jj = i + d;
        const double pix = P[3 * i], piy = P[3 * i + 1], piz = P[3 * i + 2];
        const double bx = P[3 * jj] - pix, by = P[3 * jj + 1] - piy, bz = P[3 * jj + 2] - piz;
        bs = NAN; bk = n;
        for (int e = e0; e < d; e += step) {
            const int k = i + e;
            const double ax = P[3 * k] - pix, ay = P[3 * k + 1] - piy, az = P[3 * k + 2] - piz;
            const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
            const double a = sqrt((cx * cx + cy * cy) + cz * cz) * 0.5;
            const double s = (T[off(e) + i] + T[off(d - e) + k]) + a;
            if (mf_better(s, k, bs, bk)) { bs = s; bk = k; }
        }
    };
    for (int d = 2; d < nmax; ++d) {
        const int E = n - d;                                   // entries of the span; <= 0 once this group's loop is done
        int parts = 1;                                         // lanes per entry
        if (E > 0) {
            if (E < LANES) parts = min(min(LANES / E, d - 1), MF_PARTS);
            if (parts == 1) {
                for (int i = g; i < E; i += LANES) {
                    double bs; int bk;
                    entry(i, d, 1, 1, bs, bk);
                    T[off(d) + i] = bs; K[off(d) + i] = (split_t)bk;
                }
            } else {
                const int part = g / E, i = g - part * E;
                if (part < parts) {                            // parts <= d - 1: every part has a candidate
                    double bs; int bk;
                    entry(i, d, 1 + part, parts, bs, bk);
                    redS[g] = bs; redK[g] = bk;
                }
            }
        }
        __syncthreads();
        if (E > 0 && parts > 1 && g < E) {
            double bs = redS[g]; int bk = redK[g];
            for (int p = 1; p < parts; ++p) {
                const double s = redS[g + p * E]; const int k = redK[g + p * E];
                if (mf_better(s, k, bs, bk)) { bs = s; bk = k; }
            }
            T[off(d) + g] = bs; K[off(d) + g] = (split_t)bk;
        }
        __syncthreads();
    }
    if (g != 0 || n < 3) return;
    const bool fin = isfinite(T[off(n - 1)]);
    ok[j] = fin ? 1 : 0;
    if (!fin) { atomicAdd(cnt + MF_NONFINITE, 1); return; }
    atomicMax(cnt + MF_LONGEST, n);
    // preorder by a stack of (i, j, slot), ten bits each: the right child is pushed first
    const long row0 = (long)base - 2L * j;                     // the planned place: every filled loop before this one has n - 2 rows
    int sp = 0;
    stack[sp++] = (unsigned)(n - 1) << 10;
    while (sp > 0) {
        const unsigned w = stack[--sp];
        const int ii = w & 1023, jj = (w >> 10) & 1023, s = w >> 20;
        const int k = K[off(jj - ii) + ii];
        if (k <= ii || k >= jj || s >= n - 2 || sp + 2 > NMAX) {    // cannot happen on a finite table: the loop gives no row and the call fails
            ok[j] = 0;
            cnt[MF_BROKEN] = 1;
            break;
        }
        const long row = row0 + s;
        stage[3 * row] = rvert[base + ii]; stage[3 * row + 1] = rvert[base + k]; stage[3 * row + 2] = rvert[base + jj];
        stage_j[row] = j;
        if (jj - k >= 2) stack[sp++] = (unsigned)k | (unsigned)jj << 10 | (unsigned)(s + 1 + (k - ii - 1)) << 20;
        if (k - ii >= 2) stack[sp++] = (unsigned)ii | (unsigned)k << 10 | (unsigned)(s + 1) << 20;
    }
}

__global__ void mf_ok_caps_kernel(int L, const int *__restrict__ ok, const int *__restrict__ fl_n, int *__restrict__ okc) {
    if (dev_tid() >= L) return;
    okc[dev_tid()] = ok[dev_tid()] ? fl_n[dev_tid()] - 2 : 0;
}

// a staged row moves up by the rows of the non-finite loops in front of its loop
__global__ void mf_emit_kernel(int rows, const int32_t *__restrict__ stage, const int *__restrict__ stage_j, const int *__restrict__ ok, const int *__restrict__ fl_base,
                               const int *__restrict__ fl_num, const int *__restrict__ foff, long cap_rows, int32_t *__restrict__ caps, int32_t *__restrict__ cap_loop) {
    if (dev_tid() >= rows) return;
    const long s = dev_tid();
    const int j = stage_j[s];
    if (j < 0 || !ok[j]) return;
    const long dst = (long)foff[j] + (s - ((long)fl_base[j] - 2L * j));
    if (dst < 0 || dst >= cap_rows) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) caps[3 * dst + c] = stage[3 * s + c];
    if (cap_loop) cap_loop[dst] = fl_num[j];
}

}  // namespace surfd

using namespace surfd;

struct surfd_meshfill {
    int V = 0, F = 0, max_edges = 0;
    int loops = 0, fill = 0, n0 = 0, n1 = 0, n2 = 0, points = 0, caps = 0, longest = 0;
    int64_t counts[7] = {0, 0, 0, 0, 0, 0, 0};
    char *block = nullptr;                                     // the arrays below, one allocation
    int *rvert = nullptr, *fl_n = nullptr, *fl_base = nullptr, *fl_num = nullptr, *list = nullptr, *all_n = nullptr;
    double *pts = nullptr;
};

namespace surfd {

template <int NMAX, int LANES, bool TableInLds>
static int mf_launch(const surfd_meshfill *m, int begin, int end, double *gT, void *gK, long table_entries, int32_t *stage, int *stage_j, int *ok, int *cnt,
                     hipStream_t st) {
    constexpr int GROUPS = 256 / LANES;
    constexpr size_t lds = GROUPS * mf_group_bytes<NMAX, LANES, TableInLds>();
    static_assert(lds <= 160 * 1024, "the tables of a workgroup must fit the LDS of a CU");
    if (end <= begin) return SURFD_OK;
    auto kernel = mf_triangulate_kernel<NMAX, LANES, TableInLds>;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(end - begin, GROUPS)), dim3(256), lds, st, (const int *)m->list, begin, end, (const int *)m->fl_n,
                       (const int *)m->fl_base, (const double *)m->pts, (const int *)m->rvert, gT, (mf_split_t<NMAX> *)gK, table_entries, stage, stage_j, ok, cnt);
    LAUNCH_CHECK();
    return SURFD_OK;
}

static void mf_free(surfd_meshfill *m) {
    if (!m) return;
    if (m->block) (void)hipFree(m->block);
    delete m;
}

}  // namespace surfd

extern "C" int surfd_meshfill_plan(const double *vertices, int V, const int32_t *faces, int F, int max_edges, int64_t *counts, surfd_stream s,
                                   surfd_meshfill **out) {
    const char *who = "surfd_meshfill_plan";
    if (!counts || !out) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    for (int i = 0; i < 7; ++i) counts[i] = 0;
    SURFD_TRY(mesh_sizes(who, F, V));
    if (max_edges < 3 || max_edges > MF_MAX_EDGES) SURFD_FAIL(SURFD_ERR_ARG, "%s: max_edges = %d must lie in [3, %d]", who, max_edges, MF_MAX_EDGES);
    std::unique_ptr<surfd_meshfill, void (*)(surfd_meshfill *)> m(new surfd_meshfill, mf_free);
    m->V = V; m->F = F; m->max_edges = max_edges;
    if (F == 0 || V == 0) { *out = m.release(); return SURFD_OK; }
    if (!vertices || !faces) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    hipStream_t st = as_stream(s);
    const long L = V / 3 + 1;                                  // loops are disjoint and have three vertices at least
    {
        ScratchArena own("meshfill");
        const size_t bytes = dev_slot<double>(3L * V) + dev_slot<int>(V) + 5 * dev_slot<int>(L);
        HIP_TRY(hipMalloc((void **)&m->block, bytes));
        own.adopt(m->block, bytes);
        SURFD_TRY(own.get(&m->pts, 3L * V)); SURFD_TRY(own.get(&m->rvert, V)); SURFD_TRY(own.get(&m->fl_n, L)); SURFD_TRY(own.get(&m->fl_base, L));
        SURFD_TRY(own.get(&m->fl_num, L)); SURFD_TRY(own.get(&m->list, L)); SURFD_TRY(own.get(&m->all_n, L));
    }
    DeviceScratch scratch;
    CubWorkspace cub{&scratch};
    const int H = 3 * F;
    int *cnt, *eh, *sh, *outcnt, *incnt, *nxt, *pa, *pb, *ma, *mb, *head, *isloop, *fill, *nfill, *c0, *c1, *loopnum, *jidx, *base, *p0, *p1;
    unsigned long long *key, *skey;
    ScratchArena arena("meshfill");
    SURFD_TRY(arena.open(scratch, dev_slot<int>(MF_WORDS) + 2 * dev_slot<unsigned long long>(H) + 2 * dev_slot<int>(H) + 18 * dev_slot<int>(V)));
    SURFD_TRY(zeroed_words(arena, &cnt, MF_WORDS, st));
    SURFD_TRY(arena.get(&key, H)); SURFD_TRY(arena.get(&skey, H)); SURFD_TRY(arena.get(&eh, H)); SURFD_TRY(arena.get(&sh, H));
    SURFD_TRY(arena.get(&outcnt, V)); SURFD_TRY(arena.get(&incnt, V)); SURFD_TRY(arena.get(&nxt, V));
    SURFD_TRY(arena.get(&pa, V)); SURFD_TRY(arena.get(&pb, V)); SURFD_TRY(arena.get(&ma, V)); SURFD_TRY(arena.get(&mb, V)); SURFD_TRY(arena.get(&head, V));
    SURFD_TRY(arena.get(&isloop, V)); SURFD_TRY(arena.get(&fill, V)); SURFD_TRY(arena.get(&nfill, V)); SURFD_TRY(arena.get(&c0, V)); SURFD_TRY(arena.get(&c1, V));
    SURFD_TRY(arena.get(&loopnum, V)); SURFD_TRY(arena.get(&jidx, V)); SURFD_TRY(arena.get(&base, V)); SURFD_TRY(arena.get(&p0, V)); SURFD_TRY(arena.get(&p1, V));
    HIP_TRY(hipMemsetAsync(outcnt, 0, 3 * dev_slot<int>(V), st));      // outcnt, incnt, nxt: three slots in a row
    int bits = 1;                                              // of an index below V: the keys take 2 bits of the radix sort, not 64
    while (bits < 31 && (1L << bits) < V) ++bits;
    DEV_LAUNCH(mf_edge_keys_kernel, F, faces, F, V, bits, key, eh, cnt);
    SURFD_TRY(cub.sort_pairs(key, skey, eh, sh, H, 2 * bits, st));
    DEV_LAUNCH(mf_border_next_kernel, H, (const unsigned long long *)skey, (const int *)sh, faces, H, V, outcnt, incnt, nxt);
    SURFD_TRY(cub.reduce_sum(outcnt, cnt + MF_BORDER, V, st));
    int rounds = 0;                                            // 2^rounds >= V: a walk of that many steps has met a sink or gone round its cycle
    while (rounds < 31 && (1L << rounds) < V) ++rounds;
    DEV_LAUNCH(mf_init_kernel, V, V, (const int *)outcnt, (const int *)incnt, (const int *)nxt, pa, ma);
    for (int r = 0; r < rounds; ++r) {
        DEV_LAUNCH(mf_double_kernel, V, V, (const int *)pa, (const int *)ma, pb, mb);
        std::swap(pa, pb); std::swap(ma, mb);
    }
    DEV_LAUNCH(mf_rank_init_kernel, V, V, (const int *)nxt, pa, ma, head);
    for (int r = 0; r < rounds; ++r) {
        DEV_LAUNCH(mf_rank_kernel, V, V, (const int *)pa, (const int *)ma, pb, mb);
        std::swap(pa, pb); std::swap(ma, mb);
    }
    const int *d = ma;
    DEV_LAUNCH(mf_flags_kernel, V, V, (const int *)head, d, max_edges, isloop, fill, nfill, c0, c1, cnt);
    SURFD_TRY(cub.exclusive_sum(isloop, loopnum, V, st)); SURFD_TRY(scan_total(isloop, loopnum, V, cnt + MF_LOOPS, st));
    SURFD_TRY(cub.exclusive_sum(fill, jidx, V, st));      SURFD_TRY(scan_total(fill, jidx, V, cnt + MF_FILL, st));
    SURFD_TRY(cub.exclusive_sum(nfill, base, V, st));     SURFD_TRY(scan_total(nfill, base, V, cnt + MF_POINTS, st));
    SURFD_TRY(cub.exclusive_sum(c0, p0, V, st));          SURFD_TRY(scan_total(c0, p0, V, cnt + MF_N0, st));
    SURFD_TRY(cub.exclusive_sum(c1, p1, V, st));          SURFD_TRY(scan_total(c1, p1, V, cnt + MF_N1, st));
    DEV_LAUNCH(mf_scatter_kernel, V, V, (const int *)head, d, (const int *)fill, (const int *)loopnum, (const int *)jidx, (const int *)base, (const int *)c0,
               (const int *)c1, (const int *)p0, (const int *)p1, (const int *)cnt, m->all_n, m->fl_n, m->fl_base, m->fl_num, m->list);
    DEV_LAUNCH(mf_gather_kernel, V, V, vertices, (const int *)head, d, (const int *)fill, (const int *)base, m->rvert, m->pts);
    int hc[MF_WORDS];
    SURFD_TRY(read_words(cnt, hc, MF_WORDS, st));
    if (hc[MF_BAD]) return mesh_bad_index(who, V);
    m->loops = hc[MF_LOOPS]; m->fill = hc[MF_FILL]; m->points = hc[MF_POINTS]; m->longest = hc[MF_LONGEST];
    m->n0 = hc[MF_N0]; m->n1 = hc[MF_N1]; m->n2 = m->fill - m->n0 - m->n1;
    m->caps = m->points - 2 * m->fill;
    m->counts[0] = m->fill;                                  // loops_filled
    m->counts[1] = m->caps;                                  // caps
    m->counts[2] = hc[MF_TOO_LONG];                          // loops_too_long
    m->counts[3] = 0;                                        // loops_nonfinite: known after run
    m->counts[4] = (int64_t)hc[MF_BORDER] - hc[MF_LOOP_EDGES];      // irregular_border_edges
    m->counts[5] = hc[MF_BORDER];                            // border_edges
    m->counts[6] = m->longest;                               // longest_filled
    for (int i = 0; i < 7; ++i) counts[i] = m->counts[i];
    *out = m.release();
    return SURFD_OK;
}

extern "C" int surfd_meshfill_loop_sizes(const surfd_meshfill *m, int32_t *sizes, int64_t rows, surfd_stream s) {
    const char *who = "surfd_meshfill_loop_sizes";
    if (!m) SURFD_FAIL(SURFD_ERR_ARG, "%s: null handle", who);
    if (rows < m->loops || (m->loops > 0 && !sizes)) SURFD_FAIL(SURFD_ERR_ARG, "%s: sizes must have room for %d loops, got %lld", who, m->loops, (long long)rows);
    if (m->loops > 0) HIP_TRY(hipMemcpyAsync(sizes, m->all_n, (size_t)m->loops * sizeof(int32_t), hipMemcpyDeviceToDevice, as_stream(s)));
    return SURFD_OK;
}

extern "C" int surfd_meshfill_run(surfd_meshfill *m, int32_t *caps, int64_t cap_rows, int32_t *cap_loop, int64_t *counts, surfd_stream s) {
    const char *who = "surfd_meshfill_run";
    if (!m || !counts) SURFD_FAIL(SURFD_ERR_ARG, "%s: null argument", who);
    for (int i = 0; i < 7; ++i) counts[i] = m->counts[i];
    if (cap_rows < m->caps || (m->caps > 0 && !caps))
        SURFD_FAIL(SURFD_ERR_ARG, "%s: caps must have room for the %d planned rows, got %lld", who, m->caps, (long long)cap_rows);
    if (m->fill == 0) return SURFD_OK;
    hipStream_t st = as_stream(s);
    DeviceScratch scratch;
    CubWorkspace cub{&scratch};
    int *cnt, *stage_j, *ok, *okc, *foff;
    int32_t *stage;
    ScratchArena arena("meshfill");
    SURFD_TRY(arena.open(scratch, dev_slot<int>(MF_WORDS) + dev_slot<int32_t>(3L * m->caps) + dev_slot<int>(m->caps) + 3 * dev_slot<int>(m->fill)));
    SURFD_TRY(zeroed_words(arena, &cnt, MF_WORDS, st));
    SURFD_TRY(arena.get(&stage, 3L * m->caps)); SURFD_TRY(arena.get(&stage_j, m->caps));
    SURFD_TRY(arena.get(&ok, m->fill)); SURFD_TRY(arena.get(&okc, m->fill)); SURFD_TRY(arena.get(&foff, m->fill));
    HIP_TRY(hipMemsetAsync(stage_j, 0xff, dev_bytes<int>(m->caps), st));      // -1: no row staged
    HIP_TRY(hipMemsetAsync(ok, 0, dev_bytes<int>(m->fill), st));
    SURFD_TRY((mf_launch<MF_SHORT, 64, true>(m, 0, m->n0, nullptr, nullptr, 0, stage, stage_j, ok, cnt, st)));
    SURFD_TRY((mf_launch<MF_MEDIUM, 256, true>(m, m->n0, m->n0 + m->n1, nullptr, nullptr, 0, stage, stage_j, ok, cnt, st)));
    if (m->n2 > 0) {
        const long entries = ((long)m->longest * (m->longest - 1) / 2 + 31) & ~31L;      // per table; the longest planned loop is in this class
        const long tables = std::min<long>(m->n2, std::max<long>(1, (long)(MF_TABLE_BUDGET / ((size_t)entries * 10))));
        double *gT; unsigned short *gK;
        ScratchArena big("meshfill");
        SURFD_TRY(big.open(scratch, dev_slot<double>(entries * tables) + dev_slot<unsigned short>(entries * tables)));
        SURFD_TRY(big.get(&gT, entries * tables)); SURFD_TRY(big.get(&gK, entries * tables));
        for (long b = 0; b < m->n2; b += tables) {
            const int begin = m->n0 + m->n1 + (int)b, end = begin + (int)std::min<long>(tables, m->n2 - b);
            SURFD_TRY((mf_launch<MF_MAX_EDGES, 256, false>(m, begin, end, gT, gK, entries, stage, stage_j, ok, cnt, st)));
        }
    }
    DEV_LAUNCH(mf_ok_caps_kernel, m->fill, m->fill, (const int *)ok, (const int *)m->fl_n, okc);
    SURFD_TRY(cub.exclusive_sum(okc, foff, m->fill, st));
    SURFD_TRY(scan_total(okc, foff, m->fill, cnt + MF_CAPS, st));
    if (m->caps > 0)
        DEV_LAUNCH(mf_emit_kernel, m->caps, m->caps, (const int32_t *)stage, (const int *)stage_j, (const int *)ok, (const int *)m->fl_base, (const int *)m->fl_num,
                   (const int *)foff, (long)cap_rows, caps, cap_loop);
    int hc[MF_WORDS];
    SURFD_TRY(read_words(cnt, hc, MF_WORDS, st));
    counts[0] = m->fill - hc[MF_NONFINITE];
    counts[1] = hc[MF_CAPS];
    counts[3] = hc[MF_NONFINITE];
    counts[6] = hc[MF_LONGEST];
    if (hc[MF_BROKEN]) SURFD_FAIL(SURFD_ERR_STATE, "%s: a split table does not describe a triangulation (rows of that loop were not written)", who);
    return SURFD_OK;
}

extern "C" void surfd_meshfill_destroy(surfd_meshfill *m) { mf_free(m); }
