// The auto-encoder's point-cloud encoder, Dgcnn (reference AutoEncoder/models/dgcnn.py:9-115), in eval mode: self-kNN over
// the cloud, four EdgeConv blocks, conv_5 + BN + leaky-ReLU + max over the points.  Plain fp32 throughout.
//
//   dg_knn_kernel        — brute-force self-kNN.  256 queries per workgroup (one per lane); the candidates of one split of
//                          the cloud stream through LDS in tiles of 256 points; each lane keeps its K nearest (distance,
//                          index) pairs sorted in registers (fully unrolled compare-and-shift, no dynamically indexed array).
//                          A cloud is split over S workgroups per query block so that one 10 000-point cloud fills the chip.
//   dg_knn_merge_kernel  — merges the S sorted partial lists of a query in split order (fixed, so deterministic).
//   dg_linear_kernel     — Y = X W^T on v_mfma_f32_32x32x2_f32 (64 x 64 tile per workgroup, one 32 x 32 tile per wave).
//                          For blocks 1-4 W = [W1 ; W2 - W1] and Y = [P | Q] (see below).  For conv_5 (REDUCE) the
//                          per-point output is never written: the epilogue keeps each channel's max and min over the
//                          tile's rows and writes them as per-tile partials.
//   dg_edge_kernel       — per point and channel: max (or min) over the K neighbours of P[j], then BN + leaky-ReLU once.
//   dg_global_kernel     — reduces conv_5's per-tile partials over the cloud and applies BN5 + leaky-ReLU: feat[B, L].
//
// EdgeConv factorisation.  The reference evaluates, for every edge (i, j_k), W [x_j - x_i ; x_i] with W = [W1 | W2]
// (dgcnn.py:9-24,60).  W [a - b ; b] = W1 a + (W2 - W1) b, so one per-point GEMM gives P = x W1^T and Q = x (W2 - W1)^T
// and every edge value is P[j] + Q[i]: K times fewer multiply-adds than the per-edge Linear, and no B x N x K x 2D tensor.
//
// Monotone reduction.  Eval-mode BN folded to y = s v + t (s = w / sqrt(var + eps), t = b - mean s) followed by leaky-ReLU
// (slope 0.2) is, per channel, a non-decreasing function of v where s >= 0 and a non-increasing one where s < 0; the
// per-edge value v = P[j] + Q[i] is non-decreasing in P[j].  Every step is a correctly rounded fp32 operation, and rounding is
// monotone too, so the composition stays monotone in P[j] after rounding.  Hence
//     max_k lrelu(s (P[j_k] + Q[i]) + t) = lrelu(s (max_k P[j_k] + Q[i]) + t)      (s >= 0; min_k where s < 0)
// bit for bit (when s = t = 0 every edge gives a zero, and only the sign of that zero may differ).  The same argument lets
// conv_5 reduce max / min over the points BEFORE BN5 + leaky-ReLU, which then run on B x L values only.
//
// Hazards: the only LDS reuse is the candidate tile of dg_knn_kernel and the staging tiles of dg_linear_kernel, each
// bracketed by __syncthreads() on both sides (every reader of the previous tile is past the barrier before a lane
// overwrites it); cross-lane values move with __shfl_xor only (the compiler places the waits for ds_bpermute).
#include "common.h"
#include "paramtable.h"
#include <cfloat>
#include <cmath>
#include <cstring>
#include <algorithm>
#include <utility>
#include <type_traits>

namespace surfd {

constexpr int DG_TILE = 256;        // kNN: candidates per LDS tile, and queries per workgroup
constexpr int DG_KMAX = 32;
constexpr int DG_FEAT = 512;        // x1..x4 concatenated: 64 + 64 + 128 + 256
constexpr int DG_DIN[4] = {3, 64, 64, 128};
constexpr int DG_DOUT[4] = {64, 64, 128, 256};
constexpr int DG_XOFF[4] = {0, 64, 128, 256};

// Compile-time loop: f(std::integral_constant<int, I>) for I = 0 .. N-1, so that every index into a register array is a
// constant (a dynamically indexed array is placed in scratch memory).
template <typename F, int... I>
__device__ __forceinline__ void dg_unroll_impl(F &&f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void dg_unroll(F &&f) { dg_unroll_impl(f, std::make_integer_sequence<int, N>{}); }

// Sorted (ascending distance, then ascending index) insertion of (dn, jn) into a list of KT entries held in registers.
// Callers insert in ascending index order among equal distances, so "shift the entries strictly greater than dn" keeps the
// (distance, index) order: an equal distance that is already there has the lower index and stays in front.
template <int KT>
__device__ __forceinline__ void dg_insert(float (&d)[KT], int (&id)[KT], float dn, int jn) {
    dg_unroll<KT - 1>([&](auto I) {                        // slots KT-1 down to 1: reads the old values of slots i and i - 1
        constexpr int i = KT - 1 - decltype(I)::value;
        const bool gt = d[i] > dn, sh = d[i - 1] > dn;
        d[i] = gt ? (sh ? d[i - 1] : dn) : d[i];
        id[i] = gt ? (sh ? id[i - 1] : jn) : id[i];
    });
    if (d[0] > dn) { d[0] = dn; id[0] = jn; }
}

// d[k - 1] without indexing the register array dynamically
template <int KT>
__device__ __forceinline__ float dg_kth(const float (&d)[KT], int k) {
    float r = d[KT - 1];
    dg_unroll<KT - 1>([&](auto I) { r = (decltype(I)::value == k - 1) ? d[decltype(I)::value] : r; });
    return r;
}

template <int KT>
__device__ __forceinline__ void dg_init(float (&d)[KT], int (&id)[KT]) {
    dg_unroll<KT>([&](auto I) { d[decltype(I)::value] = INFINITY; id[decltype(I)::value] = -1; });
}

// pts [B, N, 3]; split s of the cloud = candidates [s * span, min(N, (s + 1) * span)); partial lists (the k first entries
// of each lane's list) go to pd / pi [B, S, k, N] (coalesced over the queries)
template <int KT>
__global__ __launch_bounds__(256) void dg_knn_kernel(const float *__restrict__ pts, int N, int k, int S, int span,
                                                     float *__restrict__ pd, int *__restrict__ pi) {
    __shared__ float4 tile[DG_TILE];
    const int b = blockIdx.z, s = blockIdx.y, tid = threadIdx.x;
    const int n = blockIdx.x * DG_TILE + tid;
    const float *P = pts + (long)b * N * 3;
    const int nq = n < N ? n : N - 1;
    const float qx = P[(long)nq * 3], qy = P[(long)nq * 3 + 1], qz = P[(long)nq * 3 + 2];
    float d[KT];
    int id[KT];
    dg_init<KT>(d, id);
    float kth = INFINITY;
    const int c0 = s * span, c1 = min(N, c0 + span);
    for (int t0 = c0; t0 < c1; t0 += DG_TILE) {
        const int cnt = min(DG_TILE, c1 - t0);
        __syncthreads();                                     // every lane is done with the previous tile
        if (tid < cnt) {
            const long j = t0 + tid;
            tile[tid] = make_float4(P[j * 3], P[j * 3 + 1], P[j * 3 + 2], 0.f);
        }
        __syncthreads();
        for (int u = 0; u < cnt; ++u) {
            const float4 c = tile[u];
            // pytorch3d's order: diff = p1 - p2, dist += diff * diff over d = 0, 1, 2 (separately rounded: -ffp-contract=off)
            const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
            float dd = dx * dx;
            dd = dd + dy * dy;
            dd = dd + dz * dz;
            if (dd < kth) {                                  // rare after the first tile
                dg_insert<KT>(d, id, dd, t0 + u);
                kth = dg_kth<KT>(d, k);
            }
        }
    }
    if (n < N) {
        const long base = ((long)b * S + s) * k * N + n;
        dg_unroll<KT>([&](auto R) {
            constexpr int r = decltype(R)::value;
            if (r < k) { pd[base + (long)r * N] = d[r]; pi[base + (long)r * N] = id[r]; }
        });
    }
}

// merges the S partial lists of every query in split order: splits cover ascending index ranges and each list is sorted by
// (distance, index), so inserting them in that order with the strict threshold test keeps ties ordered by index.
// dist (nullable) [B, N, k] fp32, idx [B, N, k] int32
template <int KT>
__global__ __launch_bounds__(256) void dg_knn_merge_kernel(const float *__restrict__ pd, const int *__restrict__ pi, int N, int k,
                                                           int S, float *__restrict__ dist, int *__restrict__ idx) {
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float d[KT];
    int id[KT];
    dg_init<KT>(d, id);
    float kth = INFINITY;
    for (int s = 0; s < S; ++s) {
        const long base = ((long)b * S + s) * k * N + n;
        for (int r = 0; r < k; ++r) {
            const float dn = pd[base + (long)r * N];
            if (dn < kth) {
                dg_insert<KT>(d, id, dn, pi[base + (long)r * N]);
                kth = dg_kth<KT>(d, k);
            }
        }
    }
    const long o = ((long)b * N + n) * k;
    dg_unroll<KT>([&](auto R) {
        constexpr int r = decltype(R)::value;
        if (r < k) {
            if (dist) dist[o + r] = d[r];
            idx[o + r] = id[r];
        }
    });
}

// Y[b, r, o] = sum_c X[b, r, c] W[o, c] for the N rows of cloud b = blockIdx.z (a tile never spans two clouds).
// !REDUCE: Y row stride ldy.  REDUCE: pmax / pmin [B, gridDim.y, O] = max / min of the tile's valid rows per column.
template <bool REDUCE>
__global__ __launch_bounds__(256) void dg_linear_kernel(const float *__restrict__ X, long ldx, const float *__restrict__ W, int K,
                                                        int O, int N, float *__restrict__ Y, long ldy, float *__restrict__ pmax,
                                                        float *__restrict__ pmin) {
    __shared__ float As[64][33];
    __shared__ float Ws[64][33];
    __shared__ float Rs[2][2][64];                          // REDUCE: [wave row][max, min][column of the tile]
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int b = blockIdx.z;
    const int r0 = blockIdx.y * 64;
    const int o0 = blockIdx.x * 64;
    const float *Xb = X + (long)b * N * ldx;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 32) {
        __syncthreads();                                     // the previous chunk's readers are done
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = tid + 256 * i, row = e >> 5, kk = e & 31;
            const bool kin = k0 + kk < K;
            As[row][kk] = (kin && r0 + row < N) ? Xb[(long)(r0 + row) * ldx + k0 + kk] : 0.f;
            Ws[row][kk] = (kin && o0 + row < O) ? W[(long)(o0 + row) * K + k0 + kk] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 16; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[32 * wr + col][2 * s + half], Ws[32 * wc + col][2 * s + half], acc, 0, 0, 0);
    }
    const int o = o0 + 32 * wc + col;
    if constexpr (!REDUCE) {
        if (o < O) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = r0 + 32 * wr + frag_row(r, lane);
                if (row < N) Y[((long)b * N + row) * ldy + o] = acc[r];
            }
        }
    } else {
        float mx = -INFINITY, mn = INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = r0 + 32 * wr + frag_row(r, lane);
            if (row < N) { mx = fmaxf(mx, acc[r]); mn = fminf(mn, acc[r]); }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));                 // the other 16 rows of this column
        mn = fminf(mn, __shfl_xor(mn, 32));
        if (half == 0) { Rs[wr][0][32 * wc + col] = mx; Rs[wr][1][32 * wc + col] = mn; }
        __syncthreads();
        if (tid < 64 && o0 + tid < O) {
            const long p = ((long)b * gridDim.y + blockIdx.y) * O + o0 + tid;
            pmax[p] = fmaxf(Rs[0][0][tid], Rs[1][0][tid]);
            pmin[p] = fminf(Rs[0][1][tid], Rs[1][1][tid]);
        }
    }
}

__device__ __forceinline__ float dg_bn_lrelu(float e, float q, float s, float t) {
    const float y = s * (e + q) + t;                         // two roundings (no contraction), as the per-edge form
    return y > 0.f ? y : y * 0.2f;                           // F.leaky_relu(negative_slope=0.2)
}

// PQ [B * N, 2D] (P = columns [0, D), Q = [D, 2D)), idx [B, N, k] cloud-local; out row stride ldo.
// D / 4 lanes per point, 4 consecutive channels per lane (one 16-byte load per neighbour row).
__global__ __launch_bounds__(256) void dg_edge_kernel(const float *__restrict__ PQ, int D, const int *__restrict__ idx, int N, int k,
                                                      long rows, const float *__restrict__ scale, const float *__restrict__ shift,
                                                      float *__restrict__ out, long ldo) {
    const int tpp = D >> 2, ppb = 256 / tpp;
    const long p = (long)blockIdx.x * ppb + threadIdx.x / tpp;
    if (p >= rows) return;
    const int c = (threadIdx.x % tpp) * 4;
    const long cloud = (p / N) * N;
    const long ld = 2L * D;
    const float4 s = *reinterpret_cast<const float4 *>(scale + c);
    const float4 t = *reinterpret_cast<const float4 *>(shift + c);
    float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY), mn = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
    const int *nb = idx + p * k;
    for (int r = 0; r < k; ++r) {
        const int j = min(max(nb[r], 0), N - 1);             // in range even for a cloud with NaN points (no neighbour found)
        const float4 v = *reinterpret_cast<const float4 *>(PQ + (cloud + j) * ld + c);
        mx.x = fmaxf(mx.x, v.x); mx.y = fmaxf(mx.y, v.y); mx.z = fmaxf(mx.z, v.z); mx.w = fmaxf(mx.w, v.w);
        mn.x = fminf(mn.x, v.x); mn.y = fminf(mn.y, v.y); mn.z = fminf(mn.z, v.z); mn.w = fminf(mn.w, v.w);
    }
    const float4 q = *reinterpret_cast<const float4 *>(PQ + p * ld + D + c);
    float4 y;
    y.x = dg_bn_lrelu(s.x >= 0.f ? mx.x : mn.x, q.x, s.x, t.x);
    y.y = dg_bn_lrelu(s.y >= 0.f ? mx.y : mn.y, q.y, s.y, t.y);
    y.z = dg_bn_lrelu(s.z >= 0.f ? mx.z : mn.z, q.z, s.z, t.z);
    y.w = dg_bn_lrelu(s.w >= 0.f ? mx.w : mn.w, q.w, s.w, t.w);
    *reinterpret_cast<float4 *>(out + p * ldo + c) = y;
}

// feat[b, c] = lrelu(s ext + t), ext = max (s >= 0) or min (s < 0) of conv_5's per-tile partials [B, T, L]
__global__ __launch_bounds__(256) void dg_global_kernel(const float *__restrict__ pmax, const float *__restrict__ pmin, int B, int T, int L,
                                                        const float *__restrict__ scale, const float *__restrict__ shift,
                                                        float *__restrict__ feat, long ldf) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * L) return;
    const int b = e / L, c = e - b * L;
    const float s = scale[c];
    const bool up = s >= 0.f;
    float ext = up ? -INFINITY : INFINITY;
    for (int i = 0; i < T; ++i) {
        const long p = ((long)b * T + i) * L + c;
        ext = up ? fmaxf(ext, pmax[p]) : fminf(ext, pmin[p]);
    }
    feat[(long)b * ldf + c] = dg_bn_lrelu(ext, 0.f, s, shift[c]);
}

// finalize: combined weights [W1 ; W2 - W1] of blocks 1-4 and the folded BN scale / shift of all five blocks.
// PyTorch's eval-mode batch_norm: invstd = 1 / sqrt(var + eps), alpha = invstd * w, beta = b - mean * alpha.
struct DgPrep {
    const float *w[4];
    float *wc[4];
    const float *bnw[5], *bnb[5], *bnm[5], *bnv[5];
    float *sc[5], *sh[5];
    int nbn[5], din[4], dout[4];
};

__global__ void dg_prep_kernel(DgPrep pp) {
    const int blk = blockIdx.y;
    if (blk < 4) {
        const int din = pp.din[blk], dout = pp.dout[blk];
        for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < 2 * dout * din; e += gridDim.x * blockDim.x) {
            const int o = e / din, c = e - o * din;
            const float *w = pp.w[blk];
            pp.wc[blk][e] = o < dout ? w[o * 2 * din + c] : w[(o - dout) * 2 * din + din + c] - w[(o - dout) * 2 * din + c];
        }
    }
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < pp.nbn[blk]; c += gridDim.x * blockDim.x) {
        const float invstd = __fdiv_rn(1.f, __fsqrt_rn(pp.bnv[blk][c] + 1e-5f));
        const float a = invstd * pp.bnw[blk][c];
        pp.sc[blk][c] = a;
        pp.sh[blk][c] = pp.bnb[blk][c] - pp.bnm[blk][c] * a;
    }
}

template <int KT>
static int dg_knn_launch(const float *pts, int B, int N, int k, int S, int span, float *pd, int *pi, float *dist, int *idx, hipStream_t st) {
    hipLaunchKernelGGL(dg_knn_kernel<KT>, dim3((unsigned)ceil_div(N, DG_TILE), (unsigned)S, (unsigned)B), dim3(256), 0, st,
                       pts, N, k, S, span, pd, pi);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(dg_knn_merge_kernel<KT>, dim3((unsigned)ceil_div(N, 256), (unsigned)B), dim3(256), 0, st,
                       (const float *)pd, (const int *)pi, N, k, S, dist, idx);
    LAUNCH_CHECK();
    return SURFD_OK;
}

}  // namespace surfd

using namespace surfd;

struct surfd_dgcnn {
    int L = 0, k = 0;
    ParamTable params;                // Dgcnn(L).state_dict(); tag: float offset in pblock
    int bn0[5] = {}, conv[5] = {};    // table index of bn_<l+1>.weight (bias, running_mean, running_var follow) and conv_<l+1>.weight
    long nparam = 0;
    float *pblock = nullptr;          // the state_dict tensors, fp32
    float *derived = nullptr;         // combined weights of blocks 1-4, BN scale / shift of blocks 1-5
    float *wc[4] = {}, *sc[5] = {}, *sh[5] = {};
    bool finalized = false;
    mutable DeviceArena ws;           // surfd_dgcnn_knn uses it through a const handle
};

static float *dg_ptr(const surfd_dgcnn *d, int i) { return d->pblock + d->params[i].tag; }

// splits per query block: ~1024 workgroups over the chip, at least one 256-point tile per split, at most 256 / k splits so
// that the partial lists (2 x S x k words per point) fit in the x1..x4 workspace (512 words per point) of the forward pass
static void dg_splits(int B, int N, int k, int *S, int *span) {
    const long qb = (long)B * ceil_div(N, DG_TILE);
    long s = std::max<long>(1, ceil_div<long>(1024, qb));
    s = std::min<long>({s, 256 / k, (long)ceil_div(N, DG_TILE)});
    int sp = (int)ceil_div<long>(ceil_div<long>(N, s), DG_TILE) * DG_TILE;
    *span = sp;
    *S = ceil_div(N, sp);
}

static int dg_check_cloud(const surfd_dgcnn *d, const char *fn, const float *pts, int B, int N) {
    if (!d) SURFD_FAIL(SURFD_ERR_ARG, "%s: null handle", fn);
    if (!pts) SURFD_FAIL(SURFD_ERR_ARG, "%s: null points", fn);
    if (B < 1 || N < 1) SURFD_FAIL(SURFD_ERR_ARG, "%s: B = %d, N = %d must be positive", fn, B, N);
    if (N < d->k) SURFD_FAIL(SURFD_ERR_ARG, "%s: N = %d points is fewer than k = %d neighbours", fn, N, d->k);
    if (B > 65535 || N > (1 << 22) || (long)B * N > (1L << 26))
        SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "%s: B = %d x N = %d is beyond the supported size", fn, B, N);
    return SURFD_OK;
}

static int dg_knn_any(const surfd_dgcnn *d, const float *pts, int B, int N, float *pd, int *pi, int S, int span, float *dist,
                      int *idx, hipStream_t st) {
    const int k = d->k;
    if (k <= 8) return dg_knn_launch<8>(pts, B, N, k, S, span, pd, pi, dist, idx, st);
    if (k <= 16) return dg_knn_launch<16>(pts, B, N, k, S, span, pd, pi, dist, idx, st);
    if (k == 20) return dg_knn_launch<20>(pts, B, N, k, S, span, pd, pi, dist, idx, st);
    if (k <= 24) return dg_knn_launch<24>(pts, B, N, k, S, span, pd, pi, dist, idx, st);
    return dg_knn_launch<32>(pts, B, N, k, S, span, pd, pi, dist, idx, st);
}

// device copies are made on first use, so that a handle can be created and inspected on a host without a GPU
static int dg_alloc(surfd_dgcnn *d) {
    if (d->pblock) return SURFD_OK;
    const int bnc[5] = {64, 64, 128, 256, d->L};
    long nder = 0;
    for (int l = 0; l < 4; ++l) nder += 2L * DG_DOUT[l] * DG_DIN[l];
    for (int l = 0; l < 5; ++l) nder += 2L * bnc[l];
    HIP_TRY(hipMalloc(&d->pblock, d->nparam * sizeof(float)));
    HIP_TRY(hipMalloc(&d->derived, nder * sizeof(float)));
    float *q = d->derived;
    for (int l = 0; l < 4; ++l) { d->wc[l] = q; q += 2L * DG_DOUT[l] * DG_DIN[l]; }
    for (int l = 0; l < 5; ++l) { d->sc[l] = q; q += bnc[l]; d->sh[l] = q; q += bnc[l]; }   // 64-channel multiples: 16-byte aligned
    return SURFD_OK;
}

extern "C" {

int surfd_dgcnn_create(int size_latent, int k, surfd_dgcnn **out) {
    if (!out) SURFD_FAIL(SURFD_ERR_ARG, "surfd_dgcnn_create: null out");
    if (size_latent < 1) SURFD_FAIL(SURFD_ERR_ARG, "surfd_dgcnn_create: size_latent must be positive");
    if (k < 1 || k > DG_KMAX) SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_dgcnn_create: k = %d outside 1..%d", k, DG_KMAX);
    if (size_latent > 4096) SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_dgcnn_create: size_latent %d > 4096", size_latent);
    surfd_dgcnn *d = new surfd_dgcnn();
    d->L = size_latent; d->k = k;
    // the order of Dgcnn(size_latent).state_dict(): bn_1..bn_5, then conv_1..conv_5 (dgcnn.py:42-53)
    const int bnc[5] = {64, 64, 128, 256, size_latent};
    long off = 0;
    for (int l = 0; l < 5; ++l) {
        const std::string p = "bn_" + std::to_string(l + 1) + ".";
        d->bn0[l] = d->params.size();
        for (const char *f : {"weight", "bias", "running_mean", "running_var"}) {
            d->params.add(p + f, {bnc[l]}, off);
            off += bnc[l];
        }
        d->params.add(p + "num_batches_tracked", {}, 0, true);
    }
    const int cin[5] = {6, 128, 128, 256, DG_FEAT};
    for (int l = 0; l < 5; ++l) {
        d->conv[l] = d->params.add("conv_" + std::to_string(l + 1) + ".weight", {bnc[l], cin[l]}, off);
        off += (long)bnc[l] * cin[l];
    }
    d->nparam = off;
    *out = d;
    return SURFD_OK;
}

void surfd_dgcnn_destroy(surfd_dgcnn *d) {
    if (!d) return;
    (void)hipFree(d->pblock); (void)hipFree(d->derived);
    d->ws.release();
    delete d;
}

int surfd_dgcnn_num_params(const surfd_dgcnn *d) { return d ? d->params.size() : 0; }

int surfd_dgcnn_param_info(const surfd_dgcnn *d, int i, const char **key, int64_t shape[4], int *ndim) {
    return param_info(d ? &d->params : nullptr, "surfd_dgcnn_param_info", i, key, shape, ndim);
}

int surfd_dgcnn_set_param(surfd_dgcnn *d, const char *key, const void *dev_ptr, const int64_t *shape, int ndim, surfd_stream s) {
    if (!d) SURFD_FAIL(SURFD_ERR_ARG, "surfd_dgcnn_set_param: null handle");
    int i, rc;
    if ((rc = d->params.match("surfd_dgcnn_set_param", key, shape, ndim, &i))) return rc;
    if (d->params[i].ignored) { d->params.mark(i); return SURFD_OK; }
    if (!dev_ptr) SURFD_FAIL(SURFD_ERR_ARG, "surfd_dgcnn_set_param: '%s' has a null pointer", key);
    if ((rc = dg_alloc(d))) return rc;
    HIP_TRY(hipMemcpyAsync(dg_ptr(d, i), dev_ptr, d->params.numel(i) * sizeof(float), hipMemcpyDeviceToDevice, as_stream(s)));
    d->params.mark(i);
    d->finalized = false;
    return SURFD_OK;
}

int surfd_dgcnn_finalize(surfd_dgcnn *d, surfd_stream s) {
    if (!d) SURFD_FAIL(SURFD_ERR_ARG, "surfd_dgcnn_finalize: null handle");
    int rc;
    if ((rc = d->params.require_all("surfd_dgcnn_finalize"))) return rc;
    DgPrep pp;
    for (int l = 0; l < 5; ++l) {
        if (l < 4) { pp.w[l] = dg_ptr(d, d->conv[l]); pp.wc[l] = d->wc[l]; pp.din[l] = DG_DIN[l]; pp.dout[l] = DG_DOUT[l]; }
        pp.bnw[l] = dg_ptr(d, d->bn0[l]);
        pp.bnb[l] = dg_ptr(d, d->bn0[l] + 1);
        pp.bnm[l] = dg_ptr(d, d->bn0[l] + 2);
        pp.bnv[l] = dg_ptr(d, d->bn0[l] + 3);
        pp.sc[l] = d->sc[l]; pp.sh[l] = d->sh[l];
        pp.nbn[l] = l < 4 ? DG_DOUT[l] : d->L;
    }
    hipLaunchKernelGGL(dg_prep_kernel, dim3(64, 5), dim3(256), 0, as_stream(s), pp);
    LAUNCH_CHECK();
    d->finalized = true;
    return SURFD_OK;
}

int surfd_dgcnn_knn(const surfd_dgcnn *d, const float *pts, int B, int N, float *dists, int32_t *idx, surfd_stream s) {
    int rc;
    if ((rc = dg_check_cloud(d, "surfd_dgcnn_knn", pts, B, N))) return rc;
    if (!idx) SURFD_FAIL(SURFD_ERR_ARG, "surfd_dgcnn_knn: null idx");
    hipStream_t st = as_stream(s);
    int S, span;
    dg_splits(B, N, d->k, &S, &span);
    const size_t np = (size_t)B * S * d->k * N;
    if ((rc = d->ws.reserve(2 * np * sizeof(float), st))) return rc;
    float *pd = (float *)d->ws.ptr;
    return dg_knn_any(d, pts, B, N, pd, (int *)(pd + np), S, span, dists, idx, st);
}

int surfd_dgcnn_forward(surfd_dgcnn *d, const float *pts, int B, int N, float *feat, surfd_stream s) {
    return surfd_dgcnn_forward_features(d, pts, B, N, feat, nullptr, s);
}

int surfd_dgcnn_forward_features(surfd_dgcnn *d, const float *pts, int B, int N, float *feat, float *x1234, surfd_stream s) {
    int rc;
    if ((rc = dg_check_cloud(d, "surfd_dgcnn_forward", pts, B, N))) return rc;
    if (!feat) SURFD_FAIL(SURFD_ERR_ARG, "surfd_dgcnn_forward: null feat");
    if (!d->finalized) SURFD_FAIL(SURFD_ERR_STATE, "surfd_dgcnn_forward: parameters not finalized (surfd_dgcnn_finalize)");
    hipStream_t st = as_stream(s);
    const int k = d->k, L = d->L;
    const long rows = (long)B * N;
    const int T = ceil_div(N, 64);
    // arena: x1..x4 [B N, 512] | P,Q [B N, <= 512] | idx [B N, k] int32 | conv_5 partials 2 x [B, T, L]
    const size_t nx = (size_t)rows * DG_FEAT, ni = (size_t)rows * k, nr = (size_t)B * T * L;
    if ((rc = d->ws.reserve((2 * nx + ni + 2 * nr) * sizeof(float), st))) return rc;
    float *X = (float *)d->ws.ptr, *PQ = X + nx;
    int *idx = (int *)(PQ + nx);
    float *pmax = (float *)(idx + ni), *pmin = pmax + nr;
    int S, span;
    dg_splits(B, N, k, &S, &span);
    // the partial lists live in the x1..x4 region until the merge has read them (2 S k <= 512 words per point)
    if ((rc = dg_knn_any(d, pts, B, N, X, (int *)X + (size_t)B * S * k * N, S, span, nullptr, idx, st))) return rc;
    for (int l = 0; l < 4; ++l) {
        const float *in = l == 0 ? pts : X + DG_XOFF[l - 1];
        const long ldx = l == 0 ? 3 : DG_FEAT;
        const int D = DG_DOUT[l];
        hipLaunchKernelGGL(dg_linear_kernel<false>, dim3((unsigned)ceil_div(2 * D, 64), (unsigned)T, (unsigned)B), dim3(256), 0, st,
                           in, ldx, (const float *)d->wc[l], DG_DIN[l], 2 * D, N, PQ, 2L * D, (float *)nullptr, (float *)nullptr);
        LAUNCH_CHECK();
        const int ppb = 256 / (D / 4);
        hipLaunchKernelGGL(dg_edge_kernel, dim3((unsigned)ceil_div<long>(rows, ppb)), dim3(256), 0, st,
                           (const float *)PQ, D, (const int *)idx, N, k, rows, (const float *)d->sc[l], (const float *)d->sh[l],
                           X + DG_XOFF[l], (long)DG_FEAT);
        LAUNCH_CHECK();
    }
    if (x1234) HIP_TRY(hipMemcpyAsync(x1234, X, nx * sizeof(float), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(dg_linear_kernel<true>, dim3((unsigned)ceil_div(L, 64), (unsigned)T, (unsigned)B), dim3(256), 0, st,
                       (const float *)X, (long)DG_FEAT, (const float *)dg_ptr(d, d->conv[4]), DG_FEAT, L, N, (float *)nullptr, 0L,
                       pmax, pmin);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(dg_global_kernel, dim3((unsigned)ceil_div(B * L, 256)), dim3(256), 0, st,
                       (const float *)pmax, (const float *)pmin, B, T, L, (const float *)d->sc[4], (const float *)d->sh[4], feat, (long)L);
    LAUNCH_CHECK();
    return SURFD_OK;
}

}  // extern "C"
