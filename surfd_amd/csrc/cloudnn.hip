// Nearest neighbours between point clouds and the matrix of directed Chamfer means between two SETS of clouds: what the
// set metrics of a shape generator (MMD, COV, 1-NNA over Chamfer distances; Achlioptas et al. 2018, as used in PointFlow) and
// the Chamfer distance / F-score of a pair are made of.  No reference counterpart (the reference ships no evaluation code);
// the per-pair arithmetic is pytorch3d's knn_points(p1, p2, K=1), as in dg_knn_kernel.  Plain fp32, VALU only.
//
//   cn_matrix_kernel<P> — one workgroup = ONE query cloud a_i and a range of candidate clouds b_j.  The query cloud lives in
//                         registers, P points per lane (P = 8: 2 048 points in 256 lanes; larger clouds are walked in tiles of
//                         256 P points, reloaded per candidate cloud).  A candidate cloud streams through LDS in tiles of
//                         CN_TILE points (float4 per point, 32 KB); every lane reads candidate u with the same address (one
//                         ds_read_b96, a broadcast) and tests it against all P of its points, so the LDS read and the loop
//                         overhead are paid once per P pairs.  Per (i, j) the lane's minima are summed in fp64 and reduced over
//                         the workgroup in a fixed tree; thread 0 writes mean[i, j] (and below[i, j]).
//   cn_nn_kernel        — per-item nearest neighbour with the index carried: one query per lane, the candidate cloud through
//                         the same LDS tile.  Used per pair of clouds, not in bulk.
//
// Pair arithmetic — cn_pair(), the one place a squared distance is formed: diff = p - q per coordinate, d2 = (dx dx + dy dy)
// + dz dz, one rounding per operation (the library is built with -ffp-contract=off; nothing here is an fma).
// Selection: the nearest neighbour is the minimum under the total order (d2, index).  cn_matrix_kernel needs the value only
// (v_min_f32 selects, it does not round), cn_nn_kernel walks the candidates in ascending index order with a strict compare, so a
// tie keeps the lower index.  Hence the d2 of a point is bit for bit a function of (p, candidate cloud as a set): it does not
// depend on the tiling, the grid, the batch or the order of the candidate points.  A tile's tail is padded to a multiple of
// CN_UNROLL with copies of its last point, which changes neither the minimum nor (being later in the order) the index.
//
// Sum order of mean[i, j] (depends on Na only): lane t holds the points tile * 256 P + p * 256 + t; it adds their minima to an
// fp64 accumulator in (tile, p) order; the 64 accumulators of a wave are added by __shfl_xor with offsets 32, 16, .. 1 (every
// lane ends with the same value: fp64 addition is commutative, and both partners add the same two numbers); the four wave sums
// go through LDS and are added as ((w0 + w1) + w2) + w3.  mean = float(sum / double(Na)): one rounding to fp32.  The sum of
// 2^24 fp32 numbers of one sign in fp64 carries a relative error below 2^-28: invisible in fp32.
//
// Inner loop (llvm-objdump -d of the gfx950 code object, cn_matrix_kernel<8>, the block that ends in the backward branch):
// 4 candidates x 8 points = 32 pairs per trip in 273 VALU instructions = 8.53 per pair (96 v_sub, 96 v_mul, 64 v_add, 16 v_min3
// - two minima each, which is how the count falls below the 9 of the pair written out - and 1 v_mov), 4 ds_read_b96 and 3
// scalar instructions beside them.  tools/cloudmetrics_time.py counts them from the shipped library.  This file is compiled with
// -fno-slp-vectorize (surfd_amd/build.py): with the SLP vectoriser half of the v_sub / v_mul become v_pk_*_f32, which issue at
// half rate and bring 36 s_nop per trip; measured 17-20 % slower.
//
// Hazards: the candidate tile and the four-entry reduction arrays are the only LDS; the tile is bracketed by __syncthreads() on
// both sides, the reduction arrays are written after the last read of the previous candidate cloud's sums is two barriers old
// (the staging barriers of the next tile).  Cross-lane values move with __shfl_xor only.  No atomics.
#include "common.h"
#include <cfloat>
#include <cmath>
#include <algorithm>

namespace surfd {

constexpr int CN_TILE = 2048;       // candidate points per LDS tile
constexpr int CN_UNROLL = 4;        // candidates per trip of the inner loop
constexpr int CN_PMAX = 8;          // query points per lane
constexpr int CN_TARGET_WGS = 2048; // workgroups a small call is spread over (8 per CU)

// pytorch3d's order: diff = p1 - p2, dist += diff * diff over d = 0, 1, 2 (separately rounded)
__device__ __forceinline__ float cn_pair(float px, float py, float pz, float4 c) {
    const float dx = px - c.x, dy = py - c.y, dz = pz - c.z;
    float dd = dx * dx;
    dd = dd + dy * dy;
    dd = dd + dz * dz;
    return dd;
}

// stages the points [t0, t0 + cnt) of cloud C into the tile and pads to a multiple of CN_UNROLL with copies of the last one
__device__ __forceinline__ void cn_stage(float4 *tile, const float *__restrict__ C, int t0, int cnt, int tid) {
    const int padded = (cnt + CN_UNROLL - 1) / CN_UNROLL * CN_UNROLL;
    for (int e = tid; e < padded; e += 256) {
        const long j = t0 + min(e, cnt - 1);
        tile[e] = make_float4(C[j * 3], C[j * 3 + 1], C[j * 3 + 2], 0.f);
    }
}

// a[M, Na, 3], b[R, Nb, 3]; workgroup blockIdx.x = i * S + s takes the candidate clouds [s * span, min(R, (s + 1) * span))
template <int P>
__global__ __launch_bounds__(256) void cn_matrix_kernel(const float *__restrict__ a, int Na, const float *__restrict__ b, int R, int Nb,
                                                        int S, int span, float tau2, float *__restrict__ mean, int *__restrict__ below) {
    __shared__ float4 tile[CN_TILE];
    __shared__ double red_sum[4];
    __shared__ int red_cnt[4];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int i = blockIdx.x / S, s = blockIdx.x % S;
    const float *A = a + (long)i * Na * 3;
    constexpr int QT = 256 * P;                               // query points per register tile
    const int nqt = (Na + QT - 1) / QT;
    float qx[P], qy[P], qz[P];
    auto load_queries = [&](int q0) {
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const long n = min(q0 + p * 256 + tid, Na - 1);   // a lane without a point repeats the last one; it is not summed
            qx[p] = A[n * 3]; qy[p] = A[n * 3 + 1]; qz[p] = A[n * 3 + 2];
        }
    };
    if (nqt == 1) load_queries(0);
    const int j1 = min(R, (s + 1) * span);
    for (int j = s * span; j < j1; ++j) {
        const float *Bj = b + (long)j * Nb * 3;
        double acc = 0.0;
        int cnt_below = 0;
        for (int qt = 0; qt < nqt; ++qt) {
            if (nqt > 1) load_queries(qt * QT);
            float m[P];
#pragma unroll
            for (int p = 0; p < P; ++p) m[p] = INFINITY;
            for (int t0 = 0; t0 < Nb; t0 += CN_TILE) {
                const int cnt = min(CN_TILE, Nb - t0);
                __syncthreads();                              // every lane is done with the previous tile
                cn_stage(tile, Bj, t0, cnt, tid);
                __syncthreads();
                for (int u = 0; u < cnt; u += CN_UNROLL) {
#pragma unroll
                    for (int v = 0; v < CN_UNROLL; ++v) {
                        const float4 c = tile[u + v];         // the same address in every lane: a broadcast
#pragma unroll
                        for (int p = 0; p < P; ++p) m[p] = fminf(m[p], cn_pair(qx[p], qy[p], qz[p], c));
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const bool valid = qt * QT + p * 256 + tid < Na;
                acc += valid ? (double)m[p] : 0.0;
                cnt_below += (valid && m[p] < tau2) ? 1 : 0;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            acc += __shfl_xor(acc, o);
            cnt_below += __shfl_xor(cnt_below, o);
        }
        if ((tid & 63) == 0) { red_sum[wave] = acc; red_cnt[wave] = cnt_below; }
        __syncthreads();
        if (tid == 0) {
            const double sum = ((red_sum[0] + red_sum[1]) + red_sum[2]) + red_sum[3];
            mean[(long)i * R + j] = (float)(sum / (double)Na);
            if (below) below[(long)i * R + j] = ((red_cnt[0] + red_cnt[1]) + red_cnt[2]) + red_cnt[3];
        }
    }
}

// a[B, Na, 3], b[B, Nb, 3] -> d2[B, Na], idx[B, Na]; one query per lane, grid (ceil(Na / 256), B)
__global__ __launch_bounds__(256) void cn_nn_kernel(const float *__restrict__ a, const float *__restrict__ b, int Na, int Nb,
                                                    float *__restrict__ d2, int *__restrict__ idx) {
    __shared__ float4 tile[CN_TILE];
    const int tid = threadIdx.x, bi = blockIdx.y;
    const int n = blockIdx.x * 256 + tid;
    const float *A = a + (long)bi * Na * 3, *Bc = b + (long)bi * Nb * 3;
    const long nq = n < Na ? n : Na - 1;
    const float qx = A[nq * 3], qy = A[nq * 3 + 1], qz = A[nq * 3 + 2];
    float best = INFINITY;
    int bj = 0;
    for (int t0 = 0; t0 < Nb; t0 += CN_TILE) {
        const int cnt = min(CN_TILE, Nb - t0);
        __syncthreads();                                      // every lane is done with the previous tile
        cn_stage(tile, Bc, t0, cnt, tid);
        __syncthreads();
        for (int u = 0; u < cnt; u += CN_UNROLL) {
#pragma unroll
            for (int v = 0; v < CN_UNROLL; ++v) {
                const float dd = cn_pair(qx, qy, qz, tile[u + v]);
                const bool better = dd < best;                // strict, ascending index: a tie keeps the lower index
                best = better ? dd : best;
                bj = better ? t0 + u + v : bj;                // a padding copy (index >= t0 + cnt) ties its original and never wins
            }
        }
    }
    if (n < Na) {
        if (d2) d2[(long)bi * Na + n] = best;
        if (idx) idx[(long)bi * Na + n] = bj;
    }
}

template <int P>
static void cn_matrix_launch(const float *a, int M, int Na, const float *b, int R, int Nb, int S, int span, float tau2, float *mean,
                             int *below, hipStream_t st) {
    hipLaunchKernelGGL(cn_matrix_kernel<P>, dim3((unsigned)((long)M * S)), dim3(256), 0, st, a, Na, b, R, Nb, S, span, tau2, mean, below);
}

}  // namespace surfd

using namespace surfd;

extern "C" {

int surfd_cloud_nn(const float *a, const float *b, int B, int Na, int Nb, float *d2, int32_t *idx, surfd_stream s) {
    if (B < 0) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_nn: B = %d is negative", B);
    if (Na < 1 || Nb < 1) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_nn: Na = %d, Nb = %d must be positive", Na, Nb);
    if (B == 0) return SURFD_OK;
    if (!a || !b) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_nn: null a or b");
    if (B > 65535 || Na > (1 << 28) || Nb > (1 << 28))
        SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_cloud_nn: B = %d, Na = %d, Nb = %d is beyond the supported size", B, Na, Nb);
    if (!d2 && !idx) return SURFD_OK;
    hipLaunchKernelGGL(cn_nn_kernel, dim3((unsigned)ceil_div(Na, 256), (unsigned)B), dim3(256), 0, as_stream(s), a, b, Na, Nb, d2, idx);
    LAUNCH_CHECK();
    return SURFD_OK;
}

// the argument checks of surfd_cloud_nn_matrix and its launch plan, on the host alone: P query points per lane, S ranges of
// `span` candidate clouds per query cloud (about CN_TARGET_WGS workgroups over the chip, whole clouds per range), nqt register
// tiles of 256 P query points
struct CnPlan { int P, S, span, nqt; };
static int cn_matrix_plan(int M, int Na, int R, int Nb, CnPlan *plan) {
    if (M < 1 || R < 1 || Na < 1 || Nb < 1)
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_nn_matrix: M = %d, Na = %d, R = %d, Nb = %d must be positive", M, Na, R, Nb);
    if (M > (1 << 20) || R > (1 << 20) || Na > (1 << 24) || Nb > (1 << 28))
        SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_cloud_nn_matrix: M = %d, Na = %d, R = %d, Nb = %d is beyond the supported size", M, Na, R, Nb);
    const int want = std::min<long>(R, std::max<long>(1, ceil_div<long>(CN_TARGET_WGS, M)));
    plan->span = ceil_div(R, want);
    plan->S = ceil_div(R, plan->span);
    plan->P = Na <= 256 ? 1 : Na <= 512 ? 2 : Na <= 1024 ? 4 : CN_PMAX;
    plan->nqt = ceil_div(Na, 256 * plan->P);
    return SURFD_OK;
}

int surfd_cloud_nn_matrix_plan(int M, int Na, int R, int *P, int *S, int *span, int *query_tiles) {
    CnPlan plan;
    const int rc = cn_matrix_plan(M, Na, R, 1, &plan);
    if (rc != SURFD_OK) return rc;
    if (P) *P = plan.P;
    if (S) *S = plan.S;
    if (span) *span = plan.span;
    if (query_tiles) *query_tiles = plan.nqt;
    return SURFD_OK;
}

int surfd_cloud_nn_matrix(const float *a, int M, int Na, const float *b, int R, int Nb, float tau2, float *mean, int32_t *below,
                          surfd_stream s) {
    CnPlan plan;
    const int rc = cn_matrix_plan(M, Na, R, Nb, &plan);
    if (rc != SURFD_OK) return rc;
    if (!a || !b) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_nn_matrix: null a or b");
    if (!mean) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_nn_matrix: null mean");
    const int S = plan.S, span = plan.span;
    hipStream_t st = as_stream(s);
    if (plan.P == 1) cn_matrix_launch<1>(a, M, Na, b, R, Nb, S, span, tau2, mean, below, st);
    else if (plan.P == 2) cn_matrix_launch<2>(a, M, Na, b, R, Nb, S, span, tau2, mean, below, st);
    else if (plan.P == 4) cn_matrix_launch<4>(a, M, Na, b, R, Nb, S, span, tau2, mean, below, st);
    else cn_matrix_launch<CN_PMAX>(a, M, Na, b, R, Nb, S, span, tau2, mean, below, st);
    LAUNCH_CHECK();
    return SURFD_OK;
}

}  // extern "C"
