// Normals of point clouds: per point the K nearest points of its own cloud, the covariance of that neighbourhood, and its
// eigen-decomposition; the eigenvector of the smallest eigenvalue is the normal, the three eigenvalues give the surface
// variation (Pauly et al. 2002).  No reference counterpart (the reference ships no evaluation code): stands for open3d's
// estimate_normals / pytorch3d's estimate_pointcloud_normals and feeds the normal consistency of cloudmetrics.py.  fp32 pair
// arithmetic on the VALU, fp64 moments and eigen-solver, no MFMA, no atomics.
//
// The contract, for point i of cloud b with n = lengths[b] (else N) valid points; every operation named is ONE IEEE rounding
// (the library is built with -ffp-contract=off; nothing here is an fma):
//   1  pair arithmetic, cn_pair's of cloudnn.hip: d = x_j - x_i per coordinate in fp32, d2 = (dx dx + dy dy) + dz dz.
//   2  neighbourhood: the K smallest candidates j < n under the total order (d2, j), i.e. of the 64-bit key
//      bits(d2) << 32 | j (d2 >= +0, so its bit pattern orders like its value; cloudfps.hip uses the same key).  The point itself
//      is a candidate like any other: normally rank 0, and among duplicates the lower index wins.  knn_idx, when asked for, lists
//      the neighbours in ascending key order.
//   3  moments in fp64, in rank order r = 0 .. K-1, of the widened fp32 differences d_r (exact): s1_a += d_a (3 entries),
//      s2_ab += d_a d_b (6 entries: one product rounding, one add rounding); m = s1 / K; C_ab = s2_ab / K - m_a m_b.
//      Differences to the query point, not raw coordinates, keep the cancellation harmless.
//   4  cyclic Jacobi in fp64, 6 sweeps over the pairs (0,1), (0,2), (1,2), V = identity at the start, only + - * / sqrt and
//      compares.  If a_pq == 0 the rotation is skipped.  Otherwise, r the third index:
//          theta = (a_qq - a_pp) / (2 a_pq);  t = sign(theta) / (|theta| + sqrt(theta theta + 1)), sign(0) = +1 (an
//          overflowing theta theta gives t = 0, which is right);  c = 1 / sqrt(t t + 1);  s = t c;
//          a_pp -= t a_pq;  a_qq += t a_pq;  a_pq = 0;  a_rp' = c a_rp - s a_rq;  a_rq' = s a_rp + c a_rq;
//          v_kp' = c v_kp - s v_kq;  v_kq' = s v_kp + c v_kq for the rows k of V.
//   5  the three (lambda, column) pairs sorted ascending, stably (equal lambda keep column order); eigenvalues = the lambda
//      rounded once to fp32.  No clamp: lambda_0 may be a tiny negative number.
//   6  normal = the column of lambda_0, every component rounded once to fp32, not renormalised; then the whole vector is negated
//      if its component of largest magnitude (the lowest axis on a tie) is negative.
//   7  rows at or beyond lengths[b] are zeros (normals, eigenvalues) and -1 (knn_idx); their input is never read.
// The result of a point is a function of the point and its cloud as an indexed array: batch size, grid, tiling and the position
// in the batch do not enter.
//
// Work decomposition: cnrm_kernel<T> - one workgroup = one cloud and T consecutive queries of it, one query per lane.  The
// cloud streams through LDS in tiles of CNRM_TILE points (float4 each); every lane reads candidate u at the same address (a
// broadcast).  Selection: every lane keeps its K best keys SORTED in LDS, list[r * T + lane] (rank-major: the lanes of a wave
// touch consecutive 8-byte words, no bank conflict; a runtime-indexed register array would go to scratch).  The high word of
// the K-th key stays in a register.  Candidates arrive in ascending j, so a candidate enters exactly when bits(d2) is below that
// word (an equal d2 carries a higher index than everything in the list and loses).  A trip of the scan reads CNRM_UNROLL
// candidates, forms their d2 and compares the smallest with that word: the common trip is the pair arithmetic, one v_min_u32,
// one v_min3_u32 and one compare for four candidates (36 VALU instructions, 9.0 per pair, in the gfx950 code object); only when
// one of them enters are the four walked in order.  An entering key is placed by insertion from the tail; after the warm-up (the first K candidates, where
// the walk starts at rank j instead of K - 1) that happens about K ln(n / K) times per query.  T = 256 for K <= 32, T = 128 above:
// the lists take 8 K T <= 64 KB either way, the tile 16 KB, so two workgroups share a CU at the largest K.
// After the scan a lane walks its list in rank order, reloads x_j (the cloud is L2-resident) and forms the moments; the Jacobi
// sweeps run on 6 + 9 fp64 registers with static indices.
//
// Bounds: n is clamped into 0 .. N in the kernel.  A block whose queries all lie at or beyond n, or whose cloud has n < K (the
// caller's to refuse), writes padding and leaves before the first barrier.  Staging reads points below n only; a list is full of
// real keys once K <= n candidates went by, and an index decoded from it is clamped below n all the same.  LDS: the lists are
// indexed with r < K and lane < T, the tile with u < cnt <= CNRM_TILE.
#include "common.h"
#include <cmath>
#include <algorithm>

namespace surfd {

constexpr int CNRM_TILE = 1024;             // candidate points per LDS tile
constexpr int CNRM_UNROLL = 4;              // candidates per trip of the scan
constexpr int CNRM_KMIN = 3, CNRM_KMAX = 64;
constexpr int CNRM_KWIDE = 32;              // up to here 256 lanes per workgroup, above 128
constexpr int CNRM_MAX_POINTS = 1 << 20;

__host__ __device__ constexpr int cnrm_lds_bytes(int K, int T) { return CNRM_TILE * 16 + K * T * 8; }

// places key in the sorted list mine[0], mine[stride], .. of K ranks; j = how many candidates came before it (the ranks above j
// are still empty during the warm-up, so the walk starts there).  The last rank falls out.
__host__ __device__ __forceinline__ void cnrm_insert(unsigned long long *mine, int stride, int K, unsigned long long key, int j) {
    int r = j < K - 1 ? j : K - 1;
    while (r > 0) {
        const unsigned long long prev = mine[(r - 1) * stride];
        if (prev < key) break;
        mine[r * stride] = prev;
        --r;
    }
    mine[r * stride] = key;
}

// one Jacobi rotation of the pair (p, q); r is the third index.  vXp / vXq: the columns p and q of V
__host__ __device__ __forceinline__ void cnrm_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                                     double &v0q, double &v1p, double &v1q, double &v2p, double &v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double root = __builtin_sqrt(theta * theta + 1.0);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(theta) + root);
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
    const double s = t * c;
    const double tapq = t * apq;
    app = app - tapq;
    aqq = aqq + tapq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    const double n0p = c * v0p - s * v0q, n0q = s * v0p + c * v0q;
    const double n1p = c * v1p - s * v1q, n1q = s * v1p + c * v1q;
    const double n2p = c * v2p - s * v2q, n2q = s * v2p + c * v2q;
    v0p = n0p; v0q = n0q; v1p = n1p; v1q = n1q; v2p = n2p; v2q = n2q;
}

// steps 4-6: the symmetric matrix (6 unique entries) -> the canonical normal and the ascending eigenvalues, rounded to fp32
__host__ __device__ __forceinline__ void cnrm_eigen(double a00, double a11, double a22, double a01, double a02, double a12, float &nx,
                                                    float &ny, float &nz, float &e0, float &e1, float &e2) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // v[row][column]
#pragma unroll 1
    for (int sweep = 0; sweep < 6; ++sweep) {
        cnrm_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (p, q) = (0, 1), r = 2
        cnrm_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
        cnrm_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
    }
    // stable ascending sort of (lambda, column): adjacent exchanges on a strict compare
    double l0 = a00, l1 = a11, l2 = a22;
    double c0x = v00, c0y = v10, c0z = v20, c1x = v01, c1y = v11, c1z = v21, c2x = v02, c2y = v12, c2z = v22;
    auto exchange = [](double &la, double &lb, double &ax, double &ay, double &az, double &bx, double &by, double &bz) {
        if (lb < la) {
            double t;
            t = la; la = lb; lb = t;
            t = ax; ax = bx; bx = t;
            t = ay; ay = by; by = t;
            t = az; az = bz; bz = t;
        }
    };
    exchange(l0, l1, c0x, c0y, c0z, c1x, c1y, c1z);
    exchange(l1, l2, c1x, c1y, c1z, c2x, c2y, c2z);
    exchange(l0, l1, c0x, c0y, c0z, c1x, c1y, c1z);
    nx = (float)c0x; ny = (float)c0y; nz = (float)c0z;
    float big = nx, mag = fabsf(nx);
    if (fabsf(ny) > mag) { big = ny; mag = fabsf(ny); }
    if (fabsf(nz) > mag) { big = nz; }
    if (big < 0.f) { nx = -nx; ny = -ny; nz = -nz; }
    e0 = (float)l0; e1 = (float)l1; e2 = (float)l2;
}

// x[B, N, 3] -> normals[B, N, 3], eig[B, N, 3], knn[B, N, K] (nullable); grid = B * ceil(N / T), block = T,
// dynamic LDS = cnrm_lds_bytes(K, T)
template <int T>
__global__ __launch_bounds__(T) void cnrm_kernel(const float *__restrict__ x, int N, const int *__restrict__ lengths, int K, int nblk,
                                                 float *__restrict__ normals, float *__restrict__ eig, int *__restrict__ knn) {
    extern __shared__ __align__(16) unsigned char cnrm_lds[];
    float4 *tile = reinterpret_cast<float4 *>(cnrm_lds);                                                  // [CNRM_TILE]
    unsigned long long *list = reinterpret_cast<unsigned long long *>(cnrm_lds + CNRM_TILE * 16);         // [K][T]
    const int tid = threadIdx.x;
    const int b = blockIdx.x / nblk, q0 = (blockIdx.x % nblk) * T;
    const int i = q0 + tid;
    const float *X = x + (long)b * N * 3;
    const int n = min(max(lengths ? lengths[b] : N, 0), N);
    const long row = (long)b * N + i;
    if (q0 >= n || n < K) {                                   // nothing but padding in this block (uniform: before any barrier)
        if (i < N) {
            normals[row * 3] = 0.f; normals[row * 3 + 1] = 0.f; normals[row * 3 + 2] = 0.f;
            eig[row * 3] = 0.f; eig[row * 3 + 1] = 0.f; eig[row * 3 + 2] = 0.f;
            if (knn)
                for (int r = 0; r < K; ++r) knn[row * K + r] = -1;
        }
        return;
    }
    const bool active = i < n;
    const long iq = active ? i : n - 1;                       // a lane without a query repeats the last one and writes padding
    const float qx = X[iq * 3], qy = X[iq * 3 + 1], qz = X[iq * 3 + 2];
    unsigned long long *mine = list + tid;                    // mine[r * T] is rank r
    for (int r = 0; r < K; ++r) mine[r * T] = ~0ull;
    unsigned kth_hi = 0xFFFFFFFFu;                            // high word of the K-th key: above the bits of every d2
    for (int t0 = 0; t0 < n; t0 += CNRM_TILE) {
        const int cnt = min(CNRM_TILE, n - t0);
        __syncthreads();                                      // every lane is done with the previous tile
        for (int e = tid; e < cnt; e += T) {
            const long j = t0 + e;
            tile[e] = make_float4(X[j * 3], X[j * 3 + 1], X[j * 3 + 2], 0.f);
        }
        __syncthreads();
        if (active) {
            auto pair_bits = [&](float4 c) {                  // cn_pair's order; the bit pattern of d2 >= +0 orders like its value
                const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
                float dd = dx * dx;
                dd = dd + dy * dy;
                dd = dd + dz * dz;
                return __float_as_uint(dd);
            };
            auto consider = [&](unsigned hi, int j) {         // ascending j: an equal d2 loses to what is in the list
                if (hi < kth_hi) {
                    cnrm_insert(mine, T, K, ((unsigned long long)hi << 32) | (unsigned)j, j);
                    kth_hi = (unsigned)(mine[(K - 1) * T] >> 32);
                }
            };
            int u = 0;
            for (; u + CNRM_UNROLL <= cnt; u += CNRM_UNROLL) {
                unsigned h[CNRM_UNROLL];
#pragma unroll
                for (int v = 0; v < CNRM_UNROLL; ++v) h[v] = pair_bits(tile[u + v]);   // the same address in every lane: a broadcast
                unsigned lowest = h[0];
#pragma unroll
                for (int v = 1; v < CNRM_UNROLL; ++v) lowest = min(lowest, h[v]);
                if (lowest < kth_hi) {                        // rare after the warm-up: the candidates of the trip in order
#pragma unroll
                    for (int v = 0; v < CNRM_UNROLL; ++v) consider(h[v], t0 + u + v);
                }
            }
            for (; u < cnt; ++u) consider(pair_bits(tile[u]), t0 + u);
        }
    }
    if (i >= N) return;
    float *Nn = normals + row * 3, *Ev = eig + row * 3;
    int *Kn = knn ? knn + row * K : nullptr;
    if (!active) {
        Nn[0] = 0.f; Nn[1] = 0.f; Nn[2] = 0.f;
        Ev[0] = 0.f; Ev[1] = 0.f; Ev[2] = 0.f;
        if (Kn)
            for (int r = 0; r < K; ++r) Kn[r] = -1;
        return;
    }
    // moments in rank order
    double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, syy = 0.0, szz = 0.0, sxy = 0.0, sxz = 0.0, syz = 0.0;
    for (int r = 0; r < K; ++r) {
        const int j = (int)min((unsigned)mine[r * T], (unsigned)(n - 1));
        if (Kn) Kn[r] = j;
        const float fx = X[(long)j * 3] - qx, fy = X[(long)j * 3 + 1] - qy, fz = X[(long)j * 3 + 2] - qz;
        const double dx = (double)fx, dy = (double)fy, dz = (double)fz;
        s1x = s1x + dx; s1y = s1y + dy; s1z = s1z + dz;
        sxx = sxx + dx * dx; syy = syy + dy * dy; szz = szz + dz * dz;
        sxy = sxy + dx * dy; sxz = sxz + dx * dz; syz = syz + dy * dz;
    }
    const double kd = (double)K;
    const double mx = s1x / kd, my = s1y / kd, mz = s1z / kd;
    const double a00 = sxx / kd - mx * mx, a11 = syy / kd - my * my, a22 = szz / kd - mz * mz;
    const double a01 = sxy / kd - mx * my, a02 = sxz / kd - mx * mz, a12 = syz / kd - my * mz;
    float nx, ny, nz, e0, e1, e2;
    cnrm_eigen(a00, a11, a22, a01, a02, a12, nx, ny, nz, e0, e1, e2);
    Nn[0] = nx; Nn[1] = ny; Nn[2] = nz;
    Ev[0] = e0; Ev[1] = e1; Ev[2] = e2;
}

template <int T>
static int cnrm_launch(const float *x, int B, int N, const int *lengths, int K, float *normals, float *eig, int *knn, hipStream_t st) {
    const int nblk = ceil_div(N, T);
    const int lds = cnrm_lds_bytes(K, T);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&cnrm_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(cnrm_kernel<T>, dim3((unsigned)((long)B * nblk)), dim3(T), lds, st, x, N, lengths, K, nblk, normals, eig, knn);
    LAUNCH_CHECK();
    return SURFD_OK;
}

}  // namespace surfd

using namespace surfd;

extern "C" {

int surfd_cloud_normals(const float *x, int B, int N, const int32_t *lengths, int K, float *normals, float *eigenvalues, int32_t *knn_idx,
                        surfd_stream s) {
    if (B < 0) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_normals: B = %d is negative", B);
    if (N < 1) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_normals: N = %d must be positive", N);
    if (K < CNRM_KMIN || K > CNRM_KMAX)
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_normals: K = %d is outside %d .. %d", K, CNRM_KMIN, CNRM_KMAX);
    if (K > N) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_normals: K = %d exceeds N = %d", K, N);
    if (B == 0) return SURFD_OK;
    if (!x) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_normals: null x");
    if (!normals || !eigenvalues) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_normals: null normals or eigenvalues");
    const int T = K <= CNRM_KWIDE ? 256 : 128;
    if (N > CNRM_MAX_POINTS || (long)B * ceil_div(N, T) > 0x7FFFFFFFl)
        SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_cloud_normals: B = %d, N = %d is beyond the supported size (%d points per cloud, 2^31 workgroups)",
                   B, N, CNRM_MAX_POINTS);
    hipStream_t st = as_stream(s);
    if (T == 256) return cnrm_launch<256>(x, B, N, lengths, K, normals, eigenvalues, knn_idx, st);
    return cnrm_launch<128>(x, B, N, lengths, K, normals, eigenvalues, knn_idx, st);
}

}  // extern "C"
