// Farthest point sampling of point clouds: K points of a cloud, each the one farthest from all picks before it, with the
// squared covering radius after every pick.  No reference counterpart (the reference samples at random, utils/utils.py:44-77,
// restated in surfd_amd/dgcnn.py); the call stands for pytorch3d's sample_farthest_points.  Plain fp32, VALU only.
//
// Definition, per cloud b with n valid points (n = lengths[b], else N):
//     mind[i] = +inf for i < n;  s = start[b] (default 0)
//     for k in 0 .. K-1:
//         if k >= n:  idx[b,k] = -1; cover2[b,k] = 0; continue
//         idx[b,k] = s
//         d2_i = (dx dx + dy dy) + dz dz, d = p_i - p_s per coordinate        (cn_pair's order of cloudnn.hip, no fma)
//         mind[i] = min(mind[i], d2_i)
//         s = the i < n that maximises (mind[i], then the LOWER index on ties);  cover2[b,k] = mind[s]
// The minimum and the maximum only select, so with the tie rule fixed the whole index sequence is a function of the input
// bits: it does not depend on the tier, the workgroup size, the batch or the launch.
//
// Selection: one 64-bit key per candidate, (bits of mind << 32) | (0xFFFFFFFF - i), and the unsigned maximum.  mind is a sum of
// squares, never negative and never -0, so its bit pattern orders like its value; a tie goes to the lower index with no
// second compare.  A lane without a valid point carries key 0, which is below the key of every valid point.
//
// Work decomposition: ONE workgroup per cloud, and nothing ever waits on another workgroup (no cooperative launch, no counter
// in global memory, no inter-workgroup barrier).  Parallelism across CUs comes from the batch.  Two tiers, chosen on the host
// from N:
//   fps_resident_kernel<P, T> — N <= 8 192.  Lane t of T keeps the points p T + t (p < P) and their mind in registers for all
//                         K rounds.  Per round: P pair tests, the lane's best key, a wave maximum with __shfl_xor (6 steps on a
//                         64-bit value), the lane that holds the wave's maximum writes (key, x, y, z) to the wave's LDS slot,
//                         ONE __syncthreads(), every lane reads all T / 64 keys (the same address in every lane: broadcasts)
//                         and the winner's coordinates.  The slots are double-buffered by round parity: the slots of round k
//                         are rewritten in round k + 2, after the barrier of round k + 1, which a wave passes only once its
//                         reads of round k are done.  No global loads inside the loop, one global store of idx / cover2 by lane 0.
//                         (P, T): N <= 64 (1, 64); <= 256 (1, 256); <= 512 (2, 256); <= 1 024 (4, 256); <= 2 048 (8, 256);
//                         <= 4 096 (16, 256); <= 8 192 (8, 1 024).  Few waves with many points each beat many waves with few:
//                         measured 0.92 against 1.34 us per round at N = 2 048 for (8, 256) against (2, 1 024), and 1.30 against
//                         1.53 at N = 4 096 for (16, 256) against (4, 1 024) (which also has what was measured
//                         for the 8 192-point size).
//   fps_stream_kernel   — 8 192 < N <= 1 048 576, 1 024 lanes.  The same loop with the coordinates re-read from global memory
//                         every round (they stay in L2: 100 000 points are 1.2 MB); lane t owns the points j 1 024 + t.  The
//                         mind of the first 32 768 points lives in LDS, that of the rest in a caller-provided workspace of
//                         4 B max(0, N - 32 768) bytes (surfd_cloud_fps_workspace_bytes).  A lane reads and writes only the
//                         mind entries of its own points, so they need no barrier.  The lane that holds the wave's maximum
//                         reloads its winner's coordinates (one L1 / L2 hit) and writes the slot as above.
// Splitting one cloud over several workgroups would need a grid-wide exchange per round and is not built.
//
// LDS per workgroup: resident 48 T / 64 bytes (two buffers of T / 64 slots: 8-byte key + 16-byte float4), i.e. 48 B at
// T = 64, 192 B at T = 256, 768 B at T = 1 024; streamed 768 B + 4 min(N, 32 768) bytes (dynamic), at most 131 840 B.
//
// Bounds: n is clamped into 1 .. N and start into 0 .. n - 1 in the kernel; every index a lane forms is below n or clamped to
// n - 1; the winner's index is decoded from a key that a valid lane built.  Padding beyond lengths[b] is never read.
#include "common.h"
#include <cmath>
#include <algorithm>

namespace surfd {

constexpr int FPS_RESIDENT_MAX = 8192;      // largest N of the resident tier (P = 8, T = 1 024)
constexpr int FPS_LDS_POINTS = 32768;       // streamed tier: points whose mind lives in LDS
constexpr int FPS_MAX_POINTS = 1 << 20;
constexpr int FPS_MAX_CLOUDS = 1 << 20;
constexpr int FPS_STREAM_T = 1024;
constexpr int FPS_SLOT_BYTES = 2 * (FPS_STREAM_T / 64) * (8 + 16);

__device__ __forceinline__ unsigned long long fps_key(float m, int i) {
    return ((unsigned long long)__float_as_uint(m) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
}
__device__ __forceinline__ int fps_key_index(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)key); }

// cn_pair's order: diff per coordinate, (dx dx + dy dy) + dz dz, one rounding per operation
__device__ __forceinline__ float fps_pair(float px, float py, float pz, float sx, float sy, float sz) {
    const float dx = px - sx, dy = py - sy, dz = pz - sz;
    float dd = dx * dx;
    dd = dd + dy * dy;
    dd = dd + dz * dz;
    return dd;
}

__device__ __forceinline__ unsigned long long fps_wave_max(unsigned long long key) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    return key;
}

// after the barrier: the maximum over the NW slots of this round and the coordinates that came with it
template <int NW>
__device__ __forceinline__ unsigned long long fps_winner(const unsigned long long *skey, const float4 *sxyz, float &sx, float &sy, float &sz) {
    unsigned long long best = skey[0];
    int bw = 0;
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        const unsigned long long k = skey[w];
        const bool better = k > best;
        best = better ? k : best;
        bw = better ? w : bw;
    }
    const float4 c = sxyz[bw];
    sx = c.x; sy = c.y; sz = c.z;
    return best;
}

// pts[B, N, 3] -> idx[B, K], cover2[B, K] (nullable); grid = B, block = T; N <= P T
template <int P, int T>
__global__ __launch_bounds__(T) void fps_resident_kernel(const float *__restrict__ pts, int N, const int *__restrict__ lengths,
                                                         const int *__restrict__ start, int K, int *__restrict__ idx, float *__restrict__ cover2) {
    constexpr int NW = T / 64;
    __shared__ unsigned long long skey[2][NW];
    __shared__ float4 sxyz[2][NW];
    const int tid = threadIdx.x, wave = tid >> 6, b = blockIdx.x;
    const float *X = pts + (long)b * N * 3;
    const int n = min(max(lengths ? lengths[b] : N, 1), N);
    int s = min(max(start ? start[b] : 0, 0), n - 1);
    float px[P], py[P], pz[P], m[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const long j = min(p * T + tid, n - 1);               // a lane without a point repeats the last one; its key stays 0
        px[p] = X[j * 3]; py[p] = X[j * 3 + 1]; pz[p] = X[j * 3 + 2];
        m[p] = INFINITY;
    }
    float sx = X[(long)s * 3], sy = X[(long)s * 3 + 1], sz = X[(long)s * 3 + 2];
    int *I = idx + (long)b * K;
    float *C = cover2 ? cover2 + (long)b * K : nullptr;
    const int rounds = min(K, n);
    for (int k = 0; k < rounds; ++k) {
        unsigned long long key = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            m[p] = fminf(m[p], fps_pair(px[p], py[p], pz[p], sx, sy, sz));
            const int i = p * T + tid;
            const unsigned long long kp = i < n ? fps_key(m[p], i) : 0ull;
            key = kp > key ? kp : key;
        }
        const unsigned long long wmax = fps_wave_max(key);
        const int buf = k & 1;
        if (key == wmax && (key != 0 || (tid & 63) == 0)) {    // keys of valid points are distinct: one lane per wave
            const int pw = fps_key_index(wmax) / T;
            float bx = px[0], by = py[0], bz = pz[0];
#pragma unroll
            for (int p = 1; p < P; ++p) {
                const bool mine = pw == p;
                bx = mine ? px[p] : bx; by = mine ? py[p] : by; bz = mine ? pz[p] : bz;
            }
            skey[buf][wave] = wmax;
            sxyz[buf][wave] = make_float4(bx, by, bz, 0.f);
        }
        __syncthreads();
        const int picked = s;
        const unsigned long long best = fps_winner<NW>(skey[buf], sxyz[buf], sx, sy, sz);
        s = fps_key_index(best);
        if (tid == 0) {
            I[k] = picked;
            if (C) C[k] = __uint_as_float((unsigned)(best >> 32));
        }
    }
    for (int k = rounds + tid; k < K; k += T) {               // K > n: nothing left to pick
        I[k] = -1;
        if (C) C[k] = 0.f;
    }
}

// the same loop for N > FPS_RESIDENT_MAX; work[B, N - FPS_LDS_POINTS] (unused when N <= FPS_LDS_POINTS); grid = B, block = 1 024,
// dynamic LDS = FPS_SLOT_BYTES + 4 min(N, FPS_LDS_POINTS)
__global__ __launch_bounds__(FPS_STREAM_T) void fps_stream_kernel(const float *__restrict__ pts, int N, const int *__restrict__ lengths,
                                                                  const int *__restrict__ start, int K, int *__restrict__ idx,
                                                                  float *__restrict__ cover2, float *__restrict__ work) {
    constexpr int T = FPS_STREAM_T, NW = T / 64;
    extern __shared__ __align__(16) unsigned char fps_lds[];
    float4 *sxyz = reinterpret_cast<float4 *>(fps_lds);                                        // [2][NW]
    unsigned long long *skey = reinterpret_cast<unsigned long long *>(fps_lds + 2 * NW * 16);   // [2][NW]
    float *lmin = reinterpret_cast<float *>(fps_lds + FPS_SLOT_BYTES);                          // [min(N, FPS_LDS_POINTS)]
    const int tid = threadIdx.x, wave = tid >> 6, b = blockIdx.x;
    const float *X = pts + (long)b * N * 3;
    const int n = min(max(lengths ? lengths[b] : N, 1), N);
    int s = min(max(start ? start[b] : 0, 0), n - 1);
    const int nl = min(n, FPS_LDS_POINTS);
    float *G = N > FPS_LDS_POINTS ? work + (long)b * (N - FPS_LDS_POINTS) : nullptr;            // G[i - FPS_LDS_POINTS] is mind[i]
    // a lane touches only the mind entries of its own points (i = j T + tid), here and in the loop: no barrier between them
    for (int i = tid; i < nl; i += T) lmin[i] = INFINITY;
    for (int i = FPS_LDS_POINTS + tid; i < n; i += T) G[i - FPS_LDS_POINTS] = INFINITY;
    float sx = X[(long)s * 3], sy = X[(long)s * 3 + 1], sz = X[(long)s * 3 + 2];
    int *I = idx + (long)b * K;
    float *C = cover2 ? cover2 + (long)b * K : nullptr;
    const int rounds = min(K, n);
    for (int k = 0; k < rounds; ++k) {
        float bm = -1.f;                                      // below every mind; ascending i and a strict compare keep the lower index
        int bi = 0;
#pragma unroll 4
        for (int i = tid; i < nl; i += T) {
            const float mm = fminf(lmin[i], fps_pair(X[(long)i * 3], X[(long)i * 3 + 1], X[(long)i * 3 + 2], sx, sy, sz));
            lmin[i] = mm;
            const bool better = mm > bm;
            bm = better ? mm : bm;
            bi = better ? i : bi;
        }
#pragma unroll 4
        for (int i = FPS_LDS_POINTS + tid; i < n; i += T) {
            const float mm = fminf(G[i - FPS_LDS_POINTS], fps_pair(X[(long)i * 3], X[(long)i * 3 + 1], X[(long)i * 3 + 2], sx, sy, sz));
            G[i - FPS_LDS_POINTS] = mm;
            const bool better = mm > bm;
            bm = better ? mm : bm;
            bi = better ? i : bi;
        }
        const unsigned long long key = bm >= 0.f ? fps_key(bm, bi) : 0ull;
        const unsigned long long wmax = fps_wave_max(key);
        const int buf = k & 1;
        if (key == wmax && (key != 0 || (tid & 63) == 0)) {
            skey[buf * NW + wave] = wmax;
            sxyz[buf * NW + wave] = make_float4(X[(long)bi * 3], X[(long)bi * 3 + 1], X[(long)bi * 3 + 2], 0.f);   // bi < n always
        }
        __syncthreads();
        const int picked = s;
        const unsigned long long best = fps_winner<NW>(skey + buf * NW, sxyz + buf * NW, sx, sy, sz);
        s = fps_key_index(best);
        if (tid == 0) {
            I[k] = picked;
            if (C) C[k] = __uint_as_float((unsigned)(best >> 32));
        }
    }
    for (int k = rounds + tid; k < K; k += T) {
        I[k] = -1;
        if (C) C[k] = 0.f;
    }
}

template <int P, int T>
static void fps_resident_launch(const float *pts, int B, int N, const int *lengths, const int *start, int K, int *idx, float *cover2,
                                hipStream_t st) {
    hipLaunchKernelGGL((fps_resident_kernel<P, T>), dim3((unsigned)B), dim3(T), 0, st, pts, N, lengths, start, K, idx, cover2);
}

static long fps_workspace_bytes(long B, long N) { return N > FPS_LDS_POINTS ? 4 * B * (N - FPS_LDS_POINTS) : 0; }

}  // namespace surfd

using namespace surfd;

extern "C" {

int64_t surfd_cloud_fps_workspace_bytes(int B, int N) {
    if (B < 0 || N < 1 || B > FPS_MAX_CLOUDS || N > FPS_MAX_POINTS) return 0;
    return fps_workspace_bytes(B, N);
}

int surfd_cloud_fps(const float *points, int B, int N, const int32_t *lengths, const int32_t *start, int K, int32_t *idx_out,
                    float *cover2_out, void *workspace, surfd_stream s) {
    if (B < 0) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_fps: B = %d is negative", B);
    if (N < 1 || K < 1) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_fps: N = %d, K = %d must be positive", N, K);
    if (B == 0) return SURFD_OK;
    if (!points) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_fps: null points");
    if (!idx_out) SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_fps: null idx_out");
    if (B > FPS_MAX_CLOUDS || N > FPS_MAX_POINTS)
        SURFD_FAIL(SURFD_ERR_UNSUPPORTED, "surfd_cloud_fps: B = %d, N = %d is beyond the supported size (%d clouds of %d points)", B, N,
                   FPS_MAX_CLOUDS, FPS_MAX_POINTS);
    if (fps_workspace_bytes(B, N) > 0 && !workspace)
        SURFD_FAIL(SURFD_ERR_ARG, "surfd_cloud_fps: null workspace (N = %d needs surfd_cloud_fps_workspace_bytes(B, N) = %ld bytes)", N,
                   fps_workspace_bytes(B, N));
    hipStream_t st = as_stream(s);
    if (N <= 64) fps_resident_launch<1, 64>(points, B, N, lengths, start, K, idx_out, cover2_out, st);
    else if (N <= 256) fps_resident_launch<1, 256>(points, B, N, lengths, start, K, idx_out, cover2_out, st);
    else if (N <= 512) fps_resident_launch<2, 256>(points, B, N, lengths, start, K, idx_out, cover2_out, st);
    else if (N <= 1024) fps_resident_launch<4, 256>(points, B, N, lengths, start, K, idx_out, cover2_out, st);
    else if (N <= 2048) fps_resident_launch<8, 256>(points, B, N, lengths, start, K, idx_out, cover2_out, st);
    else if (N <= 4096) fps_resident_launch<16, 256>(points, B, N, lengths, start, K, idx_out, cover2_out, st);
    else if (N <= FPS_RESIDENT_MAX) fps_resident_launch<8, 1024>(points, B, N, lengths, start, K, idx_out, cover2_out, st);
    else {
        const int lds = FPS_SLOT_BYTES + 4 * std::min(N, FPS_LDS_POINTS);
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&fps_stream_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL(fps_stream_kernel, dim3((unsigned)B), dim3(FPS_STREAM_T), lds, st, points, N, lengths, start, K, idx_out,
                           cover2_out, static_cast<float *>(workspace));
    }
    LAUNCH_CHECK();
    return SURFD_OK;
}

}  // extern "C"
