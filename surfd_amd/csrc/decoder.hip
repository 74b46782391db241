// Fused UDF field kernels for gfx950: positional encoding -> 11-layer conditional-BN
// residual MLP -> sigmoid/UDF epilogue, and the same with an in-kernel analytic reverse
// sweep for -normalize(d udf / d p).
//
// Replaces, per point tile, what the reference launches as 20 sin/cos + cat, 34 Conv1d(k=1),
// 11 batch_norm, 11 ReLU (+ a full autograd backward for gradients):
//   CoordsEncoder.encode          AutoEncoder/models/coordsenc.py:25-51
//   DecoderConditionalBatchNorm   AutoEncoder/models/cbndec.py:35-47
//   ConditionalBatchNorm1d        AutoEncoder/models/cbndec.py:68-82   (hoisted to a*x+b tables)
//   ConditionalResnetBlock1d      AutoEncoder/models/cbndec.py:99-103
//   udf_func                      sample/generate_uncond.py:96-101
//   sample_grads                  meshudf/meshudf.py:231-251
//
// Kernel shape (MFMA-bound, exact fp32: v_mfma_f32_32x32x2_f32):
//   one workgroup = 256 threads = 4 waves (one per SIMD), tile = 64 points x 512 channels.
//   Wave w owns output channels [128w,128w+128): 2 (point tiles) x 4 (channel tiles)
//   accumulators of 32x32 -> the residual stream lives in 128 accumulator registers and
//   never leaves the register file; the activation that feeds the next GEMM goes through
//   one LDS buffer X[64][516] (row stride 516 floats: conflict-free ds_read_b128 A-fragments).
//   Weights are pre-packed fragment-major (common.h) and streamed from L2/MALL with one
//   fully coalesced 16-byte load per lane per 4 MFMAs.
//   Algorithmic work: 5 308 416 FLOP per forward point, x3 for a gradient point.
#include "common.h"
#include "paramtable.h"
#include "points.h"
#include <string.h>
#include <stdlib.h>
#include <type_traits>
#include <utility>

namespace surfd {

constexpr int H = 512;        // hidden width
constexpr int NB = 5;         // residual blocks
constexpr int NCBN = 2 * NB + 1;
constexpr int TP = 64;        // points per tile
constexpr int XS = H + 4;     // LDS row stride of X
constexpr int ES = 68;        // LDS row stride of the 64-wide encoding / its adjoint
constexpr int KG_H = H / 8;   // k-groups of a 512-deep contraction
constexpr int KG_E = 8;       // k-groups of the 64-deep (63 + pad) first layer

// private weight arena (floats): all MFMA-packed matrices in one buffer, all vectors in another,
// so that every kernel-side address is one base pointer + a compile-time offset
constexpr size_t SZ_FCP = (size_t)16 * KG_E * 256;     // packed fc_p       [16][8][64][4]
constexpr size_t SZ_HH = (size_t)16 * KG_H * 256;      // packed 512x512    [16][64][64][4]
constexpr size_t SZ_FCPT = (size_t)2 * KG_H * 256;     // packed fc_p^T     [2][64][64][4]
constexpr size_t OFF_FCP = 0;
__host__ __device__ constexpr size_t off_fc(int k, int which) { return SZ_FCP + (size_t)(2 * k + which) * SZ_HH; }
__host__ __device__ constexpr size_t off_fcT(int k, int which) { return SZ_FCP + (size_t)(2 * NB + 2 * k + which) * SZ_HH; }
constexpr size_t OFF_FCPT = SZ_FCP + (size_t)4 * NB * SZ_HH;
constexpr size_t WPACK_FLOATS = OFF_FCPT + SZ_FCPT;
constexpr int VOFF_BFCP = 0;
__host__ __device__ constexpr int voff_bfc(int k, int which) { return H * (1 + 2 * k + which); }
constexpr int VOFF_WOUT = H * (1 + 2 * NB);
constexpr int VOFF_BOUT = H * (2 + 2 * NB);
// f16x2 kernels: the biases that would be added to the residual stream are folded into the shift of the next conditional
// BN instead (a*(net + CB) + b = a*net + (a*CB + b)): CB[k] = b_fc_p + sum_{j<k} b_fc_1[j], built at finalize.  The
// accumulators are then never touched by the vector ALU between the matrix products (no AGPR -> VGPR -> AGPR round trips).
__host__ __device__ constexpr int voff_cb(int k) { return VOFF_BOUT + 4 + H * k; }
constexpr int VEC_FLOATS = VOFF_BOUT + 4 + H * (NB + 1);

// ---- "f16x2" arithmetic (default; surfd_decoder_set_precision / SURFD_DECODER_PRECISION) -----------------
// Every fp32 operand is split into two fp16 terms, x = xh + xl with |x - xh - xl| <= 2^-22 |x|, and the
// three products xh*wh + xh*wl + xl*wh are accumulated in fp32 on the fp16 matrix pipe
// (v_mfma_f32_32x32x16_f16, 16x the fp32 MFMA rate): 16/3 = 5.3x the fp32 matrix rate at fp32-class
// accuracy (measured error vs an fp64 evaluation is the same size as the fp32 kernel's own).
//  * weights are multiplied by one power of two SC (max |W|*SC in [256, 512)) before the split so that
//    the low terms stay in fp16's normal range; SC is folded back exactly in the epilogues;
//  * activations live in LDS already split (the producing epilogue splits each value once): row p of
//    X is [256 words of high halves][256 words of low halves][4 pad], word w = two consecutive k-slots;
//    k-slot order is chosen so that the epilogue's natural register pairs are the two halves of a word:
//        slot s -> channel 128*(s>>7) + 64*((s>>6)&1) + 32*(s&1) + ((s>>1)&31)
//  * activations saturate at 65504 (fp16 max) in this mode (counted in DecParams.sat); the fp32 path has no such limit;
//  * the reverse sweep uses the same machinery with the transposed matrices; its operand (the adjoint, no natural
//    range) is scaled per 64-point tile by one power of two so that the tile maximum lands in [2^14, 2^15).
// Weight planes, fragment-major for the 32x32x16 MFMA:
//   whf[(((tile*KS + ks)*2 + plane)*64 + lane)*8 + e] = plane(SC * W[tile*32 + (lane&31)][chan(ks*16 + 8*(lane>>5) + e)])
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int KS_H = H / 16;                  // k16 steps of a 512-deep contraction
constexpr int KS_E = 4;                       // k16 steps of the 64-deep first layer
constexpr size_t HF_FCP = (size_t)16 * KS_E * 2 * 64 * 8;     // fp16 elements
constexpr size_t HF_HH = (size_t)16 * KS_H * 2 * 64 * 8;
__host__ __device__ constexpr size_t hf_off_fc(int k, int which) { return HF_FCP + (size_t)(2 * k + which) * HF_HH; }
// transposed hidden matrices (reverse sweep in f16x2): same fragment layout and k-slot order, after the forward ones
__host__ __device__ constexpr size_t hf_off_fcT(int k, int which) { return HF_FCP + (size_t)(2 * NB + 2 * k + which) * HF_HH; }
constexpr size_t WHF_ELEMS = HF_FCP + (size_t)4 * NB * HF_HH;
constexpr int VOFF_SC = VOFF_BOUT + 1;        // SC, 1/SC (floats) and max|W| bits, after b_out
// SURFD_DEC_OVL (experiment, default OFF): the k-slot order puts the first two channel tiles of EVERY wave into the first
// half of K,   slot s -> channel 128*((s>>6)&3) + 32*(2*(s>>8) + (s&1)) + ((s>>1)&31),
// so that a GEMM can start on the half of its operand that the preceding epilogue has finished while the other half of
// that epilogue is issued BETWEEN the MFMAs of the GEMM's first half (forward kernel, below).  Built, bit-correct (every
// decoder / grid test green), measured (profiles/r03_decoder_variants.md): 435 vs 429-434 TFLOP/s.  The phase stamps say why:
// the half-epilogue costs the same ~3.5 k cycles inside the GEMM as in front of it.  With ONE wave per SIMD every
// instruction issued between two MFMAs opens a ~6-cycle bubble in the matrix pipe (MI355X_MICROARCH.md: "between MFMAs on
// DIFFERENT accumulators ~6 cyc/state"; the same 6 cycles x 12 memory instructions per 24 MFMAs are the GEMM loops' own 9 %
// loss) — vector work does not hide under the same wave's MFMAs; it would take a second wave per SIMD, i.e. half the
// registers per wave.  Kept as the record of that measurement; costs 25 spilled registers, so it is not the default.
#ifndef SURFD_DEC_OVL
#define SURFD_DEC_OVL 0
#endif
constexpr bool DEC_OVL = SURFD_DEC_OVL != 0;
__host__ __device__ constexpr int slot_channel(int s) {
    return DEC_OVL ? 128 * ((s >> 6) & 3) + 32 * (2 * (s >> 8) + (s & 1)) + ((s >> 1) & 31)
                   : 128 * (s >> 7) + 64 * ((s >> 6) & 1) + 32 * (s & 1) + ((s >> 1) & 31);
}
constexpr int XW_WAVE = DEC_OVL ? 32 : 64;     // word stride of a wave's / of a tile pair's block inside one fp16 plane of an X row
constexpr int XW_Q = DEC_OVL ? 128 : 32;

struct DecParams {
    const float *wpack;   // WPACK_FLOATS
    const _Float16 *whf;  // WHF_ELEMS (f16x2 kernels only)
    const float *vecs;    // VEC_FLOATS: biases, w_out, b_out
    const float *tab;     // [S][NCBN][2][H] scale/shift tables of the bound latents
    int input_dim;
    unsigned *sat;        // f16x2 forward path: waves that saw an activation beyond the fp16 range (it is clamped)
};

typedef float __attribute__((address_space(1))) gfloat;
typedef f32x4 __attribute__((address_space(1))) gf32x4;

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// acc[mt][nt] += A[64 x 8*KG] (LDS, row stride astride) * Wp(4 channel tiles of this wave)
// Software pipeline: weight fragments of k-group kg+1 are requested before the 32 MFMAs of
// k-group kg are issued (ping-pong register sets, no copies), so one k-group of MFMA time
// (2048 cycles) covers the L2/MALL latency.
__device__ __forceinline__ void mfma_group(const f32x4 &x0, const f32x4 &x1, const f32x4 (&b)[4], f32x16 (&acc)[2][4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            acc[0][nt] = mfma(x0[q], b[nt][q], acc[0][nt]);
            acc[1][nt] = mfma(x1[q], b[nt][q], acc[1][nt]);
        }
    }
}

template <int KG>
__device__ __forceinline__ void gemm_2x4(const float *A, int astride, const gfloat *Wp, f32x16 (&acc)[2][4], int lane) {
    static_assert(KG % 2 == 0, "k-group count must be even");
    const float *a0 = A + (lane & 31) * astride + 4 * (lane >> 5);
    const float *a1 = a0 + 32 * astride;
    const gf32x4 *w = reinterpret_cast<const gf32x4 *>(Wp) + lane;
    f32x4 bA[4], bB[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) bA[nt] = w[(nt * KG) * 64];
    f32x4 xa0 = *reinterpret_cast<const f32x4 *>(a0), xa1 = *reinterpret_cast<const f32x4 *>(a1);
#pragma unroll 1
    for (int kg = 0; kg < KG; kg += 2) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) bB[nt] = w[(nt * KG + kg + 1) * 64];
        const f32x4 xb0 = *reinterpret_cast<const f32x4 *>(a0 + (kg + 1) * 8);
        const f32x4 xb1 = *reinterpret_cast<const f32x4 *>(a1 + (kg + 1) * 8);
        __builtin_amdgcn_sched_barrier(0);
        mfma_group(xa0, xa1, bA, acc);
        __builtin_amdgcn_sched_barrier(0);
        const int k2 = (kg + 2 < KG) ? kg + 2 : kg;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) bA[nt] = w[(nt * KG + k2) * 64];
        xa0 = *reinterpret_cast<const f32x4 *>(a0 + k2 * 8);
        xa1 = *reinterpret_cast<const f32x4 *>(a1 + k2 * 8);
        __builtin_amdgcn_sched_barrier(0);
        mfma_group(xb0, xb1, bB, acc);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// two fp32 values -> (high halves, low halves), each a packed pair
__device__ __forceinline__ void split2(const f32x2 u, unsigned &hi, unsigned &lo) {
    const f16x2 h = __builtin_convertvector(u, f16x2);
    const f32x2 r = u - __builtin_convertvector(h, f32x2);
    const f16x2 l = __builtin_convertvector(r, f16x2);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}

typedef f16x8 __attribute__((address_space(1))) gf16x8;

// low fp16 halves of a split pair, packed: f16(u - f32(h)) per half, the subtraction exact in fp32 as in split2 — as two
// mixed-precision FMAs (h * -1 + u with an fp16 operand and an fp16 result written to one half of the register) instead of
// two conversions back, a packed subtraction and a packed conversion: 2 instructions instead of 4 per pair in the epilogues
#ifndef SURFD_DEC_MIX
#define SURFD_DEC_MIX 1
#endif
#ifndef SURFD_DEC_GRAD_W
#define SURFD_DEC_GRAD_W 2        // value pairs of the gradient kernel's epilogues processed stage by stage (2 / 4 / 8: 35 / 37 / 46 spilled registers, 413 TFLOP/s each)
#endif
#ifndef SURFD_DEC_GRAD_MIX
#define SURFD_DEC_GRAD_MIX 0      // the same two mixed FMAs in the gradient kernel's epilogues: 8 % fewer epilogue instructions, 46 instead of 37 spilled registers, 411.7 against 413.4 TFLOP/s
#endif
__device__ __forceinline__ unsigned split_low_pair(unsigned h, float u0, float u1) {
#if SURFD_DEC_MIX
    unsigned l;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "=&v"(l) : "v"(h), "v"(u0), "v"(u1));
    return l;
#else
    const f16x2 hh = __builtin_bit_cast(f16x2, h);
    const f32x2 hf = __builtin_convertvector(hh, f32x2);
    const f32x2 rr = {u0 - hf.x, u1 - hf.y};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(rr, f16x2));
#endif
}

__device__ __forceinline__ void mfma_step_f16x2(const f16x8 (&a)[2][2], const f16x8 (&b)[4][2], f32x16 (&acc)[2][4]) {
    // term-major: the 8 accumulators are independent, so consecutive MFMAs never wait on each other;
    // small terms first
    constexpr int TA[3] = {1, 0, 0};     // activation plane
    constexpr int TB[3] = {0, 1, 0};     // weight plane
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mt][TA[t]], b[nt][TB[t]], acc[mt][nt], 0, 0, 0);
}

// acc[mt][nt] += A[64 x 16*KS] (split fp16 planes in LDS) * W (two fp16 planes, 4 channel tiles of this wave).
// One k-step is 24 MFMAs = 768 matrix-pipe cycles.  The weight stream is software-pipelined ACROSS the
// GEMMs of a tile: D register stages rotate, stage (ks + D-1) is requested while k-step ks computes, and
// the last D-1 k-steps of a GEMM already request the first stages of the NEXT matrix (weights do not
// depend on activations), so the L2 latency at every layer boundary hides behind the epilogue.
// The 8 weight loads and 4 activation-fragment LDS reads of a k-step are interleaved one per MFMA.
struct WStages { f16x8 b[4][4][2]; };        // D = 4 stages x 4 channel tiles x 2 planes
// Stages of the NEXT matrix that the tail of a GEMM requests (they stay live through the epilogue in between, the point
// of highest register pressure: both accumulator sets, the epilogue's temporaries).  D - 1 = 3 keeps the pipeline full
// across the boundary; 2 leaves 32 more registers to the epilogue and requests the third stage when the next GEMM
// starts (its k-steps 0 and 1, 1536 matrix-pipe cycles, cover that load's latency).
#ifndef SURFD_DEC_WS_AHEAD
#define SURFD_DEC_WS_AHEAD 0
#endif
constexpr int WS_AHEAD = SURFD_DEC_WS_AHEAD;
// where the left-out stages are requested: 0 = when the GEMM starts, 1 = by the caller before the barrier in front of the
// GEMM, 2 = the first of them before that barrier and the others at the start (measured, profiles/r03_decoder_variants.md:
// forward 425 / 392-410 / 434 TFLOP/s; 2 leaves the forward kernel without a single spilled register)
#ifndef SURFD_DEC_REQ_EARLY
#define SURFD_DEC_REQ_EARLY 2
#endif
constexpr bool REQ_EARLY = SURFD_DEC_REQ_EARLY != 0;
constexpr int REQ_EARLY_UPTO = SURFD_DEC_REQ_EARLY == 2 ? WS_AHEAD + 1 : 3;      // 2: only the first left-out stage goes early, the rest at GEMM start
#ifndef SURFD_DEC_FWD_STAGED
#define SURFD_DEC_FWD_STAGED 0
#endif
constexpr bool FWD_STAGED = SURFD_DEC_FWD_STAGED != 0;   // forward kernel's epilogue in the gradient kernel's four-pairs-per-stage form

template <int KS>
__device__ __forceinline__ void load_wstage(f16x8 (&dst)[4][2], const _Float16 *Whf, unsigned lofs, int ks) {
    // uniform base (SGPRs) + 32-bit per-lane byte offset: fragment (nt, ks, plane) at ((nt*KS + ks)*2 + plane) KiB
    // The four channel-tile bases are re-derived from the one matrix base at every use (two scalar adds each): kept live
    // as four SGPR pairs per matrix they were spilled in the rolled layer loop, and every reload of a spilled scalar is a
    // scratch load + s_waitcnt vmcnt(0) — a full drain of the weight pipeline in the middle of the GEMM.
    const unsigned long long wa = (unsigned long long)Whf;
    unsigned wlo = __builtin_amdgcn_readfirstlane((unsigned)wa), whi = __builtin_amdgcn_readfirstlane((unsigned)(wa >> 32));
    asm volatile("" : "+s"(wlo), "+s"(whi));
    const __attribute__((address_space(1))) char *wb = (const __attribute__((address_space(1))) char *)(((unsigned long long)whi << 32) | wlo);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int q = 0; q < 2; ++q)
            dst[nt][q] = *reinterpret_cast<const gf16x8 *>(wb + (size_t)(nt * KS * 2048) + (lofs + (unsigned)((ks * 2 + q) * 1024)));
}

// first D-1 stages of a matrix (once per kernel, before the first tile)
template <int KS>
__device__ __forceinline__ void gemm_prefetch_f16x2(WStages &ws, const _Float16 *Whf, int lane) {
    unsigned lofs = (unsigned)lane * 16u;
    asm volatile("" : "+v"(lofs));
#pragma unroll
    for (int d = 0; d < WS_AHEAD; ++d) load_wstage<KS>(ws.b[d], Whf, lofs, d);
}

// the stages of a matrix that the previous GEMM's tail left out: requested by the caller once its epilogue's stores are
// issued, BEFORE the barrier in front of the GEMM (the barrier wait and the accumulator set-up then cover the latency)
template <int KS>
__device__ __forceinline__ void gemm_request_f16x2(WStages &ws, const _Float16 *Whf, int lane) {
    if constexpr (WS_AHEAD < 3 && REQ_EARLY) {
        __builtin_amdgcn_sched_barrier(0);          // not hoisted into the epilogue: that is where the registers are needed
        unsigned lofs = (unsigned)lane * 16u;
        asm volatile("" : "+v"(lofs));
#pragma unroll
        for (int d = WS_AHEAD; d < REQ_EARLY_UPTO; ++d) load_wstage<KS>(ws.b[d], Whf, lofs, d);
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int KS, int KSN>
__device__ __forceinline__ void gemm_2x4_f16x2(const float *A, const _Float16 *Whf, const _Float16 *Wnext, WStages &ws,
                                               f32x16 (&acc)[2][4], int lane) {
    constexpr int D = 4;
    static_assert(KS % D == 0 && KSN >= D - 1, "k-step count must be a multiple of the pipeline depth");
    const float *a0 = A + (lane & 31) * XS + 4 * (lane >> 5);
    const float *a1 = a0 + 32 * XS;
    unsigned lofs = (unsigned)lane * 16u;
    asm volatile("" : "+v"(lofs));      // keep the per-fragment offsets 32-bit adds, not hoisted 64-bit addresses
    f16x8 x[2][2][2];
    auto load_x = [&](f16x8 (&dst)[2][2], int ks) {
        dst[0][0] = *reinterpret_cast<const f16x8 *>(a0 + ks * 8); dst[0][1] = *reinterpret_cast<const f16x8 *>(a0 + 256 + ks * 8);
        dst[1][0] = *reinterpret_cast<const f16x8 *>(a1 + ks * 8); dst[1][1] = *reinterpret_cast<const f16x8 *>(a1 + 256 + ks * 8);
    };
    auto load_xg = [&](f16x8 (&dst)[2][2], int goff, int j) {       // k-step j of the group whose first operand column is goff
        dst[0][0] = *reinterpret_cast<const f16x8 *>(a0 + goff + j * 8); dst[0][1] = *reinterpret_cast<const f16x8 *>(a0 + goff + 256 + j * 8);
        dst[1][0] = *reinterpret_cast<const f16x8 *>(a1 + goff + j * 8); dst[1][1] = *reinterpret_cast<const f16x8 *>(a1 + goff + 256 + j * 8);
    };
    auto group = [&](int ks0, auto last) {
        // the group's LDS operand addresses are two registers (both point tiles) + immediates, re-derived here: as loop-carried
        // induction variables there were six of them, spilled, and a reloaded address is a scratch load + vmcnt(0) in the GEMM
        int goff = ks0 * 8;
        asm volatile("" : "+v"(goff));
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int ks = ks0 + j;
            if (decltype(last)::value && j >= 1) { if (j - 1 < WS_AHEAD) load_wstage<KSN>(ws.b[(j + D - 1) % D], Wnext, lofs, j - 1); }
            else load_wstage<KS>(ws.b[(j + D - 1) % D], Whf, lofs, ks + D - 1);
            load_xg(x[(j + 1) & 1], goff, (decltype(last)::value && j == D - 1) ? j : j + 1);
            mfma_step_f16x2(x[j & 1], ws.b[j], acc);
            // issue order: one memory instruction per MFMA, then the remaining MFMAs
#pragma unroll
            for (int i = 0; i < 8; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); }
#pragma unroll
            for (int i = 0; i < 4; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
            __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    load_x(x[0], 0);
#pragma unroll
    for (int d = REQ_EARLY ? REQ_EARLY_UPTO : WS_AHEAD; d < D - 1; ++d) load_wstage<KS>(ws.b[d], Whf, lofs, d);
#pragma unroll 1
    for (int ks0 = 0; ks0 < KS - D; ks0 += D) group(ks0, std::false_type{});
    group(KS - D, std::true_type{});
}

template <int... I, typename F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F &&f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f) { static_for_impl(std::make_integer_sequence<int, N>{}, f); }

// k-steps [BEG, BEG + 16) of a 32-step GEMM (forward kernel with SURFD_DEC_OVL).  BEG = 0: stage 0 was requested by the
// caller before the barrier, stages 1 and 2 are requested here; BEG = 16 continues the ring across the barrier in between.
// WITH_CHUNKS: fully unrolled, chunk(idx) (idx = k-step - BEG, a compile-time constant) contributes a slice of the preceding
// epilogue's second half to every k-step's scheduling region — 2 value pairs = ~30 vector / LDS instructions next to 24
// MFMAs of 32 cycles each, i.e. in issue slots the matrix pipe leaves free.
template <int BEG, bool WITH_CHUNKS, typename ChunkFn>
__device__ __forceinline__ void gemm_half_f16x2(const float *A, const _Float16 *Whf, WStages &ws, f32x16 (&acc)[2][4], int lane, ChunkFn &&chunk) {
    constexpr int D = 4, KS = KS_H, END = BEG + 16;
    const float *a0 = A + (lane & 31) * XS + 4 * (lane >> 5);
    const float *a1 = a0 + 32 * XS;
    unsigned lofs = (unsigned)lane * 16u;
    asm volatile("" : "+v"(lofs));
    f16x8 x[2][2][2];
    auto load_x = [&](f16x8 (&dst)[2][2], int ks) {
        dst[0][0] = *reinterpret_cast<const f16x8 *>(a0 + ks * 8); dst[0][1] = *reinterpret_cast<const f16x8 *>(a0 + 256 + ks * 8);
        dst[1][0] = *reinterpret_cast<const f16x8 *>(a1 + ks * 8); dst[1][1] = *reinterpret_cast<const f16x8 *>(a1 + 256 + ks * 8);
    };
    load_x(x[0], BEG);
    if constexpr (BEG == 0) {
#pragma unroll
        for (int d = REQ_EARLY ? REQ_EARLY_UPTO : 0; d < D - 1; ++d) load_wstage<KS>(ws.b[d], Whf, lofs, d);
    }
    if constexpr (WITH_CHUNKS) {
        static_for<16>([&](auto idx) {
            constexpr int ks = BEG + decltype(idx)::value, j = ks % D;
            if constexpr (ks + D - 1 < KS) load_wstage<KS>(ws.b[(j + D - 1) % D], Whf, lofs, ks + D - 1);
            if constexpr (ks + 1 < END) load_x(x[(ks + 1) & 1], ks + 1);
            chunk(idx);
            mfma_step_f16x2(x[ks & 1], ws.b[j], acc);
#pragma unroll
            for (int i = 0; i < 8; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 1, 0); }
#pragma unroll
            for (int i = 0; i < 4; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 2, 0); }
#pragma unroll
            for (int i = 0; i < 8; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, 2, 0); }
#pragma unroll
            for (int i = 0; i < 4; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x200, 1, 0); }
            __builtin_amdgcn_sched_barrier(0);
        });
    } else {
        auto group = [&](int ks0, auto last) {
            int goff = ks0 * 8;
            asm volatile("" : "+v"(goff));
#pragma unroll
            for (int j = 0; j < D; ++j) {
                // (the last group of the matrix has one stage left to request, at j = 0)
                if (!decltype(last)::value || j == 0) load_wstage<KS>(ws.b[(j + D - 1) % D], Whf, lofs, ks0 + j + D - 1);
                const int jn = (decltype(last)::value && j == D - 1) ? j : j + 1;
                x[(j + 1) & 1][0][0] = *reinterpret_cast<const f16x8 *>(a0 + goff + jn * 8); x[(j + 1) & 1][0][1] = *reinterpret_cast<const f16x8 *>(a0 + goff + 256 + jn * 8);
                x[(j + 1) & 1][1][0] = *reinterpret_cast<const f16x8 *>(a1 + goff + jn * 8); x[(j + 1) & 1][1][1] = *reinterpret_cast<const f16x8 *>(a1 + goff + 256 + jn * 8);
                mfma_step_f16x2(x[j & 1], ws.b[j], acc);
#pragma unroll
                for (int i = 0; i < 8; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); }
#pragma unroll
                for (int i = 0; i < 4; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
                __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        static_assert(END == KS, "the rolled half is the second one");
#pragma unroll 1
        for (int ks0 = BEG; ks0 < END - D; ks0 += D) group(ks0, std::false_type{});
        group(END - D, std::true_type{});
    }
}

// one 32x32 tile: rows = points [32*mt, +32), cols = packed tile `Wp_tile`
template <int KG>
__device__ __forceinline__ void gemm_1x1(const float *A, int astride, int mt, const gfloat *Wp_tile, f32x16 &acc, int lane) {
    const float *a0 = A + (32 * mt + (lane & 31)) * astride + 4 * (lane >> 5);
    const gf32x4 *w = reinterpret_cast<const gf32x4 *>(Wp_tile) + lane;
#pragma unroll 4
    for (int kg = 0; kg < KG; ++kg) {
        const f32x4 x0 = *reinterpret_cast<const f32x4 *>(a0 + kg * 8);
        const f32x4 b = w[kg * 64];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = mfma(x0[q], b[q], acc);
    }
}

__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2][4]) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
}

// bit position of accumulator element (mt, nt, r) in a lane's 128-bit ReLU mask
__device__ __forceinline__ constexpr int mword(int mt, int nt) { return (mt * 4 + nt) >> 1; }
__device__ __forceinline__ constexpr int mbit(int mt, int nt, int r) { return ((mt * 4 + nt) & 1) * 16 + r; }

// Positional encoding of a 64-point tile (reference AutoEncoder/models/coordsenc.py: x, then per frequency 2^f, f = 0..9,
// [sin(2^f x), sin(2^f y), sin(2^f z), cos(2^f x), cos(2^f y), cos(2^f z)]; column 63 is the pad) straight into the split
// fp16 planes of X's rows (identity k-slot order: feature j = half j of the high plane, the low plane 512 halves behind).
// TPP threads per point; thread `part` takes the (coordinate, frequency) pairs part, part + TPP, ... of the 30: ONE range
// reduction per angle gives both its features (the old form evaluated a generic feature(j) — index arithmetic, both sinf
// and cosf — per column: 3.4 % of a tile's cycles, profiles/r03_decoder_variants.md).  Pre-encoded inputs (PT_EMB) are copied.
template <int TPP>
__device__ __forceinline__ void encode_tile_f16x2(const PtIO &io, long e0, long npts, const float *PT, float *X, int tid, int &sat_flag) {
    constexpr int LOG2 = TPP == 8 ? 3 : 2;
    static_assert(TPP == 4 || TPP == 8, "threads per point");
    const int p = tid >> LOG2, part = tid & (TPP - 1);
    _Float16 *hrow = reinterpret_cast<_Float16 *>(reinterpret_cast<unsigned *>(X) + p * XS);
    auto put = [&](int j, float u) {
        const _Float16 h = (_Float16)u;
        hrow[j] = h;
        hrow[512 + j] = (_Float16)(u - (float)h);
    };
    if (io.mode == PT_EMB) {
        const long e = e0 + p;
        bool bad = false;
#pragma unroll 2
        for (int i = 0; i < 64 / TPP; ++i) {
            const int j = part * (64 / TPP) + i;
            float u = (e < npts && j < io.emb_dim) ? io.xyz[e * io.emb_dim + j] : 0.f;
            bad |= __builtin_fabsf(u) > 65504.f;
            u = __builtin_amdgcn_fmed3f(u, -65504.f, 65504.f);
            put(j, u);
        }
        sat_flag |= __any(bad);
        return;
    }
    const float x = PT[p * 4 + 0], y = PT[p * 4 + 1], z = PT[p * 4 + 2];
    {
        float u = part == 0 ? x : (part == 1 ? y : z);
        const bool bad = part < 3 && __builtin_fabsf(u) > 65504.f;
        sat_flag |= __any(bad);
        u = __builtin_amdgcn_fmed3f(u, -65504.f, 65504.f);
        if (part < 3) put(part, u);
        if (part == 3) put(63, 0.f);
    }
    int f = part / 3, r = part - 3 * (part / 3);
#pragma unroll
    for (int q0 = 0; q0 < 30; q0 += TPP) {
        if (q0 + part < 30) {
            const float a = (r == 0 ? x : (r == 1 ? y : z)) * (float)(1 << f);      // exact: power-of-two scale
            float sn, cs;
            sincosf(a, &sn, &cs);
            put(3 + 6 * f + r, sn);
            put(6 + 6 * f + r, cs);
        }
        r += TPP % 3; f += TPP / 3;
        if (r >= 3) { r -= 3; ++f; }
    }
}

// Optional phase timing of the forward kernel (-DSURFD_DEC_STAMPS, debugging only): shader-clock cycles of
// workgroup 0 / wave 0 accumulated per phase: 0 fetch+encode, 1 GEMM loops, 2 epilogues, 3 barrier waits, 4 output
#ifdef SURFD_DEC_STAMPS
__device__ long long g_dec_stamps[8];
#define TDECL() long long tacc_[5] = {0, 0, 0, 0, 0}, t0_ = __builtin_readcyclecounter()
#define TADD(slot) do { const long long t1_ = __builtin_readcyclecounter(); tacc_[slot] += t1_ - t0_; t0_ = t1_; } while (0)
#define TBAR() do { TADD(tphase_); __syncthreads(); TADD(3); } while (0)
#define TPHASE(x) tphase_ = (x)
#define TFLUSH() do { if (blockIdx.x == 0 && threadIdx.x == 0) { for (int i_ = 0; i_ < 5; ++i_) g_dec_stamps[i_] += tacc_[i_]; g_dec_stamps[5] += 1; } } while (0)
#else
#define TDECL()
#define TADD(slot)
#define TBAR() __syncthreads()
#define TPHASE(x)
#define TFLUSH()
#endif

template <bool GRAD, bool F16X2 = false>
__global__ __launch_bounds__(256, 1) void decoder_kernel(DecParams P, PtBatch B) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *X = lds;                      // [TP][XS]
    float *E = lds;                      // [TP][ES] first-layer input, aliases X (dead before X is written)
    float *PT = lds + TP * XS;           // [TP][4]: x, y, z, voxel index bits
    float *LOG = PT + TP * 4;            // [TP]
    float *E2 = LOG + TP;                // [TP][ES] d logit / d enc          (GRAD only)
    float *DV = E2 + TP * ES;            // [TP][4]  d logit / d xyz          (GRAD only)
    float *RED = DV + TP * 4;            // [4] per-wave maxima of the adjoint   (GRAD && F16X2 only)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);      // provably uniform: keeps weight bases in SGPRs
    // per-lane LDS bases of this wave's accumulator footprint in X (one per point tile): every
    // element (mt, nt, r) is then base + compile-time offset (< 64 KB, fits the ds immediate)
    typedef float __attribute__((address_space(3))) lds_f32;       // LDS-typed: stays a ds_write through the asm below
    lds_f32 *xb0 = (lds_f32 *)(X + (4 * (lane >> 5)) * XS + 128 * wave + col);
    lds_f32 *xb1 = xb0 + 32 * XS;
    // In front of a block of XAT stores in the f16x2 gradient kernel: makes the two bases opaque at that point, so the ~64
    // (base + constant) addresses the stores need are formed there, next to their use, instead of in the kernel prologue —
    // from where the register allocator carried them through every GEMM in scratch (88 of the kernel's spilled registers)
    auto fresh_xat_bases = [&]() { if constexpr (GRAD && F16X2) asm volatile("" : "+v"(xb0), "+v"(xb1)); };
#define XAT(mt, nt, r) ((mt) ? xb1 : xb0)[(((r) & 3) + 8 * ((r) >> 2)) * XS + 32 * (nt)]
    // f16x2 mode: word (wave, q, col) of plane `pl` in the same rows (see the layout comment at the top)
    typedef unsigned __attribute__((address_space(3))) lds_u32;
    lds_u32 *xw0 = (lds_u32 *)(reinterpret_cast<unsigned *>(X) + (4 * (lane >> 5)) * XS + XW_WAVE * wave + col);
    lds_u32 *xw1 = xw0 + 32 * XS;
#define XW(mt, q, r, pl) ((mt) ? xw1 : xw0)[(((r) & 3) + 8 * ((r) >> 2)) * XS + XW_Q * (q) + 256 * (pl)]
    // X <- split(min(relu(a*v + b), 65504)) for this wave's accumulator footprint (a, b per channel tile).
    // Scalar fp32 ops on purpose: packed-f32 ops would need register pairs built from two accumulator
    // tiles (copies + spills), and this mode has no bitwise contract, so the affine map is one fma.
    int sat_flag = 0;      // wave-uniform: some lane of this wave produced an activation beyond the fp16 range (f16x2 mode)
    auto store_split = [&](const f32x16 (&v)[2][4], const float (&sa)[4], const float (&sb)[4], unsigned *mk, auto qn) {
        float umax = 0.f;  // local to one epilogue: a value kept across the GEMM loops would cost spills in the hot loop
#pragma unroll
        for (int q = 0; q < decltype(qn)::value; ++q)          // qn = 1: only the tile pair that forms the first half of K (SURFD_DEC_OVL)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                if constexpr (!GRAD && !FWD_STAGED) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float t0 = __builtin_fmaf(sa[2 * q], v[mt][2 * q][r], sb[2 * q]);
                        const float t1 = __builtin_fmaf(sa[2 * q + 1], v[mt][2 * q + 1][r], sb[2 * q + 1]);
                        umax = __builtin_fmaxf(__builtin_fmaxf(umax, t0), t1);          // one v_max3_f32 per pair (the other nesting costs 1.5): range accounting
                        const float u0 = __builtin_amdgcn_fmed3f(t0, 0.f, 65504.f);
                        const float u1 = __builtin_amdgcn_fmed3f(t1, 0.f, 65504.f);
                        const f32x2 u = {u0, u1};
                        const unsigned h = __builtin_bit_cast(unsigned, __builtin_convertvector(u, f16x2));      // one v_cvt_pk_f16_f32
                        XW(mt, q, r, 0) = h;
                        XW(mt, q, r, 1) = split_low_pair(h, u0, u1);
                    }
                    continue;
                }
                // gradient kernel (more live state: gates, both accumulators): one accumulator-tile pair at a time bounds
                // the live ranges, and SURFD_DEC_GRAD_W independent value pairs are processed stage by stage (measured +6 %)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int r0 = 0; r0 < 16; r0 += SURFD_DEC_GRAD_W) {
                    float t0[SURFD_DEC_GRAD_W], t1[SURFD_DEC_GRAD_W];
                    f32x2 u[SURFD_DEC_GRAD_W];
                    f16x2 h[SURFD_DEC_GRAD_W];
                    unsigned l[SURFD_DEC_GRAD_W];
#pragma unroll
                    for (int i = 0; i < SURFD_DEC_GRAD_W; ++i) {
                        t0[i] = __builtin_fmaf(sa[2 * q], v[mt][2 * q][r0 + i], sb[2 * q]);
                        t1[i] = __builtin_fmaf(sa[2 * q + 1], v[mt][2 * q + 1][r0 + i], sb[2 * q + 1]);
                    }
#pragma unroll
                    for (int i = 0; i < SURFD_DEC_GRAD_W; ++i) {
                        umax = __builtin_fmaxf(__builtin_fmaxf(umax, t0[i]), t1[i]);      // one v_max3_f32: range accounting
                        if constexpr (GRAD) {                                             // ReLU gates for the reverse sweep
                            mk[mword(mt, 2 * q)] |= t0[i] > 0.f ? 1u << mbit(mt, 2 * q, r0 + i) : 0u;              // branch-free: compare, select, or
                            mk[mword(mt, 2 * q + 1)] |= t1[i] > 0.f ? 1u << mbit(mt, 2 * q + 1, r0 + i) : 0u;
                        }
                        u[i].x = __builtin_amdgcn_fmed3f(t0[i], 0.f, 65504.f);
                        u[i].y = __builtin_amdgcn_fmed3f(t1[i], 0.f, 65504.f);
                    }
#pragma unroll
                    for (int i = 0; i < SURFD_DEC_GRAD_W; ++i) h[i] = __builtin_convertvector(u[i], f16x2);      // one v_cvt_pk_f16_f32
#pragma unroll
                    for (int i = 0; i < SURFD_DEC_GRAD_W; ++i) {
#if SURFD_DEC_GRAD_MIX
                        l[i] = split_low_pair(__builtin_bit_cast(unsigned, h[i]), u[i].x, u[i].y);      // same bits as convert back, subtract, convert
#else
                        l[i] = __builtin_bit_cast(unsigned, __builtin_convertvector(u[i] - __builtin_convertvector(h[i], f32x2), f16x2));
#endif
                    }
#pragma unroll
                    for (int i = 0; i < SURFD_DEC_GRAD_W; ++i) {
                        XW(mt, q, r0 + i, 0) = __builtin_bit_cast(unsigned, h[i]);
                        XW(mt, q, r0 + i, 1) = l[i];
                    }
                }
            }
        sat_flag |= __any(umax > 65504.f);
    };
    // two value pairs of the SECOND tile pair (q = 1) of an epilogue, for the scheduling region of k-step `idx` of the next
    // GEMM's first half (gemm_half_f16x2): pair pi = 2 idx + i -> point tile pi >> 4, accumulator register pi & 15
    auto split_chunk = [&](auto idx, const f32x16 (&v)[2][4], const float (&sa)[4], const float (&sb)[4], float &umax) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            constexpr int base = 2 * decltype(idx)::value;
            const int mt = (base + i) >> 4, r = (base + i) & 15;
            const float t0 = __builtin_fmaf(sa[2], v[mt][2][r], sb[2]);
            const float t1 = __builtin_fmaf(sa[3], v[mt][3][r], sb[3]);
            umax = __builtin_fmaxf(__builtin_fmaxf(umax, t0), t1);
            const float u0 = __builtin_amdgcn_fmed3f(t0, 0.f, 65504.f);
            const float u1 = __builtin_amdgcn_fmed3f(t1, 0.f, 65504.f);
            const f32x2 u = {u0, u1};
            const f16x2 h = __builtin_convertvector(u, f16x2);
            const f32x2 hf = __builtin_convertvector(h, f32x2);
            const f32x2 rr = {u0 - hf.x, u1 - hf.y};
            const f16x2 l = __builtin_convertvector(rr, f16x2);
            XW(mt, 1, r, 0) = __builtin_bit_cast(unsigned, h);
            XW(mt, 1, r, 1) = __builtin_bit_cast(unsigned, l);
        }
    };

    WStages ws;
    if constexpr (F16X2) gemm_prefetch_f16x2<KS_E>(ws, P.whf + (size_t)(4 * wave_u) * KS_E * 2 * 512, lane);

    TDECL(); int tphase_ = 0; (void)tphase_;
    for (int bi = 0; bi < B.n; ++bi) {
    const PtIO &io = B.io[bi];                       // kernel-argument segment: uniform loads
    const long npts = pt_count(io);
    const long ntiles = (npts + TP - 1) / TP;
    const float *tab_sample = P.tab + (size_t)B.sample[bi] * NCBN * 2 * H;
    const long tstep = io.shard_n > 1 ? io.shard_n : 1;       // grid-shard mode: this rank's tiles are shard_i, shard_i + shard_n, ...
    for (long tile = blockIdx.x * tstep + (io.shard_n > 1 ? io.shard_i : 0); tile < ntiles; tile += gridDim.x * tstep) {
        const long e0 = tile * TP;
        // re-materialise the arena bases per tile: keeps the compiler from hoisting ~100 derived
        // 64-bit layer addresses out of the tile loop and spilling them to scratch
        const float *wpack_ = P.wpack, *vecs_ = P.vecs, *tab_ = tab_sample;
        const _Float16 *whf = P.whf;
        // f16x2 gradient kernel: the thread index is made opaque per tile and the names below shadow the kernel-level ones, so
        // the dozen LDS addresses of the fetch / encode / output phases are formed where they are used instead of in the
        // prologue (from where they were carried through every GEMM in scratch).  No asm, no change for the other kernels.
        int tid_tile = threadIdx.x;
        if constexpr (GRAD && F16X2) asm volatile("" : "+v"(tid_tile));
        const int tid = tid_tile, lane = tid & 63, wave = tid >> 6, col = lane & 31;
        int cb = 128 * wave + col;          // first of this lane's four channels (+32 per tile)
        asm volatile("" : "+s"(wpack_), "+s"(vecs_), "+s"(tab_));
        if constexpr (F16X2) asm volatile("" : "+s"(whf), "+v"(cb), "+v"(xw0), "+v"(xw1));
        // (the asm erases the address space: restore "global" so loads stay global_load, not flat)
        const gfloat *wpack = (const gfloat *)wpack_, *vecs = (const gfloat *)vecs_, *tab = (const gfloat *)tab_;
        TPHASE(4);
        TBAR();   // previous tile's readers of PT/LOG/E2/DV are done
        // ---- 1. fetch points ------------------------------------------------------------
        if (tid < TP) {
            const long e = e0 + tid;
            float x = 0.f, y = 0.f, z = 0.f;
            int vox = -1;
            if (e < npts) {
                if (io.mode == PT_XYZ) {
                    x = io.xyz[e * 3 + 0]; y = io.xyz[e * 3 + 1]; z = io.xyz[e * 3 + 2];
                    vox = 0;
                } else if (io.mode == PT_EMB) {
                    vox = 0;
                } else {
                    vox = pt_voxel(io, e);
                    voxel_xyz(io, vox, x, y, z);
                }
            }
            PT[tid * 4 + 0] = x; PT[tid * 4 + 1] = y; PT[tid * 4 + 2] = z;
            PT[tid * 4 + 3] = __int_as_float(vox);
        }
        TPHASE(0);
        TBAR();
        // ---- 2. positional encoding into E[p][0..63] ---------------------------------------
        if constexpr (!F16X2) {
            const int p = tid >> 2, part = tid & 3;
            if (io.mode == PT_EMB) {
                const long e = e0 + p;
#pragma unroll 4
                for (int jj = 0; jj < 16; ++jj) {
                    const int j = part * 16 + jj;
                    E[p * ES + j] = (e < npts && j < io.emb_dim) ? io.xyz[e * io.emb_dim + j] : 0.f;
                }
            } else {
                const float c3[3] = {PT[p * 4 + 0], PT[p * 4 + 1], PT[p * 4 + 2]};
#pragma unroll 4
                for (int jj = 0; jj < 16; ++jj) {
                    const int j = part * 16 + jj;
                    float v;
                    if (j < 3) v = c3[j];
                    else if (j == 63) v = 0.f;
                    else {
                        const int f = (j - 3) / 6, r = (j - 3) % 6;
                        const float a = c3[r % 3] * (float)(1 << f);      // exact: power-of-two scale
                        v = (r < 3) ? sinf(a) : cosf(a);
                    }
                    E[p * ES + j] = v;
                }
            }
        } else {
            encode_tile_f16x2<4>(io, e0, npts, PT, X, tid, sat_flag);
        }
        if constexpr (F16X2) gemm_request_f16x2<KS_E>(ws, whf + (size_t)(4 * wave_u) * KS_E * 2 * 512, lane);
        TPHASE(0);
        TBAR();
        // ---- 3. fc_p -----------------------------------------------------------------------
        f32x16 net[2][4], tmp[2][4];
        unsigned msk[GRAD ? NCBN : 1][4];
        zero_acc(net);
        // scale/shift of the next conditional-BN layer: requested before the GEMM whose epilogue uses
        // them, so their L2 latency hides behind the MFMAs instead of opening every epilogue
        float nsa[4], nsb[4];
        // f16x2: accumulators carry SC * value; SC (a power of two) is folded back exactly into the
        // scale of the next conditional BN and into the biases
        const float wsc = F16X2 ? vecs[VOFF_SC] : 1.f, winv = F16X2 ? vecs[VOFF_SC + 1] : 1.f;
        auto scl = [](float v, float f) { if constexpr (F16X2) return v * f; else return v; };
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const std::conditional_t<F16X2, unsigned, int> c = F16X2 ? cb + 32 * nt : 32 * (4 * wave + nt) + col;
            nsa[nt] = scl(tab[c], winv); nsb[nt] = tab[H + c];
            if constexpr (F16X2) nsb[nt] = __builtin_fmaf(tab[c], vecs[voff_cb(0) + c], nsb[nt]);      // fc_p's bias, folded
        }
        if constexpr (F16X2) gemm_2x4_f16x2<KS_E, KS_H>(X, whf + (size_t)(4 * wave_u) * KS_E * 2 * 512,
                                                      whf + hf_off_fc(0, 0) + (size_t)(4 * wave_u) * KS_H * 2 * 512, ws, net, lane);
        else gemm_2x4<KG_E>(E, ES, wpack + OFF_FCP + (size_t)(4 * wave) * KG_E * 256, net, lane);
        if constexpr (!F16X2) {
            float bias[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) bias[nt] = vecs[VOFF_BFCP + 32 * (4 * wave + nt) + col];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) net[mt][nt][r] += bias[nt];
        }
        TPHASE(1);
        TBAR();   // E (aliasing X) fully consumed
        // ---- 4. residual blocks ---------------------------------------------------------------
        if constexpr (F16X2 && !GRAD && DEC_OVL) {
            // Forward kernel, overlapped form.  Per GEMM: the half of the preceding epilogue that produces the FIRST half of K
            // (tile pair q = 0 of every wave) is exposed; the GEMM then starts on that half while the other half of the epilogue
            // (q = 1: words [128, 256) of both planes, which nobody reads before the barrier in the middle of the GEMM) runs in
            // the MFMAs' shadow; the second half of K follows behind that barrier.  Hazards: an epilogue's q = 0 half rewrites
            // words [0, 128) — last read by the first half of the previous GEMM, which every wave left before the barrier in
            // that GEMM's middle; its q = 1 half rewrites words [128, 256) — last read by the previous GEMM's second half,
            // which every wave left before the barrier behind this epilogue's q = 0 half.  Four barriers per block, as before.
            const size_t woff = (size_t)(4 * wave_u) * KS_H * 2 * 512;
#pragma unroll 1
            for (int k = 0; k < NB; ++k) {
                const _Float16 *W0 = whf + (HF_FCP + (size_t)(2 * k) * HF_HH) + woff, *W1 = W0 + HF_HH;
                float sa[4], sb[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) { sa[nt] = nsa[nt]; sb[nt] = nsb[nt]; }
                store_split(net, sa, sb, nullptr, std::integral_constant<int, 1>{});
                gemm_request_f16x2<KS_H>(ws, W0, lane);
                TPHASE(2);
                TBAR();
                zero_acc(tmp);
                float sa1[4], sbb[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const unsigned c = cb + 32 * nt;
                    const float a = tab[(2 * k + 1) * 2 * H + c];
                    sa1[nt] = a * winv;
                    sbb[nt] = __builtin_fmaf(a, vecs[H * (1 + 2 * k) + c], tab[(2 * k + 1) * 2 * H + H + c]);      // a*(t/SC + bias0) + b
                }
                float um = 0.f;
                gemm_half_f16x2<0, true>(X, W0, ws, tmp, lane, [&](auto idx) { split_chunk(idx, net, sa, sb, um); });
                sat_flag |= __any(um > 65504.f);
                TPHASE(1);
                TBAR();
                gemm_half_f16x2<16, false>(X, W0, ws, tmp, lane, [](auto) {});
                store_split(tmp, sa1, sbb, nullptr, std::integral_constant<int, 1>{});
                gemm_request_f16x2<KS_H>(ws, W1, lane);
                TPHASE(2);
                TBAR();
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const unsigned c = cb + 32 * nt;
                    const float a = tab[(2 * k + 2) * 2 * H + c];                // next block's first CBN (or the final one)
                    nsa[nt] = a * winv;
                    nsb[nt] = __builtin_fmaf(a, vecs[voff_cb(0) + H * (k + 1) + c], tab[(2 * k + 2) * 2 * H + H + c]);   // biases so far, folded
                }
                um = 0.f;
                gemm_half_f16x2<0, true>(X, W1, ws, net, lane, [&](auto idx) { split_chunk(idx, tmp, sa1, sbb, um); });
                sat_flag |= __any(um > 65504.f);
                TPHASE(1);
                TBAR();
                gemm_half_f16x2<16, false>(X, W1, ws, net, lane, [](auto) {});
            }
            TPHASE(1);
            TBAR();        // every wave is done reading X before the final layer rewrites it
        } else {
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            // X <- relu(a*net + b), layer 2k
            {
                float sa[4], sb[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) { sa[nt] = nsa[nt]; sb[nt] = nsb[nt]; }
                if constexpr (GRAD) { msk[2 * k][0] = msk[2 * k][1] = msk[2 * k][2] = msk[2 * k][3] = 0u; }
                if constexpr (F16X2) {
                    unsigned *mk = nullptr;
                    if constexpr (GRAD) mk = msk[2 * k];
                    store_split(net, sa, sb, mk, std::integral_constant<int, 2>{});
                } else {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float u = sa[nt] * net[mt][nt][r] + sb[nt];
                            if constexpr (GRAD) if (u > 0.f) msk[2 * k][mword(mt, nt)] |= 1u << mbit(mt, nt, r);
                            XAT(mt, nt, r) = fmaxf(u, 0.f);
                        }
                }
            }
            if constexpr (F16X2) gemm_request_f16x2<KS_H>(ws, whf + hf_off_fc(k, 0) + (size_t)(4 * wave_u) * KS_H * 2 * 512, lane);
            TPHASE(2);
            TBAR();
            zero_acc(tmp);
            float sa1[4], sb1[4], bias0[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const std::conditional_t<F16X2, unsigned, int> c = F16X2 ? cb + 32 * nt : 32 * (4 * wave + nt) + col;
                sa1[nt] = scl(tab[(2 * k + 1) * 2 * H + c], winv);
                sb1[nt] = tab[(2 * k + 1) * 2 * H + H + c];
                bias0[nt] = scl(vecs[voff_bfc(k, 0) + c], wsc);
            }
            if constexpr (F16X2) gemm_2x4_f16x2<KS_H, KS_H>(X, whf + hf_off_fc(k, 0) + (size_t)(4 * wave_u) * KS_H * 2 * 512,
                                                          whf + hf_off_fc(k, 1) + (size_t)(4 * wave_u) * KS_H * 2 * 512, ws, tmp, lane);
            else gemm_2x4<KG_H>(X, XS, wpack + off_fc(k, 0) + (size_t)(4 * wave) * KG_H * 256, tmp, lane);
            TPHASE(1);
            TBAR();
            // X <- relu(a*(tmp + bias0) + b), layer 2k+1
            {
                float sa[4], sb[4], bias[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) { sa[nt] = sa1[nt]; sb[nt] = sb1[nt]; bias[nt] = bias0[nt]; }
                if constexpr (GRAD) { msk[2 * k + 1][0] = msk[2 * k + 1][1] = msk[2 * k + 1][2] = msk[2 * k + 1][3] = 0u; }
                if constexpr (F16X2) {
                    float sbb[4];      // a*(t + bias) + b = a*t + (a*bias + b)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) sbb[nt] = __builtin_fmaf(sa[nt], bias[nt], sb[nt]);
                    unsigned *mk = nullptr;
                    if constexpr (GRAD) mk = msk[2 * k + 1];
                    store_split(tmp, sa, sbb, mk, std::integral_constant<int, 2>{});
                } else {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float u = sa[nt] * (tmp[mt][nt][r] + bias[nt]) + sb[nt];
                            if constexpr (GRAD) if (u > 0.f) msk[2 * k + 1][mword(mt, nt)] |= 1u << mbit(mt, nt, r);
                            XAT(mt, nt, r) = fmaxf(u, 0.f);
                        }
                }
            }
            if constexpr (F16X2) gemm_request_f16x2<KS_H>(ws, whf + hf_off_fc(k, 1) + (size_t)(4 * wave_u) * KS_H * 2 * 512, lane);
            TPHASE(2);
            TBAR();
            // net += fc_1(X) + bias1   (residual accumulates straight into the MFMA C operand)
            float bias1[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const std::conditional_t<F16X2, unsigned, int> c = F16X2 ? cb + 32 * nt : 32 * (4 * wave + nt) + col;
                bias1[nt] = F16X2 ? 0.f : vecs[voff_bfc(k, 1) + c];
                nsa[nt] = scl(tab[(2 * k + 2) * 2 * H + c], winv);   // next block's first CBN (or the final one)
                nsb[nt] = tab[(2 * k + 2) * 2 * H + H + c];
                if constexpr (F16X2) nsb[nt] = __builtin_fmaf(tab[(2 * k + 2) * 2 * H + c], vecs[voff_cb(k + 1) + c], nsb[nt]);   // biases so far, folded
            }
            if constexpr (F16X2) {
                if (k + 1 < NB) gemm_2x4_f16x2<KS_H, KS_H>(X, whf + hf_off_fc(k, 1) + (size_t)(4 * wave_u) * KS_H * 2 * 512,
                                                           whf + hf_off_fc(k + 1 < NB ? k + 1 : 0, 0) + (size_t)(4 * wave_u) * KS_H * 2 * 512, ws, net, lane);
                else if constexpr (GRAD) gemm_2x4_f16x2<KS_H, KS_H>(X, whf + hf_off_fc(k, 1) + (size_t)(4 * wave_u) * KS_H * 2 * 512,
                                                whf + hf_off_fcT(NB - 1, 1) + (size_t)(4 * wave_u) * KS_H * 2 * 512, ws, net, lane);   // first matrix of the reverse sweep
                else gemm_2x4_f16x2<KS_H, KS_E>(X, whf + hf_off_fc(k, 1) + (size_t)(4 * wave_u) * KS_H * 2 * 512,
                                                whf + (size_t)(4 * wave_u) * KS_E * 2 * 512, ws, net, lane);     // next tile's fc_p
            }
            else gemm_2x4<KG_H>(X, XS, wpack + off_fc(k, 1) + (size_t)(4 * wave) * KG_H * 256, net, lane);
            if constexpr (!F16X2) {
                float bias[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) bias[nt] = bias1[nt];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) net[mt][nt][r] += bias[nt];
            }
            TPHASE(1);
            TBAR();
        }
        }      // (non-overlapped form)
        // ---- 5. final CBN + ReLU + fc_out (512 -> 1) -----------------------------------------
        float wo[4], a10[4];
        {
            float sb[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const std::conditional_t<F16X2, unsigned, int> c = F16X2 ? cb + 32 * nt : 32 * (4 * wave + nt) + col;
                a10[nt] = nsa[nt];
                sb[nt] = nsb[nt];
                wo[nt] = vecs[VOFF_WOUT + c];
            }
            fresh_xat_bases();
            unsigned mlast[4] = {0u, 0u, 0u, 0u};      // gates of the last layer, built in registers and stored once
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float u = a10[nt] * net[mt][nt][r] + sb[nt];
                        if constexpr (GRAD) mlast[mword(mt, nt)] |= u > 0.f ? 1u << mbit(mt, nt, r) : 0u;
                        XAT(mt, nt, r) = fmaxf(u, 0.f) * wo[nt];
                    }
            if constexpr (GRAD) { msk[2 * NB][0] = mlast[0]; msk[2 * NB][1] = mlast[1]; msk[2 * NB][2] = mlast[2]; msk[2 * NB][3] = mlast[3]; }
        }
        TPHASE(2);
        TBAR();
        {
            const float bo = vecs[VOFF_BOUT];
            for (int pp = 0; pp < TP / 4; ++pp) {
                const int p = wave * (TP / 4) + pp;
                float sacc = 0.f;
#pragma unroll
                for (int i = 0; i < H / 64; ++i) sacc += X[p * XS + lane + 64 * i];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) sacc += __shfl_xor(sacc, off);
                if (lane == 0) LOG[p] = sacc + bo;
            }
        }
        TBAR();

        TPHASE(4);
        if constexpr (!GRAD) {
            if (tid < TP) {          // exactly wave 0: all 64 lanes reach the aggregated append
                const long e = e0 + tid;
                const bool valid = e < npts;
                float udf = 0.f;
                int vox = 0;
                if (valid) {
                    const float o = LOG[tid];
                    const float y = 1.f / (1.f + expf(-o));
                    udf = (1.f - y) * 0.1f;
                    if (io.out_logit) io.out_logit[e] = o;
                    if (io.out_udf) io.out_udf[e] = udf;
                    if (io.grid_udf) {
                        vox = __float_as_int(PT[tid * 4 + 3]);
                        io.grid_udf[vox] = udf;
                    }
                }
                if (io.grid_udf && io.grad_list) {
                    const int slot = wave_append_slot(io.grad_count, valid && udf < io.grad_thr);
                    if (slot >= 0) io.grad_list[slot] = vox;
                }
            }
        }

        if constexpr (GRAD) {
            // ---- 6. reverse sweep: g = d logit / d net, kept in the accumulator layout ----------
            f32x16 (&g)[2][4] = net;   // net is dead from here on
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        g[mt][nt][r] = ((msk[2 * NB][mword(mt, nt)] >> mbit(mt, nt, r)) & 1u) ? scl(wo[nt] * a10[nt], wsc) : 0.f;   // a10 carries 1/SC in f16x2 mode
            if constexpr (F16X2) {
                // The adjoint has no natural range (unlike post-ReLU activations), so every operand tile is brought to
                // [2^14, 2^15) by ONE power of two per 64-point tile before it is split: rows are independent, the
                // factor is exact, the accumulators stay fp32, and it is divided out in the next epilogue.  The maximum
                // goes through LDS between the two barriers every GEMM needs anyway.
                auto lane_absmax = [&](const f32x16 (&v)[2][4]) {
                    float m = 0.f;
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                            for (int r = 0; r < 16; r += 2)
                                m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fabsf(v[mt][nt][r]), __builtin_fabsf(v[mt][nt][r + 1])));
                    return m;
                };
                // -> (s, 1/s); contains the barrier that also retires the previous GEMM's readers of X
                auto tile_scale = [&](float m, float &inv) {
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, off));
                    if (lane == 0) RED[wave] = m;
                    __syncthreads();
                    const float t = __builtin_fmaxf(__builtin_fmaxf(RED[0], RED[1]), __builtin_fmaxf(RED[2], RED[3]));
                    const int e = (int)(__float_as_uint(t) >> 23);                 // biased exponent of the tile maximum
                    const int se = (e == 0 || e == 255) ? 127 : min(max(268 - e, 4), 250);
                    inv = __uint_as_float((unsigned)(254 - se) << 23);
                    return __uint_as_float((unsigned)se << 23);
                };
                auto store_split_scaled = [&](const f32x16 (&v)[2][4], float s) {
#pragma unroll
                    for (int q = 0; q < 2; ++q)
#pragma unroll
                        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const f32x2 u = {v[mt][2 * q][r] * s, v[mt][2 * q + 1][r] * s};
                                unsigned hi, lo;
                                split2(u, hi, lo);
                                XW(mt, q, r, 0) = hi;
                                XW(mt, q, r, 1) = lo;
                            }
                };
#pragma unroll
                for (int k = NB - 1; k >= 0; --k) {
                    float inv_s;
                    const float s1 = tile_scale(lane_absmax(g), inv_s);
                    store_split_scaled(g, s1);                                       // X <- g
                    float f1[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) f1[nt] = tab[(2 * k + 1) * 2 * H + cb + 32 * nt] * (winv * inv_s);
                    gemm_request_f16x2<KS_H>(ws, whf + hf_off_fcT(k, 1) + (size_t)(4 * wave_u) * KS_H * 2 * 512, lane);
                    __syncthreads();
                    zero_acc(tmp);
                    gemm_2x4_f16x2<KS_H, KS_H>(X, whf + hf_off_fcT(k, 1) + (size_t)(4 * wave_u) * KS_H * 2 * 512,
                                               whf + hf_off_fcT(k, 0) + (size_t)(4 * wave_u) * KS_H * 2 * 512, ws, tmp, lane);   // t = fc_1^T g
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const bool on = (msk[2 * k + 1][mword(mt, nt)] >> mbit(mt, nt, r)) & 1u;
                                tmp[mt][nt][r] = on ? tmp[mt][nt][r] * f1[nt] : 0.f;
                            }
                    const float s0 = tile_scale(lane_absmax(tmp), inv_s);
                    store_split_scaled(tmp, s0);
                    float f0[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) f0[nt] = tab[(2 * k) * 2 * H + cb + 32 * nt] * (winv * inv_s);
                    gemm_request_f16x2<KS_H>(ws, whf + hf_off_fcT(k, 0) + (size_t)(4 * wave_u) * KS_H * 2 * 512, lane);
                    __syncthreads();
                    zero_acc(tmp);
                    if (k > 0) gemm_2x4_f16x2<KS_H, KS_H>(X, whf + hf_off_fcT(k, 0) + (size_t)(4 * wave_u) * KS_H * 2 * 512,
                                                          whf + hf_off_fcT(k > 0 ? k - 1 : 0, 1) + (size_t)(4 * wave_u) * KS_H * 2 * 512, ws, tmp, lane);   // fc_0^T t
                    else gemm_2x4_f16x2<KS_H, KS_E>(X, whf + hf_off_fcT(k, 0) + (size_t)(4 * wave_u) * KS_H * 2 * 512,
                                                    whf + (size_t)(4 * wave_u) * KS_E * 2 * 512, ws, tmp, lane);                 // then the next tile's fc_p
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const bool on = (msk[2 * k][mword(mt, nt)] >> mbit(mt, nt, r)) & 1u;
                                g[mt][nt][r] += on ? tmp[mt][nt][r] * f0[nt] : 0.f;
                            }
                }
                __syncthreads();       // the last GEMM's readers of X are done
            } else {
#pragma unroll
            for (int k = NB - 1; k >= 0; --k) {
                // X <- g
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            XAT(mt, nt, r) = g[mt][nt][r];
                __syncthreads();
                zero_acc(tmp);
                gemm_2x4<KG_H>(X, XS, wpack + off_fcT(k, 1) + (size_t)(4 * wave) * KG_H * 256, tmp, lane);   // t = fc_1^T g
                __syncthreads();
                {
                    float sa[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) sa[nt] = tab[(2 * k + 1) * 2 * H + 32 * (4 * wave + nt) + col];
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const bool on = (msk[2 * k + 1][mword(mt, nt)] >> mbit(mt, nt, r)) & 1u;
                                XAT(mt, nt, r) = on ? tmp[mt][nt][r] * sa[nt] : 0.f;
                            }
                }
                __syncthreads();
                zero_acc(tmp);
                gemm_2x4<KG_H>(X, XS, wpack + off_fcT(k, 0) + (size_t)(4 * wave) * KG_H * 256, tmp, lane);   // fc_0^T t
                {
                    float sa[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) sa[nt] = tab[(2 * k) * 2 * H + 32 * (4 * wave + nt) + col];
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const bool on = (msk[2 * k][mword(mt, nt)] >> mbit(mt, nt, r)) & 1u;
                                g[mt][nt][r] += on ? tmp[mt][nt][r] * sa[nt] : 0.f;
                            }
                }
                __syncthreads();
            }
            }
            // X <- g ; e2 = fc_p^T g  (64 x 64)
            fresh_xat_bases();
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        XAT(mt, nt, r) = g[mt][nt][r];
            __syncthreads();
            {
                f32x16 ea;
#pragma unroll
                for (int r = 0; r < 16; ++r) ea[r] = 0.f;
                const int mt = wave & 1, et = wave >> 1;
                gemm_1x1<KG_H>(X, XS, mt, wpack + OFF_FCPT + (size_t)et * KG_H * 256, ea, lane);
#pragma unroll
                for (int r = 0; r < 16; ++r) E2[(32 * mt + frag_row(r, lane)) * ES + 32 * et + col] = ea[r];
            }
            __syncthreads();
            if (tid < TP * 3) {
                const int p = tid / 3, c = tid % 3;
                const float xc = PT[p * 4 + c];
                float d = E2[p * ES + c];
#pragma unroll
                for (int j = 0; j < 10; ++j) {
                    const float f = (float)(1 << j);
                    float sn, cs;
                    sincosf(xc * f, &sn, &cs);
                    d += f * (cs * E2[p * ES + 3 + 6 * j + c] - sn * E2[p * ES + 6 + 6 * j + c]);
                }
                DV[p * 4 + c] = d;
            }
            __syncthreads();
            if (tid < TP) {
                const long e = e0 + tid;
                if (e < npts) {
                    const float o = LOG[tid];
                    const float y = 1.f / (1.f + expf(-o));
                    const float udf = (1.f - y) * 0.1f;
                    const float sfac = -0.1f * ((1.f - y) * y);   // d udf / d logit as torch's sigmoid backward forms it
                    const float gx = sfac * DV[tid * 4 + 0], gy = sfac * DV[tid * 4 + 1], gz = sfac * DV[tid * 4 + 2];
                    const float nrm = fmaxf(sqrtf(gx * gx + gy * gy + gz * gz), 1e-12f);
                    const float ox = -(gx / nrm), oy = -(gy / nrm), oz = -(gz / nrm);
                    if (io.out_logit) io.out_logit[e] = o;
                    if (io.out_udf) io.out_udf[e] = udf;
                    if (io.out_dlogit) { io.out_dlogit[e * 3 + 0] = DV[tid * 4 + 0]; io.out_dlogit[e * 3 + 1] = DV[tid * 4 + 1]; io.out_dlogit[e * 3 + 2] = DV[tid * 4 + 2]; }
                    if (io.out_ngrad) { io.out_ngrad[e * 3 + 0] = ox; io.out_ngrad[e * 3 + 1] = oy; io.out_ngrad[e * 3 + 2] = oz; }
                    if (io.grid_grads) {
                        const long vox = __float_as_int(PT[tid * 4 + 3]);
                        io.grid_grads[vox * 3 + 0] = ox; io.grid_grads[vox * 3 + 1] = oy; io.grid_grads[vox * 3 + 2] = oz;
                    }
                }
            }
        }
    }
    }
    if constexpr (F16X2) {
        if (sat_flag && lane == 0) atomicAdd(P.sat, 1u);
    }
    TFLUSH();
}

#undef XAT

// =============================================================================================================================
// Forward kernel, 8-wave form (f16x2): 512 threads = TWO waves per SIMD on the same 64-point x 512-channel tile.
// Wave w owns channels [64 w, 64 w + 64): 2 (point tiles) x 2 (channel tiles) accumulators for the residual stream and as
// many for the block intermediate (128 of its 256 registers), 4 weight stages of 2 x 2 fragments, the same X rows in LDS
// (a wave's tile pair is one 32-bit word column: word 32 w + col of both planes — the k-slot order of the 4-wave kernels is
// exactly this order, so the packed weights are shared).  Why: with one wave per SIMD nothing hides behind anything — every
// load or LDS read issued between two MFMAs idles the matrix pipe for ~6 cycles (9 % of every GEMM), and an epilogue is a
// single dependent instruction stream at ~8 cycles per instruction (22 % of a tile; profiles/r03_decoder_variants.md).  With
// two waves per SIMD the partner's MFMAs fill the issue bubbles of a GEMM and the two epilogue streams interleave.  No
// weight byte is fetched twice (the eight waves partition the 512 output channels); each wave reads all of X, so the LDS
// read traffic doubles (32 KB per k-step pair: 42 B/clk/CU of the 256 the LDS delivers).
// =============================================================================================================================
struct WStages8 { f16x8 b[4][2][2]; };        // 4 stages x 2 channel tiles x 2 planes (64 registers)

template <int KS>
__device__ __forceinline__ void load_wstage8(f16x8 (&dst)[2][2], const _Float16 *Whf, unsigned lofs, int ks) {
    const unsigned long long wa = (unsigned long long)Whf;
    unsigned wlo = __builtin_amdgcn_readfirstlane((unsigned)wa), whi = __builtin_amdgcn_readfirstlane((unsigned)(wa >> 32));
    asm volatile("" : "+s"(wlo), "+s"(whi));
    const __attribute__((address_space(1))) char *wb = (const __attribute__((address_space(1))) char *)(((unsigned long long)whi << 32) | wlo);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#if defined(SURFD_DEC_W_NT) && SURFD_DEC_W_NT        // experiment: weight planes with the non-temporal policy
            dst[nt][q] = __builtin_nontemporal_load(reinterpret_cast<const gf16x8 *>(wb + (size_t)(nt * KS * 2048) + (lofs + (unsigned)((ks * 2 + q) * 1024))));
#else
            dst[nt][q] = *reinterpret_cast<const gf16x8 *>(wb + (size_t)(nt * KS * 2048) + (lofs + (unsigned)((ks * 2 + q) * 1024)));
#endif
}

__device__ __forceinline__ void mfma_step8(const f16x8 (&a)[2][2], const f16x8 (&b)[2][2], f32x16 (&acc)[2][2]) {
    constexpr int TA[3] = {1, 0, 0};     // activation plane
    constexpr int TB[3] = {0, 1, 0};     // weight plane (small terms first)
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mt][TA[t]], b[nt][TB[t]], acc[mt][nt], 0, 0, 0);
}

// stage 0 of a matrix, requested by the caller before the barrier in front of the GEMM (as gemm_request_f16x2)
template <int KS>
__device__ __forceinline__ void gemm8_request(WStages8 &ws, const _Float16 *Whf, int lane) {
    __builtin_amdgcn_sched_barrier(0);
    unsigned lofs = (unsigned)lane * 16u;
    asm volatile("" : "+v"(lofs));
    load_wstage8<KS>(ws.b[0], Whf, lofs, 0);
    __builtin_amdgcn_sched_barrier(0);
}

// acc[mt][nt] += A[64 x 16 KS] (split fp16 planes in LDS) * W (2 channel tiles of this wave); 12 MFMAs per k-step
template <int KS>
__device__ __forceinline__ void gemm8(const float *A, const _Float16 *Whf, WStages8 &ws, f32x16 (&acc)[2][2], int lane) {
    constexpr int D = 4;
    static_assert(KS % D == 0, "k-step count must be a multiple of the pipeline depth");
    const float *a0 = A + (lane & 31) * XS + 4 * (lane >> 5);
    const float *a1 = a0 + 32 * XS;
    unsigned lofs = (unsigned)lane * 16u;
    asm volatile("" : "+v"(lofs));
    f16x8 x[2][2][2];
    auto group = [&](int ks0, auto last) {
        int goff = ks0 * 8;
        asm volatile("" : "+v"(goff));
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (!decltype(last)::value || j == 0) load_wstage8<KS>(ws.b[(j + D - 1) % D], Whf, lofs, ks0 + j + D - 1);
            const int jn = (decltype(last)::value && j == D - 1) ? j : j + 1;
            x[(j + 1) & 1][0][0] = *reinterpret_cast<const f16x8 *>(a0 + goff + jn * 8); x[(j + 1) & 1][0][1] = *reinterpret_cast<const f16x8 *>(a0 + goff + 256 + jn * 8);
            x[(j + 1) & 1][1][0] = *reinterpret_cast<const f16x8 *>(a1 + goff + jn * 8); x[(j + 1) & 1][1][1] = *reinterpret_cast<const f16x8 *>(a1 + goff + 256 + jn * 8);
            mfma_step8(x[j & 1], ws.b[j], acc);
#pragma unroll
            for (int i = 0; i < 4; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); }
#pragma unroll
            for (int i = 0; i < 4; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    x[0][0][0] = *reinterpret_cast<const f16x8 *>(a0); x[0][0][1] = *reinterpret_cast<const f16x8 *>(a0 + 256);
    x[0][1][0] = *reinterpret_cast<const f16x8 *>(a1); x[0][1][1] = *reinterpret_cast<const f16x8 *>(a1 + 256);
    if constexpr (KS > D) {
#pragma unroll
        for (int d = 1; d < D - 1; ++d) load_wstage8<KS>(ws.b[d], Whf, lofs, d);
#pragma unroll 1
        for (int ks0 = 0; ks0 < KS - D; ks0 += D) group(ks0, std::false_type{});
        group(KS - D, std::true_type{});
    } else {
        // the 4-step first layer: all of its stages at once (stage 0 came early), then one group without further requests
#pragma unroll
        for (int d = 1; d < D; ++d) load_wstage8<KS>(ws.b[d], Whf, lofs, d);
        int goff = 0;
        asm volatile("" : "+v"(goff));
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int jn = j == D - 1 ? j : j + 1;
            x[(j + 1) & 1][0][0] = *reinterpret_cast<const f16x8 *>(a0 + goff + jn * 8); x[(j + 1) & 1][0][1] = *reinterpret_cast<const f16x8 *>(a0 + goff + 256 + jn * 8);
            x[(j + 1) & 1][1][0] = *reinterpret_cast<const f16x8 *>(a1 + goff + jn * 8); x[(j + 1) & 1][1][1] = *reinterpret_cast<const f16x8 *>(a1 + goff + 256 + jn * 8);
            mfma_step8(x[j & 1], ws.b[j], acc);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

__global__ __launch_bounds__(512, 1) void decoder_fwd8_kernel(DecParams P, PtBatch B) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *X = lds;                      // [TP][XS]
    float *PT = lds + TP * XS;           // [TP][4]
    float *LOG = PT + TP * 4;            // [TP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;          // wave 0..7
    const int col = lane & 31;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    float *const xb0 = X + (4 * (lane >> 5)) * XS + 64 * wave + col;        // fp32 view (final layer)
    float *const xb1 = xb0 + 32 * XS;
#define XAT8(mt, nt, r) ((mt) ? xb1 : xb0)[(((r) & 3) + 8 * ((r) >> 2)) * XS + 32 * (nt)]
    typedef unsigned __attribute__((address_space(3))) lds_u32;
    lds_u32 *xw0 = (lds_u32 *)(reinterpret_cast<unsigned *>(X) + (4 * (lane >> 5)) * XS + 32 * wave + col);
    lds_u32 *xw1 = xw0 + 32 * XS;
#define XW8(mt, r, pl) ((mt) ? xw1 : xw0)[(((r) & 3) + 8 * ((r) >> 2)) * XS + 256 * (pl)]
    // Sustained shader clock of this launch: the kernel is power-bound, its rate follows the clock the chip can
    // hold under it.  Workgroup 0 (persistent: it runs from the first tile to the last) notes the shader-cycle counter and the
    // 100 MHz real-time counter now and adds the differences to the handle's record when it leaves; the start values wait in
    // the workgroup's OWN LDS (behind LOG: the forward kernel uses nothing there), not in registers (the kernel sits at its
    // 256-register / SGPR limit) and not in the handle's record (round 5: two launches on one handle that overlap — batch-grid
    // pipelines, several streams — overwrote each other's start values there and added wrapped differences).
    // Experiment (-DSURFD_DEC_XCD_STAGGER=k, default off): the workgroups of XCD x (block b runs on XCD b % 8)
    // start x * k sleeps of ~4.8 us late, so that the eight XCDs walk the 11 layers out of phase (k = 6: an eighth of a tile's
    // ~215 us per XCD) instead of fetching the same 1 MB of a layer's planes from the fabric at the same moment.
#ifndef SURFD_DEC_XCD_STAGGER
#define SURFD_DEC_XCD_STAGGER 0
#endif
#if SURFD_DEC_XCD_STAGGER > 0
    for (int k_ = 0; k_ < (int)(blockIdx.x & 7) * SURFD_DEC_XCD_STAGGER; ++k_) __builtin_amdgcn_s_sleep(127);
#endif
#ifndef SURFD_DEC_CLOCK
#define SURFD_DEC_CLOCK 1
#endif
#if SURFD_DEC_CLOCK
    unsigned long long *const clk = reinterpret_cast<unsigned long long *>(P.sat + 2);
    unsigned long long *const clk0 = reinterpret_cast<unsigned long long *>(LOG + TP);       // 8-byte aligned: (TP * XS + TP * 4 + TP) floats
    if (blockIdx.x == 0 && tid == 0) {
        clk0[0] = (unsigned long long)__builtin_readcyclecounter();
        clk0[1] = (unsigned long long)__builtin_amdgcn_s_memrealtime();
    }
#endif
    int sat_flag = 0;
    // X <- split(min(relu(a*v + b), 65504)) for this wave's 64 channels x 64 points
    auto store8 = [&](const f32x16 (&v)[2][2], const float (&sa)[2], const float (&sb)[2]) {
        float umax = 0.f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float t0 = __builtin_fmaf(sa[0], v[mt][0][r], sb[0]);
                const float t1 = __builtin_fmaf(sa[1], v[mt][1][r], sb[1]);
                umax = __builtin_fmaxf(__builtin_fmaxf(umax, t0), t1);
                const float u0 = __builtin_amdgcn_fmed3f(t0, 0.f, 65504.f);
                const float u1 = __builtin_amdgcn_fmed3f(t1, 0.f, 65504.f);
                const f32x2 u = {u0, u1};
                const unsigned h = __builtin_bit_cast(unsigned, __builtin_convertvector(u, f16x2));
                XW8(mt, r, 0) = h;
                XW8(mt, r, 1) = split_low_pair(h, u0, u1);
            }
        sat_flag |= __any(umax > 65504.f);
    };
    auto zero8 = [](f32x16 (&a)[2][2]) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) a[mt][nt][r] = 0.f;
    };
    WStages8 ws;
    for (int bi = 0; bi < B.n; ++bi) {
    const PtIO &io = B.io[bi];
    const long npts = pt_count(io);
    const long ntiles = (npts + TP - 1) / TP;
    const float *tab_sample = P.tab + (size_t)B.sample[bi] * NCBN * 2 * H;
    const long tstep = io.shard_n > 1 ? io.shard_n : 1;       // grid-shard mode: this rank's tiles are shard_i, shard_i + shard_n, ...
    for (long tile = blockIdx.x * tstep + (io.shard_n > 1 ? io.shard_i : 0); tile < ntiles; tile += gridDim.x * tstep) {
        const long e0 = tile * TP;
        const float *vecs_ = P.vecs, *tab_ = tab_sample;
        const _Float16 *whf = P.whf;
        unsigned cb = 64 * wave + col;              // first of this lane's two channels (+32 for the second tile)
        asm volatile("" : "+s"(vecs_), "+s"(tab_), "+s"(whf), "+v"(cb), "+v"(xw0), "+v"(xw1));
        const gfloat *vecs = (const gfloat *)vecs_, *tab = (const gfloat *)tab_;
        const size_t woff_e = (size_t)(2 * wave_u) * KS_E * 2 * 512, woff = (size_t)(2 * wave_u) * KS_H * 2 * 512;
        __syncthreads();        // previous tile's readers of PT / LOG are done
        {   // fetch + encode with the thread index opaque: their LDS addresses are formed here, not carried from the prologue in scratch
        int tid_fe = threadIdx.x;
        asm volatile("" : "+v"(tid_fe));
        const int tid = tid_fe;
        // ---- 1. fetch points ------------------------------------------------------------------
        if (tid < TP) {
            const long e = e0 + tid;
            float x = 0.f, y = 0.f, z = 0.f;
            int vox = -1;
            if (e < npts) {
                if (io.mode == PT_XYZ) { x = io.xyz[e * 3 + 0]; y = io.xyz[e * 3 + 1]; z = io.xyz[e * 3 + 2]; vox = 0; }
                else if (io.mode == PT_EMB) vox = 0;
                else { vox = pt_voxel(io, e); voxel_xyz(io, vox, x, y, z); }
            }
            PT[tid * 4 + 0] = x; PT[tid * 4 + 1] = y; PT[tid * 4 + 2] = z;
            PT[tid * 4 + 3] = __int_as_float(vox);
        }
        __syncthreads();
        // ---- 2. positional encoding, split planes in X's row layout (identity k-slot order): 8 threads per point ------
        encode_tile_f16x2<8>(io, e0, npts, PT, X, tid, sat_flag);
        }
        gemm8_request<KS_E>(ws, whf + woff_e, lane);
        __syncthreads();
        // ---- 3. fc_p ---------------------------------------------------------------------------
        f32x16 net[2][2], tmp[2][2];
        zero8(net);
        const float winv = vecs[VOFF_SC + 1];
        float nsa[2], nsb[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const unsigned c = cb + 32 * nt;
            const float a = tab[c];
            nsa[nt] = a * winv;
            nsb[nt] = __builtin_fmaf(a, vecs[voff_cb(0) + c], tab[H + c]);        // fc_p's bias, folded
        }
        gemm8<KS_E>(X, whf + woff_e, ws, net, lane);
        __syncthreads();        // the encoding (aliasing X) is fully consumed
        // ---- 4. residual blocks ------------------------------------------------------------------
#pragma unroll 1
        for (int k = 0; k < NB; ++k) {
            const _Float16 *W0 = whf + (HF_FCP + (size_t)(2 * k) * HF_HH) + woff, *W1 = W0 + HF_HH;
            {
                float sa[2] = {nsa[0], nsa[1]}, sb[2] = {nsb[0], nsb[1]};
                store8(net, sa, sb);                                            // X <- relu(a*net + b), layer 2k
            }
            gemm8_request<KS_H>(ws, W0, lane);
            __syncthreads();
            zero8(tmp);       // (clearing it inside the preceding GEMM instead does not survive the optimiser: both values reaching the loop head are the constant)
            float sa1[2], sbb[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const unsigned c = cb + 32 * nt;
                const float a = tab[(2 * k + 1) * 2 * H + c];
                sa1[nt] = a * winv;
                sbb[nt] = __builtin_fmaf(a, vecs[H * (1 + 2 * k) + c], tab[(2 * k + 1) * 2 * H + H + c]);      // a*(t/SC + bias0) + b
            }
            gemm8<KS_H>(X, W0, ws, tmp, lane);
            __syncthreads();
            store8(tmp, sa1, sbb);                                              // layer 2k+1
            gemm8_request<KS_H>(ws, W1, lane);
            __syncthreads();
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const unsigned c = cb + 32 * nt;
                const float a = tab[(2 * k + 2) * 2 * H + c];                     // next block's first CBN (or the final one)
                nsa[nt] = a * winv;
                nsb[nt] = __builtin_fmaf(a, vecs[voff_cb(0) + H * (k + 1) + c], tab[(2 * k + 2) * 2 * H + H + c]);
            }
            gemm8<KS_H>(X, W1, ws, net, lane);                                    // net += fc_1(X)
            __syncthreads();
        }
        // ---- 5. final CBN + ReLU + fc_out (512 -> 1) -------------------------------------------------
        {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const float wo = vecs[VOFF_WOUT + cb + 32 * nt];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float u = nsa[nt] * net[mt][nt][r] + nsb[nt];
                        XAT8(mt, nt, r) = fmaxf(u, 0.f) * wo;
                    }
            }
        }
        __syncthreads();
        {
            const float bo = vecs[VOFF_BOUT];
            for (int pp = 0; pp < TP / 8; ++pp) {
                const int p = wave * (TP / 8) + pp;
                float sacc = 0.f;
#pragma unroll
                for (int i = 0; i < H / 64; ++i) sacc += X[p * XS + lane + 64 * i];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) sacc += __shfl_xor(sacc, off);
                if (lane == 0) LOG[p] = sacc + bo;
            }
        }
        __syncthreads();
        if (tid < TP) {          // exactly wave 0: all 64 lanes reach the aggregated append
            const long e = e0 + tid;
            const bool valid = e < npts;
            float udf = 0.f;
            int vox = 0;
            if (valid) {
                const float o = LOG[tid];
                const float y = 1.f / (1.f + expf(-o));
                udf = (1.f - y) * 0.1f;
                if (io.out_logit) io.out_logit[e] = o;
                if (io.out_udf) io.out_udf[e] = udf;
                if (io.grid_udf) {
                    vox = __float_as_int(PT[tid * 4 + 3]);
                    io.grid_udf[vox] = udf;
                }
            }
            if (io.grid_udf && io.grad_list) {
                const int slot = wave_append_slot(io.grad_count, valid && udf < io.grad_thr);
                if (slot >= 0) io.grad_list[slot] = vox;
            }
        }
    }
    }
    if (sat_flag && lane == 0) atomicAdd(P.sat, 1u);
#if SURFD_DEC_CLOCK
    if (blockIdx.x == 0 && tid == 0) {
        const unsigned long long c1 = (unsigned long long)__builtin_readcyclecounter(), r1 = (unsigned long long)__builtin_amdgcn_s_memrealtime();
        atomicAdd(clk + 2, c1 - clk0[0]);        // same thread wrote them: program order, no barrier
        atomicAdd(clk + 3, r1 - clk0[1]);
    }
#endif
}
#undef XAT8
#undef XW8

#undef XW
constexpr size_t DEC_LDS_BYTES = (size_t)(TP * XS + TP * 4 + TP + TP * ES + TP * 4 + 4) * sizeof(float);

// ---------------------------------------------------------------------------------------------
// per-sample conditional-BN tables
// ---------------------------------------------------------------------------------------------
// max |w| over a float range, as the bit pattern of a non-negative float (monotone as unsigned)
__global__ void absmax_kernel(const float *src, size_t n, unsigned *out) {
    unsigned m = 0u;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        m = max(m, __float_as_uint(src[i]) & 0x7fffffffu);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// SC = 2^(8 - floor(log2 max|W|)): max |W| * SC in [256, 512); sc[0] = SC, sc[1] = 1/SC
__global__ void weight_scale_kernel(const unsigned *maxbits, float *sc) {
    const unsigned b = *maxbits;
    int e = (int)(b >> 23) - 127;
    if (b == 0u || e > 100 || e < -100) e = 8;         // degenerate weights: SC = 1
    sc[0] = __uint_as_float((unsigned)(127 + 8 - e) << 23);
    sc[1] = __uint_as_float((unsigned)(127 - 8 + e) << 23);
}

// fragment-major fp32 pack (PackDesc layout, KG k-groups per tile) -> two fragment-major fp16 planes of SC*W
// (layout comment at the top); `permute` selects the hidden-layer k-slot order
__global__ void pack_f16x2_kernel(const float *wp, int KG, int KS, int permute, const float *sc, _Float16 *dst) {
    const float scale = sc[0];
    const long total = (long)16 * KS * 64 * 8;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int el = e & 7, lane = (e >> 3) & 63;
        const long tk = e >> 9;
        const int ks = tk % KS, tile = tk / KS;
        const int slot = ks * 16 + 8 * (lane >> 5) + el;
        const int k = permute ? slot_channel(slot) : slot;
        const float x = wp[((size_t)(tile * KG + (k >> 3)) * 64 + (lane & 31) + 32 * ((k >> 2) & 1)) * 4 + (k & 3)] * scale;
        const _Float16 h = (_Float16)x;
        const _Float16 l = (_Float16)(x - (float)h);
        const size_t base = ((size_t)(tile * KS + ks) * 2) * 512 + (size_t)lane * 8 + el;
        dst[base] = h; dst[base + 512] = l;
    }
}

// CB[k][c] = b_fc_p[c] + sum_{j<k} b_fc_1[j][c], k = 0..NB
__global__ void cumbias_kernel(float *vecs) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= H) return;
    float acc = vecs[VOFF_BFCP + c];
    vecs[voff_cb(0) + c] = acc;
    for (int k = 0; k < NB; ++k) { acc += vecs[voff_bfc(k, 1) + c]; vecs[voff_cb(k + 1) + c] = acc; }
}

struct CbnParams {
    const float *gw[NCBN], *gb[NCBN], *bw[NCBN], *bb[NCBN], *mean[NCBN], *var[NCBN];
};

__global__ void cbn_table_kernel(CbnParams P, const float *lat, int S, int D, float *tab) {
    const int total = S * NCBN * H;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int c = e % H, l = (e / H) % NCBN, s = e / (H * NCBN);
        float gamma = 0.f, beta = 0.f;
        for (int d = 0; d < D; ++d) {
            const float z = lat[s * D + d];
            gamma += P.gw[l][c * D + d] * z;
            beta += P.bw[l][c * D + d] * z;
        }
        gamma += P.gb[l][c];
        beta += P.bb[l][c];
        const float a = gamma / sqrtf(P.var[l][c] + 1e-5f);
        tab[((size_t)(s * NCBN + l) * 2 + 0) * H + c] = a;
        tab[((size_t)(s * NCBN + l) * 2 + 1) * H + c] = beta - a * P.mean[l][c];
    }
}

}  // namespace surfd

// =============================================================================================
// host side
// =============================================================================================
// the compiled configuration of this file (surfd_build_config); SURFD_DEC_OVL is the one variant recorded as not to be shipped
// (25 spilled registers, kept as the record of a measurement): fenced like conv_f16x2.hip's
#define DEC_STR_(x) #x
#define DEC_STR(x) DEC_STR_(x)
#if defined(SURFD_DEC_W_NT) && SURFD_DEC_W_NT
#define DEC_CFG_W_NT 1
#else
#define DEC_CFG_W_NT 0
#endif
#if defined(SURFD_DEC_STAMPS)
#define DEC_CFG_STAMPS 1
#else
#define DEC_CFG_STAMPS 0
#endif
#if SURFD_DEC_OVL != 0 && !defined(SURFD_ALLOW_UNSAFE_VARIANTS)
#error "SURFD_DEC_OVL=1 is an experiment kept as a record (profiles/r03_decoder_variants.md); -DSURFD_ALLOW_UNSAFE_VARIANTS builds it anyway"
#endif
namespace surfd {
const char *decoder_build_config() {
    return "DEC_OVL=" DEC_STR(SURFD_DEC_OVL) " DEC_MIX=" DEC_STR(SURFD_DEC_MIX) " DEC_GRAD_W=" DEC_STR(SURFD_DEC_GRAD_W) " DEC_GRAD_MIX=" DEC_STR(SURFD_DEC_GRAD_MIX)
           " DEC_WS_AHEAD=" DEC_STR(SURFD_DEC_WS_AHEAD) " DEC_REQ_EARLY=" DEC_STR(SURFD_DEC_REQ_EARLY) " DEC_FWD_STAGED=" DEC_STR(SURFD_DEC_FWD_STAGED)
           " DEC_XCD_STAGGER=" DEC_STR(SURFD_DEC_XCD_STAGGER) " DEC_CLOCK=" DEC_STR(SURFD_DEC_CLOCK) " DEC_W_NT=" DEC_STR(DEC_CFG_W_NT) " DEC_STAMPS=" DEC_STR(DEC_CFG_STAMPS);
}
int decoder_build_unsafe() { return SURFD_DEC_OVL != 0; }
}  // namespace surfd

using namespace surfd;

struct surfd_decoder {
    int input_dim = 63, D = 32, hidden = 512, nb = 5, device = -1;
    ParamTable params;                // CbnDecoder.state_dict()
    bool allocated = false, finalized = false;
    // private device copies
    float *wpack = nullptr, *vecs = nullptr;
    _Float16 *whf = nullptr;          // f16x2 planes of the forward matrices (built by finalize)
    int precision = 1;                // forward kernel: 1 = f16x2 (default), 0 = exact fp32 MFMA
    int fwd8 = 1;                     // f16x2 forward kernel in its 8-wave form (two waves per SIMD: 453 against 438 TFLOP/s); SURFD_DECODER_FWD8=0 selects the 4-wave kernel
    float *gw[NCBN] = {}, *gb[NCBN] = {}, *bw[NCBN] = {}, *bb[NCBN] = {}, *mean[NCBN] = {}, *var[NCBN] = {};
    float *tab = nullptr;
    int S = 0, tab_cap = 0;
    int num_cus = 256;
    int grid_blocks = 0;              // persistent workgroups per launch; 0 = one per CU
    unsigned *sat = nullptr;          // device counter: waves of the f16x2 kernel that clamped an activation
    std::vector<void *> allocs;
};

static void dec_add(surfd_decoder *d, const std::string &k, std::initializer_list<int64_t> shape) { d->params.add(k, shape); }

static void dec_add_cbn(surfd_decoder *d, const std::string &p) {
    const int64_t Hh = d->hidden, D = d->D;
    dec_add(d, p + ".conv_gamma.weight", {Hh, D, 1}); dec_add(d, p + ".conv_gamma.bias", {Hh});
    dec_add(d, p + ".conv_beta.weight", {Hh, D, 1});  dec_add(d, p + ".conv_beta.bias", {Hh});
    dec_add(d, p + ".bn.running_mean", {Hh});         dec_add(d, p + ".bn.running_var", {Hh});
    d->params.add(p + ".bn.num_batches_tracked", {}, 0, true);
}

static int dec_alloc(surfd_decoder *d) {
    if (d->allocated) return SURFD_OK;
    HIP_TRY(hipGetDevice(&d->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, d->device));
    d->num_cus = prop.multiProcessorCount;
    auto A = [&](float **p, size_t n) -> int {
        HIP_TRY(hipMalloc((void **)p, n * sizeof(float)));
        d->allocs.push_back(*p);
        return SURFD_OK;
    };
    int rc;
    if ((rc = A(&d->wpack, WPACK_FLOATS))) return rc;
    if ((rc = A(&d->vecs, VEC_FLOATS))) return rc;
    HIP_TRY(hipMalloc((void **)&d->whf, WHF_ELEMS * sizeof(_Float16)));
    d->allocs.push_back(d->whf);
    // [0]: saturation counter; 8 bytes in: the clock record of the 8-wave forward kernel {start cycles, start ticks, sum of shader
    // cycles, sum of 100 MHz ticks} (surfd_decoder_sustained_clock)
    HIP_TRY(hipMalloc((void **)&d->sat, 8 + 4 * sizeof(unsigned long long)));
    d->allocs.push_back(d->sat);
    HIP_TRY(hipMemset(d->sat, 0, 8 + 4 * sizeof(unsigned long long)));
    if (const char *pe = getenv("SURFD_DECODER_PRECISION")) d->precision = !strcmp(pe, "fp32") ? 0 : 1;
    if (const char *pe = getenv("SURFD_DECODER_FWD8")) d->fwd8 = atoi(pe) != 0;
    for (int l = 0; l < NCBN; ++l) {
        if ((rc = A(&d->gw[l], (size_t)H * d->D))) return rc;
        if ((rc = A(&d->bw[l], (size_t)H * d->D))) return rc;
        if ((rc = A(&d->gb[l], H))) return rc;
        if ((rc = A(&d->bb[l], H))) return rc;
        if ((rc = A(&d->mean[l], H))) return rc;
        if ((rc = A(&d->var[l], H))) return rc;
    }
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&decoder_kernel<false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)DEC_LDS_BYTES));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&decoder_kernel<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)DEC_LDS_BYTES));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&decoder_kernel<false, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)DEC_LDS_BYTES));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&decoder_kernel<true, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)DEC_LDS_BYTES));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&decoder_fwd8_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)DEC_LDS_BYTES));
    d->allocated = true;
    return SURFD_OK;
}

static int pack_matrix(const float *src, int N, int K, bool transpose, float *dst, hipStream_t s) {
    // logical W[n][k]; source is row-major [N][K] (or [K][N] when transpose: W^T)
    PackDesc pd;
    pd.src = src; pd.dst = dst;
    pd.N = N; pd.K = K;
    pd.Npad = ceil_div(N, 32) * 32; pd.Kpad = ceil_div(K, 8) * 8;
    pd.inner = pd.Kpad; pd.inner_valid = K; pd.os = 0;
    if (!transpose) { pd.rs = K; pd.is = 1; }
    else { pd.rs = 1; pd.is = N; }
    pd.KGtot = pd.Kpad / 8; pd.kg_off = 0;
    return launch_pack(pd, s);
}

extern "C" {

int surfd_decoder_create(int input_dim, int latent_dim, int hidden_dim, int num_blocks, surfd_decoder **out) {
    if (!out) SURFD_FAIL(SURFD_ERR_ARG, "surfd_decoder_create: out is null");
    if (hidden_dim != H || num_blocks != NB || input_dim < 1 || input_dim > 63 || latent_dim < 1)
        SURFD_FAIL(SURFD_ERR_UNSUPPORTED,
                   "surfd_decoder_create: kernels are built for CbnDecoder(<=63, D, 512, 5); got (%d, %d, %d, %d)",
                   input_dim, latent_dim, hidden_dim, num_blocks);
    auto *d = new surfd_decoder();
    d->input_dim = input_dim; d->D = latent_dim; d->hidden = hidden_dim; d->nb = num_blocks;
    dec_add(d, "decoder.fc_p.weight", {H, input_dim, 1});
    dec_add(d, "decoder.fc_p.bias", {H});
    for (int k = 0; k < NB; ++k) {
        const std::string b = "decoder.blocks." + std::to_string(k);
        dec_add_cbn(d, b + ".bn_0");
        dec_add_cbn(d, b + ".bn_1");
        dec_add(d, b + ".fc_0.weight", {H, H, 1}); dec_add(d, b + ".fc_0.bias", {H});
        dec_add(d, b + ".fc_1.weight", {H, H, 1}); dec_add(d, b + ".fc_1.bias", {H});
    }
    dec_add_cbn(d, "decoder.bn");
    dec_add(d, "decoder.fc_out.weight", {1, H, 1});
    dec_add(d, "decoder.fc_out.bias", {1});
    *out = d;
    return SURFD_OK;
}

void surfd_decoder_destroy(surfd_decoder *d) {
    if (!d) return;
    for (void *p : d->allocs) (void)hipFree(p);
    if (d->tab) (void)hipFree(d->tab);
    delete d;
}

int surfd_decoder_num_params(const surfd_decoder *d) { return d ? d->params.size() : 0; }

int surfd_decoder_param_info(const surfd_decoder *d, int i, const char **key, int64_t shape[4], int *ndim) {
    return param_info(d ? &d->params : nullptr, "surfd_decoder_param_info", i, key, shape, ndim);
}

int surfd_decoder_set_param(surfd_decoder *d, const char *key, const void *dev_ptr, const int64_t *shape, int ndim,
                            surfd_stream s) {
    if (!d) SURFD_FAIL(SURFD_ERR_ARG, "surfd_decoder_set_param: null handle");
    int pi, rc;
    if ((rc = d->params.match("surfd_decoder_set_param", key, shape, ndim, &pi))) return rc;
    if (d->params[pi].ignored) { d->params.mark(pi); return SURFD_OK; }
    if (!dev_ptr) SURFD_FAIL(SURFD_ERR_ARG, "surfd_decoder_set_param: '%s' has a null pointer", key);
    if ((rc = dec_alloc(d))) return rc;
    const std::string &k = d->params[pi].key;
    const size_t numel = d->params.numel(pi);
    hipStream_t st = as_stream(s);
    const float *src = static_cast<const float *>(dev_ptr);
    auto copy = [&](float *dst) -> int {
        HIP_TRY(hipMemcpyAsync(dst, src, numel * sizeof(float), hipMemcpyDeviceToDevice, st));
        return SURFD_OK;
    };
    // which CBN layer / block does the key belong to?
    auto cbn_index = [&](const std::string &kk) -> int {
        if (kk.rfind("decoder.bn.", 0) == 0) return 2 * NB;
        int blk = -1, which = -1;
        if (sscanf(kk.c_str(), "decoder.blocks.%d.bn_%d.", &blk, &which) == 2) return 2 * blk + which;
        return -1;
    };
    if (k == "decoder.fc_p.weight") {
        if ((rc = pack_matrix(src, H, d->input_dim, false, d->wpack + OFF_FCP, st))) return rc;
        // adjoint: rows = encoding index (padded to 64), k = hidden
        PackDesc pd;
        pd.src = src; pd.dst = d->wpack + OFF_FCPT; pd.N = d->input_dim; pd.K = H; pd.Npad = 64; pd.Kpad = H;
        pd.inner = H; pd.inner_valid = H; pd.os = 0; pd.rs = 1; pd.is = d->input_dim; pd.KGtot = KG_H; pd.kg_off = 0;
        rc = launch_pack(pd, st);
    } else if (k == "decoder.fc_p.bias") rc = copy(d->vecs + VOFF_BFCP);
    else if (k == "decoder.fc_out.weight") rc = copy(d->vecs + VOFF_WOUT);
    else if (k == "decoder.fc_out.bias") rc = copy(d->vecs + VOFF_BOUT);
    else if (k.find(".conv_gamma.weight") != std::string::npos) rc = copy(d->gw[cbn_index(k)]);
    else if (k.find(".conv_gamma.bias") != std::string::npos) rc = copy(d->gb[cbn_index(k)]);
    else if (k.find(".conv_beta.weight") != std::string::npos) rc = copy(d->bw[cbn_index(k)]);
    else if (k.find(".conv_beta.bias") != std::string::npos) rc = copy(d->bb[cbn_index(k)]);
    else if (k.find(".running_mean") != std::string::npos) rc = copy(d->mean[cbn_index(k)]);
    else if (k.find(".running_var") != std::string::npos) rc = copy(d->var[cbn_index(k)]);
    else {
        int blk = -1, which = -1;
        char leaf[16] = "";
        if (sscanf(k.c_str(), "decoder.blocks.%d.fc_%d.%15s", &blk, &which, leaf) != 3 || blk < 0 || blk >= NB)
            SURFD_FAIL(SURFD_ERR_ARG, "surfd_decoder_set_param: cannot place key '%s'", key);
        if (!strcmp(leaf, "bias")) rc = copy(d->vecs + voff_bfc(blk, which ? 1 : 0));
        else {
            if ((rc = pack_matrix(src, H, H, false, d->wpack + off_fc(blk, which ? 1 : 0), st))) return rc;
            rc = pack_matrix(src, H, H, true, d->wpack + off_fcT(blk, which ? 1 : 0), st);
        }
    }
    if (rc) return rc;
    d->params.mark(pi);
    d->finalized = false;
    return SURFD_OK;
}

int surfd_decoder_finalize(surfd_decoder *d, surfd_stream s) {
    if (!d) SURFD_FAIL(SURFD_ERR_ARG, "surfd_decoder_finalize: null handle");
    int rc;
    if ((rc = d->params.require_all("surfd_decoder_finalize"))) return rc;
    // f16x2 planes of the forward matrices: one power-of-two scale from max |W|, then split (all on the
    // stream, no host round trip); the fp32 packs are the source
    hipStream_t st = as_stream(s);
    unsigned *maxbits = reinterpret_cast<unsigned *>(d->vecs + VOFF_SC + 2);
    HIP_TRY(hipMemsetAsync(maxbits, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(absmax_kernel, dim3(512), dim3(256), 0, st, d->wpack, SZ_FCP + (size_t)2 * NB * SZ_HH, maxbits);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(weight_scale_kernel, dim3(1), dim3(1), 0, st, maxbits, d->vecs + VOFF_SC);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(cumbias_kernel, dim3(H / 256), dim3(256), 0, st, d->vecs);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(pack_f16x2_kernel, dim3(128), dim3(256), 0, st, d->wpack + OFF_FCP, KG_E, KS_E, 0, d->vecs + VOFF_SC, d->whf);
    LAUNCH_CHECK();
    for (int k = 0; k < NB; ++k)
        for (int which = 0; which < 2; ++which) {
            hipLaunchKernelGGL(pack_f16x2_kernel, dim3(1024), dim3(256), 0, st, d->wpack + off_fc(k, which), KG_H, KS_H, 1,
                               d->vecs + VOFF_SC, d->whf + hf_off_fc(k, which));
            LAUNCH_CHECK();
            hipLaunchKernelGGL(pack_f16x2_kernel, dim3(1024), dim3(256), 0, st, d->wpack + off_fcT(k, which), KG_H, KS_H, 1,
                               d->vecs + VOFF_SC, d->whf + hf_off_fcT(k, which));
            LAUNCH_CHECK();
        }
    d->finalized = true;
    return SURFD_OK;
}

#ifdef SURFD_DEC_STAMPS
extern "C" int surfd_decoder_debug_stamps(long long *out8, int reset) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_dec_stamps), 8 * sizeof(long long)));
    if (reset) { long long z[8] = {}; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_dec_stamps), z, sizeof(z))); }
    return SURFD_OK;
}
#endif

int surfd_decoder_set_grid_blocks(surfd_decoder *d, int blocks) {
    if (!d || blocks < 0) SURFD_FAIL(SURFD_ERR_ARG, "surfd_decoder_set_grid_blocks: bad argument");
    d->grid_blocks = blocks;
    return SURFD_OK;
}

int surfd_decoder_set_precision(surfd_decoder *d, int mode) {
    if (!d || (mode != 0 && mode != 1)) SURFD_FAIL(SURFD_ERR_ARG, "surfd_decoder_set_precision: mode must be 0 (fp32) or 1 (f16x2)");
    d->precision = mode;
    return SURFD_OK;
}

int surfd_decoder_saturation_count(surfd_decoder *d, int reset, int64_t *count, surfd_stream s) {
    if (!d || !count) SURFD_FAIL(SURFD_ERR_ARG, "surfd_decoder_saturation_count: null argument");
    *count = 0;
    if (!d->sat) return SURFD_OK;
    unsigned v = 0;
    hipStream_t st = as_stream(s);
    HIP_TRY(hipMemcpyAsync(&v, d->sat, sizeof(v), hipMemcpyDeviceToHost, st));
    if (reset) HIP_TRY(hipMemsetAsync(d->sat, 0, sizeof(v), st));
    HIP_TRY(hipStreamSynchronize(st));
    *count = v;
    return SURFD_OK;
}

int surfd_decoder_sustained_clock(surfd_decoder *d, int reset, double *ghz, surfd_stream s) {
    if (!d || !ghz) SURFD_FAIL(SURFD_ERR_ARG, "surfd_decoder_sustained_clock: null argument");
    *ghz = 0.0;
    if (!d->sat) return SURFD_OK;
    unsigned long long v[4] = {0, 0, 0, 0};
    hipStream_t st = as_stream(s);
    unsigned long long *clk = reinterpret_cast<unsigned long long *>(d->sat + 2);
    HIP_TRY(hipMemcpyAsync(v, clk, sizeof(v), hipMemcpyDeviceToHost, st));
    if (reset) HIP_TRY(hipMemsetAsync(clk + 2, 0, 2 * sizeof(unsigned long long), st));
    HIP_TRY(hipStreamSynchronize(st));
    if (v[3] > 0) {
        const double g = (double)v[2] / ((double)v[3] * 10.0);        // cycles per 10 ns tick = GHz x 10
        if (g > 0.0 && g <= 3.0) *ghz = g;                            // anything else is not a clock (a wrapped counter): reported as "not measured"
    }
    return SURFD_OK;
}

int surfd_decoder_bind_latents(surfd_decoder *d, const float *lat, int S, surfd_stream s) {
    if (!d || !lat || S < 1) SURFD_FAIL(SURFD_ERR_ARG, "surfd_decoder_bind_latents: bad argument");
    if (!d->finalized) SURFD_FAIL(SURFD_ERR_STATE, "surfd_decoder_bind_latents: call surfd_decoder_finalize first");
    if (S > d->tab_cap) {
        if (d->tab) HIP_TRY(hipFree(d->tab));
        d->tab = nullptr;
        HIP_TRY(hipMalloc((void **)&d->tab, (size_t)S * NCBN * 2 * H * sizeof(float)));
        d->tab_cap = S;
    }
    CbnParams P;
    for (int l = 0; l < NCBN; ++l) {
        P.gw[l] = d->gw[l]; P.gb[l] = d->gb[l]; P.bw[l] = d->bw[l]; P.bb[l] = d->bb[l];
        P.mean[l] = d->mean[l]; P.var[l] = d->var[l];
    }
    const int total = S * NCBN * H;
    hipLaunchKernelGGL(cbn_table_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, as_stream(s), P, lat, S, d->D, d->tab);
    LAUNCH_CHECK();
    d->S = S;
    return SURFD_OK;
}

}  // extern "C"

namespace surfd {

// Enqueue the decoder over a point source; used by the C entry points below and by grid.hip.
int decoder_launch(surfd_decoder *d, int sample, PtIO io, bool grad, long ntiles_hint, hipStream_t st) {
    PtBatch b;
    memset(&b, 0, sizeof(b));
    b.n = 1; b.sample[0] = sample; b.io[0] = io;
    return decoder_launch_batch(d, b, grad, ntiles_hint, st);
}

int decoder_launch_batch(surfd_decoder *d, const PtBatch &batch, bool grad, long ntiles_hint, hipStream_t st) {
    if (!d) SURFD_FAIL(SURFD_ERR_ARG, "decoder: null handle");
    if (!d->finalized) SURFD_FAIL(SURFD_ERR_STATE, "decoder: parameters not finalized");
    if (batch.n < 1 || batch.n > PT_BATCH_MAX) SURFD_FAIL(SURFD_ERR_ARG, "decoder: 1..%d point sources per launch", PT_BATCH_MAX);
    PtBatch io = batch;
    for (int i = 0; i < io.n; ++i) {
        if (io.sample[i] < 0 || io.sample[i] >= d->S)
            SURFD_FAIL(SURFD_ERR_STATE, "decoder: sample %d not bound (%d latents bound)", io.sample[i], d->S);
        io.io[i].emb_dim = d->input_dim;
    }
    DecParams P;
    P.wpack = d->wpack; P.vecs = d->vecs; P.whf = d->whf;
    P.tab = d->tab;
    P.input_dim = d->input_dim;
    P.sat = d->sat;
    // one workgroup per CU (LDS-limited); a device-side count is handled by the tile loop
    long blocks = d->grid_blocks > 0 ? std::min(d->grid_blocks, d->num_cus) : d->num_cus;
    if (ntiles_hint >= 0) blocks = std::min<long>(blocks, std::max<long>(ntiles_hint, 1));
    hipEvent_t prof_ev = prof_begin(grad ? PROF_DEC_GRAD : PROF_DEC_FWD, st);
    if (grad && d->precision == 1)
        hipLaunchKernelGGL((decoder_kernel<true, true>), dim3((unsigned)blocks), dim3(256), DEC_LDS_BYTES, st, P, io);
    else if (grad)
        hipLaunchKernelGGL(decoder_kernel<true>, dim3((unsigned)blocks), dim3(256), DEC_LDS_BYTES, st, P, io);
    else if (d->precision == 1 && d->fwd8)
        hipLaunchKernelGGL(decoder_fwd8_kernel, dim3((unsigned)blocks), dim3(512), DEC_LDS_BYTES, st, P, io);
    else if (d->precision == 1)
        hipLaunchKernelGGL((decoder_kernel<false, true>), dim3((unsigned)blocks), dim3(256), DEC_LDS_BYTES, st, P, io);
    else
        hipLaunchKernelGGL(decoder_kernel<false>, dim3((unsigned)blocks), dim3(256), DEC_LDS_BYTES, st, P, io);
    prof_end(grad ? PROF_DEC_GRAD : PROF_DEC_FWD, prof_ev, st);
    LAUNCH_CHECK();
    return SURFD_OK;
}

}  // namespace surfd

extern "C" {

static PtIO make_io(int mode, const float *src, int64_t n) {
    PtIO io;
    memset(&io, 0, sizeof(io));
    io.mode = mode; io.xyz = src; io.n = n;
    return io;
}

int surfd_decoder_logits_emb(surfd_decoder *d, int sample, const float *emb, int64_t n, float *logits, surfd_stream s) {
    if (n == 0) return SURFD_OK;          // empty query: nothing to do (pointers may be null)
    if (!emb || !logits || n < 0) SURFD_FAIL(SURFD_ERR_ARG, "surfd_decoder_logits_emb: bad argument");
    PtIO io = make_io(PT_EMB, emb, n);
    io.out_logit = logits;
    return decoder_launch(d, sample, io, false, ceil_div<long>(n, TP), as_stream(s));
}

int surfd_decoder_udf(surfd_decoder *d, int sample, const float *pts, int64_t n, float *udf, float *logits, surfd_stream s) {
    if (n == 0) return SURFD_OK;
    if (!pts || (!udf && !logits) || n < 0) SURFD_FAIL(SURFD_ERR_ARG, "surfd_decoder_udf: bad argument");
    PtIO io = make_io(PT_XYZ, pts, n);
    io.out_udf = udf; io.out_logit = logits;
    return decoder_launch(d, sample, io, false, ceil_div<long>(n, TP), as_stream(s));
}

int surfd_decoder_udf_grad(surfd_decoder *d, int sample, const float *pts, int64_t n, float *udf, float *ngrad,
                           float *dlogit, surfd_stream s) {
    if (n == 0) return SURFD_OK;
    if (!pts || (!ngrad && !dlogit) || n < 0) SURFD_FAIL(SURFD_ERR_ARG, "surfd_decoder_udf_grad: bad argument");
    PtIO io = make_io(PT_XYZ, pts, n);
    io.out_udf = udf; io.out_ngrad = ngrad; io.out_dlogit = dlogit;
    return decoder_launch(d, sample, io, true, ceil_div<long>(n, TP), as_stream(s));
}

}  // extern "C"
