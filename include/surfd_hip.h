/*
 * surfd_hip.h — C ABI of libsurfd_hip.so: the MI355X (gfx950) implementation of Surf-D's
 * sampling hot path.  Plain pointers and sizes only; no torch types.
 *
 * The reference (Yzmblog/SurfD) has no FFI layer: its boundary is the set of Python call
 * signatures used by sample/generate_*.py.  Every entry point below names the reference
 * interface it replaces (paths relative to the reference root); INTEGRATION.md shows the
 * ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *  - every function returns 0 on success or a negative surfd_status; the message is
 *    available from surfd_last_error() (thread-local).  No exceptions, no abort().
 *  - all device buffers are owned by the caller (torch), contiguous, fp32 unless noted;
 *    the library owns only re-laid-out private weight copies and a workspace arena.
 *  - all work is enqueued on the caller's hipStream_t (passed as void*); functions do
 *    not synchronise unless documented ("host-sync").
 *  - handles are bound to the device current at create time; one handle per process/rank.
 */
#ifndef SURFD_HIP_H
#define SURFD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    SURFD_OK = 0,
    SURFD_ERR_ARG = -1,        /* bad shape / null pointer / unknown key      */
    SURFD_ERR_STATE = -2,      /* missing parameter, latents not bound, ...   */
    SURFD_ERR_HIP = -3,        /* a HIP runtime call failed                   */
    SURFD_ERR_UNSUPPORTED = -4 /* configuration outside what the path covers  */
} surfd_status;

typedef void *surfd_stream;    /* hipStream_t */
typedef struct surfd_unet surfd_unet;
typedef struct surfd_decoder surfd_decoder;
typedef struct surfd_grid surfd_grid;

const char *surfd_last_error(void);
int surfd_abi_version(void);
/* number of visible HIP devices (0 on a CPU-only host; never fails) */
int surfd_device_count(void);
/* Compile-time configuration of the library (no reference counterpart): "name=value" for every experiment macro of the kernel
 * sources, then "unsafe_variants=N" = how many of them select a variant recorded as wrong, not bit-stable, or a developer aid
 * (0 for the product build: such variants need -DSURFD_ALLOW_UNSAFE_VARIANTS to compile at all).  bench.py prints it as
 * config.build_flags; tests/test_abi_cpu.py asserts the shipped library was built with the defaults.  Static storage. */
const char *surfd_build_config(void);

/* Measurement aid (no reference counterpart): when enabled, the library brackets its dominant
 * kernels with HIP events on the stream they are launched on.  kind 0 = decoder forward kernel,
 * 1 = decoder forward+reverse kernel, 2 = whole surfd_sample_loop.  read is host-sync and clears. */
int surfd_profile_enable(int on);
int surfd_profile_read(int kind, int64_t *launches, double *total_ms);
/* developer aid: with SURFD_CONV_DEBUG=1 in the environment every conv launch records shader-clock
 * stamps of its phases (16 int64 per launch); host-sync read + reset, returns the launch count */
int surfd_unet_debug_read(surfd_unet *u, long long *out, int max_launches);

/* ------------------------------------------------------------------------------------ */
/* Denoiser: UNetModel (models/openaimodel.py:413-749) as configured by MDM             */
/* (models/mdm.py:34-57).                                                               */
/* ------------------------------------------------------------------------------------ */
typedef struct {
    int in_channels, model_channels, out_channels, num_res_blocks;
    int n_mult, channel_mult[8];
    int n_attn, attention_resolutions[8];
    int num_heads;
    int context_dim;   /* 0: no sketch_emb */
    int num_classes;   /* 0: no label_emb  */
} surfd_unet_cfg;

/* Builds the execution plan on the host (no device needed).  Replaces
 * UNetModel.__init__ (openaimodel.py:443-692). */
int surfd_unet_create(const surfd_unet_cfg *cfg, surfd_unet **out);
void surfd_unet_destroy(surfd_unet *u);
/* state_dict layout the handle expects (keys relative to "Unet.", reference order):
 * lets the host build its nn.Module / check a checkpoint without a device. */
int surfd_unet_num_params(const surfd_unet *u);
int surfd_unet_param_info(const surfd_unet *u, int i, const char **key, int64_t shape[4], int *ndim);
/* One call per state_dict tensor (load_model_wo_clip, utils/model_util.py:6-9).
 * dev_ptr: device fp32, contiguous; repacked into the private MFMA fragment layout. */
int surfd_unet_set_param(surfd_unet *u, const char *key, const void *dev_ptr,
                         const int64_t *shape, int ndim, surfd_stream s);
/* fails with SURFD_ERR_STATE naming the first tensor that was not set */
int surfd_unet_finalize(surfd_unet *u, surfd_stream s);
/* UNetModel.forward (openaimodel.py:710-749) / MDM.forward (mdm.py:91-110):
 * x[B,1,L], t[B] (int64, original-scale timesteps), ctx[B,context_dim] or NULL,
 * cls[B] (int64) or NULL -> out[B,1,L].  All device pointers. */
int surfd_unet_forward(surfd_unet *u, const float *x, const int64_t *t, const float *ctx,
                       const int64_t *cls, float *out, int B, int L, surfd_stream s);

/* Arithmetic of the denoiser's convolutions (every Conv1d of openaimodel.py ResBlock / AttentionBlock /
 * Downsample / Upsample / head; the embedding Linears always run in fp32):
 * 1 = "f16x2" (default): operands split into two fp16 terms, three products on the fp16 matrix pipe, fp32
 *     accumulation (same scheme as surfd_decoder_set_precision); operands outside +-65504 are clamped and
 *     counted (surfd_unet_saturation_count).  0 = "fp32": exact v_mfma_f32_32x32x2_f32, no range limit.
 * The initial mode can also be set with SURFD_UNET_PRECISION=fp32|f16x2. */
int surfd_unet_set_precision(surfd_unet *u, int mode);
/* How many CUs this handle's launches can count on (default 256 = the whole chip).  The conv kernel splits the
 * contraction of small layers over extra workgroups until about two per CU are in flight; a handle that shares the
 * chip (several loops next to the decoder, surfd_amd.parallel.BatchPipeline) is told its share so that it does not
 * pay the split's redundant operand staging for parallelism it cannot get.  Results for different budgets differ in
 * fp32 summation order only.  No reference counterpart. */
int surfd_unet_set_cu_budget(surfd_unet *u, int cus);
/* Work decomposition of the f16x2 conv kernel.  design_batch = 0 (default): latency form — a workgroup owns one
 * 32-row tile of a layer's output and the K split follows the batch at hand: fastest for ONE narrow loop alone on
 * the chip.  design_batch > 0: wide form for loops over tens of latents (reference: the `batch_size` of
 * sample/generate_*.py is the only batching the reference has) — a workgroup stages its GroupNorm/SiLU operand once
 * for FOUR row tiles, and the K split is fixed per layer for a batch of `design_batch`, so a latent's result is
 * bit-identical whatever batch width it rides in (tests/test_gpu_unet.py).  Results of the two forms differ in fp32
 * summation order only.  No reference counterpart. */
int surfd_unet_set_wide(surfd_unet *u, int design_batch);
/* host-sync: number of workgroups of the f16x2 conv kernel that had to clamp an operand to the fp16 range since the
 * last reset (0 = every evaluation so far was inside the range the mode is exact for) */
int surfd_unet_saturation_count(surfd_unet *u, int reset, int64_t *count, surfd_stream s);
/* Iterations the handle's fused reverse loop (surfd_sample_loop) has finished so far — the device-side loop counter, read over a
 * private stream beside the one the loop runs on, so a host thread can draw the reference's progress bar
 * (diffusion/gaussian_diffusion.py:677-681, `progress=True` in every sample/generate_*.py) while the loop is in flight.
 * *iteration = -1 before the first loop. */
int surfd_unet_loop_progress(surfd_unet *u, int *iteration);
/* developer aid: op >= 0 restricts the f16x2 kernel to that one conv op of the plan (the others run fp32); -1 lifts it */
int surfd_unet_debug_only_op(surfd_unet *u, int op);
/* test tap: runs only the ops of ONE module of UNetModel ("input_blocks.1.0" ResBlock, "input_blocks.1.1" AttentionBlock,
 * "input_blocks.3.0" Downsample, "out" head, ...) on in[B,Cin,Lin] -> out[B,Cout,Lout], with the embedding rows left by
 * the preceding surfd_unet_forward (same t, B, L): lets the tests compare single modules with the reference's hooks */
int surfd_unet_debug_run_module(surfd_unet *u, const char *module, const float *in, int Cin, int Lin,
                                float *out, int Cout, int Lout, int B, int L, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Reverse loop: p_sample_loop / ddim_sample_loop                                       */
/* (diffusion/gaussian_diffusion.py:570-708, 858-972; diffusion/respace.py:63-132).      */
/* ------------------------------------------------------------------------------------ */
typedef struct {
    int sampler;            /* 0 = DDPM ancestral (p_sample :471-520), 1 = DDIM (:711-761) */
    int num_steps;          /* T' (after respacing)                                         */
    int clip_denoised;      /* clamp x0 to [-1,1] (process_xstart :330-336)                 */
    float eta;              /* DDIM only                                                    */
    const int64_t *timestep_map;   /* host [T']: loop index -> original timestep (respace.py:123-128) */
    /* host float32 tables [T'], already cast float64->float32 as _extract_into_tensor does (:1339) */
    const float *coef1, *coef2, *log_variance;                /* DDPM */
    const float *sqrt_recip_ab, *sqrt_recipm1_ab, *ab, *ab_prev;   /* DDIM */
} surfd_sampler_cfg;

/* Whole reverse loop without returning to the host: noise[T'+1,B,1,L] (row 0 = x_T,
 * row 1+k = z of loop iteration k), ctx/cls as in surfd_unet_forward (constant over the
 * loop), x_out[B,1,L]; traj (nullable) [T',B,1,L] receives x after every iteration.
 * One iteration (~117 kernel nodes) is captured once into a hipGraph and replayed T' times on the
 * caller's stream.  Host-sync once at entry (schedule tables are uploaded and the stream is quiesced
 * before capture); the T' replays themselves are asynchronous. */
int surfd_sample_loop(surfd_unet *u, const surfd_sampler_cfg *cfg, const float *noise,
                      const float *ctx, const int64_t *cls, float *x_out, float *traj,
                      int B, int L, surfd_stream s);
/* The same loop in three calls, for a host thread that drives several loops (one surfd_unet handle and one stream each) in
 * turns: begin = the host-synchronous part (embedding rows, coefficient table, state <- noise row 0, the captured iteration),
 * run = up to `iterations` more graph replays on s (asynchronous; *remaining, nullable, = replays still to launch),
 * end = x_out <- state once every iteration has been launched (SURFD_ERR_STATE before that).  begin + run(T') + end IS
 * surfd_sample_loop; noise / ctx / cls / traj must stay alive until the stream has passed end.  One loop per handle at a time
 * (a second begin on the same handle abandons the first; several loops = several handles, all three calls of a handle from one
 * host thread or externally serialised); a begin that fails leaves no loop open.  The loop they spell is
 * p_sample_loop_progressive's for-loop (diffusion/gaussian_diffusion.py:682-708) cut at iteration boundaries. */
int surfd_sample_loop_begin(surfd_unet *u, const surfd_sampler_cfg *cfg, const float *noise,
                            const float *ctx, const int64_t *cls, float *traj, int B, int L,
                            surfd_stream s);
int surfd_sample_loop_run(surfd_unet *u, int iterations, int *remaining, surfd_stream s);
int surfd_sample_loop_end(surfd_unet *u, float *x_out, surfd_stream s);
/* single posterior updates on n elements (used by the generic Python loop) */
int surfd_ddpm_step(const float *x_t, const float *x0, const float *z, float coef1, float coef2,
                    float log_variance, int t_nonzero, int clip_denoised, float *out, int64_t n,
                    surfd_stream s);
int surfd_ddim_step(const float *x_t, const float *x0, const float *z, float sqrt_recip_ab,
                    float sqrt_recipm1_ab, float ab, float ab_prev, float eta, int t_nonzero,
                    int clip_denoised, float *out, int64_t n, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* UDF field: CoordsEncoder.encode (AutoEncoder/models/coordsenc.py:25-51) +             */
/* CbnDecoder.forward (AutoEncoder/models/cbndec.py:35-47,127-134) + the udf_func        */
/* closure (sample/generate_uncond.py:96-101) + sample_grads (meshudf/meshudf.py:231-251) */
/* ------------------------------------------------------------------------------------ */
int surfd_decoder_create(int input_dim, int latent_dim, int hidden_dim, int num_blocks,
                         surfd_decoder **out);
void surfd_decoder_destroy(surfd_decoder *d);
int surfd_decoder_num_params(const surfd_decoder *d);
int surfd_decoder_param_info(const surfd_decoder *d, int i, const char **key, int64_t shape[4], int *ndim);
/* keys exactly as in ckpt["decoder"] ("decoder.fc_p.weight", ...); num_batches_tracked is
 * accepted and ignored (dev_ptr may be NULL for it). */
int surfd_decoder_set_param(surfd_decoder *d, const char *key, const void *dev_ptr,
                            const int64_t *shape, int ndim, surfd_stream s);
int surfd_decoder_finalize(surfd_decoder *d, surfd_stream s);
/* Arithmetic of the decoder kernels (udf / logits / grid fill, and the forward + reverse sweep of
 * surfd_decoder_udf_grad):
 * 1 = "f16x2" (default): every fp32 operand is split into two fp16 terms (weights pre-scaled by one power
 *     of two), the three significant products are accumulated in fp32 on the fp16 matrix pipe.  Error
 *     against an fp64 evaluation is the same size as the plain fp32 kernel's (tests/test_gpu_decoder_grid.py);
 *     activations saturate at 65504.  2.85x the throughput of mode 0 on MI355X.
 * 0 = "fp32": v_mfma_f32_32x32x2_f32, bitwise an fmaf chain, no range limit.
 * In mode 1 the reverse sweep scales the adjoint of each 64-point tile by one power of two before the fp16 split
 * (exact, divided out afterwards; no range limit): directions agree with mode 0 to the golden tolerance, but a point's
 * last bits can depend on the points it shares a tile with; mode 0 is bitwise independent of the tiling.
 * The initial mode can also be set with SURFD_DECODER_PRECISION=fp32|f16x2. */
int surfd_decoder_set_precision(surfd_decoder *d, int mode);
/* host-sync: waves of the f16x2 forward kernel that produced an activation beyond +-65504 (clamped) since the last
 * reset.  Non-zero = this checkpoint / latent leaves the range mode 1 is exact for: switch to mode 0. */
int surfd_decoder_saturation_count(surfd_decoder *d, int reset, int64_t *count, surfd_stream s);
/* Shader clock (GHz) the chip sustained under the forward decoder kernel since the last reset: workgroup 0 of every launch of the
 * 8-wave forward kernel adds its shader-cycle and 100 MHz real-time differences to a device-side record (the kernel is
 * power-bound: its rate follows this clock, bench.py `roofline.sustained_clock_ghz`).  0 when no launch ran.  Measurement aid,
 * no reference counterpart. */
int surfd_decoder_sustained_clock(surfd_decoder *d, int reset, double *ghz, surfd_stream s);
/* The decoder kernels are persistent: `blocks` workgroups (one per CU, LDS-limited) loop over the point tiles.
 * 0 (default) = every CU.  A smaller value leaves CUs free for work on another stream (bench.py overlaps the
 * reverse loop of the next batch with the grid evaluation of the current one this way). */
int surfd_decoder_set_grid_blocks(surfd_decoder *d, int blocks);
/* lat[S,D]: computes the per-sample conditional-BN scale/shift tables [S,11,2,H]
 * (the 22 per-point Conv1d(D->H) of cbndec.py:74-79 collapse to this when one latent is
 * broadcast to all points, cbndec.py:131-132). */
int surfd_decoder_bind_latents(surfd_decoder *d, const float *lat, int S, surfd_stream s);
/* CbnDecoder.forward on pre-encoded coordinates emb[n,input_dim] -> logits[n] */
int surfd_decoder_logits_emb(surfd_decoder *d, int sample, const float *emb, int64_t n,
                             float *logits, surfd_stream s);
/* udf_func: pts[n,3] -> udf[n] = (1 - sigmoid(decoder(encode(p), lat))) * 0.1;
 * logits (nullable) receives the raw decoder output */
int surfd_decoder_udf(surfd_decoder *d, int sample, const float *pts, int64_t n, float *udf,
                      float *logits, surfd_stream s);
/* sample_grads: ngrad[n,3] = -normalize(d udf/d p) (eps 1e-12; exact zero vector where the
 * fp32 sigmoid derivative vanishes); udf (nullable) as above; dlogit (nullable) receives the
 * raw d logit / d p [n,3] (what an autograd backward through CbnDecoder.forward needs).
 * At least one of ngrad / dlogit must be given. */
int surfd_decoder_udf_grad(surfd_decoder *d, int sample, const float *pts, int64_t n, float *udf,
                           float *ngrad, float *dlogit, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* UDF grid: GridFiller / get_udf_and_grads (meshudf/meshudf.py:23-304)                  */
/* ------------------------------------------------------------------------------------ */
#define SURFD_GRID_MAX_LEVELS 8
typedef struct {
    int n_levels;
    int levels[SURFD_GRID_MAX_LEVELS];
    int64_t fwd_points[SURFD_GRID_MAX_LEVELS];   /* decoder forward queries per level */
    int64_t grad_points;                         /* forward+backward queries          */
} surfd_grid_stats;

/* N = final resolution (power of two >= 64); allocates the per-level work lists. */
int surfd_grid_create(int N, surfd_grid **out);
void surfd_grid_destroy(surfd_grid *g);
/* thresholds are computed by the host exactly as the reference's Python does and handed
 * over as float32: refine[l] = float32(1.5*1.7*(2.0/levels[l])) (meshudf.py:185-188),
 * grad = float32(2.5*2.0/N) (:200), voxel = float32(2.0/(N-1)) (:53), origin -1. */
int surfd_grid_set_thresholds(surfd_grid *g, const float *refine, int n_levels, float grad_thr,
                              float voxel, float origin);
/* GridFiller.fill_grid fused with the native decoder: no host round trip, no Python.
 * udf[N^3], grads[N^3*3] device outputs (grads may be NULL: watertight variant,
 * utils/utils.py:151-339). */
int surfd_grid_fill(surfd_grid *g, surfd_decoder *d, int sample, float *udf, float *grads,
                    surfd_stream s);
/* The same for the grids of n <= 8 shapes at once (what the sample scripts do shape after shape, generate_uncond.py:
 * 91-123): one grid handle, bound-latent index, udf and grads (entries or the array may be NULL) pointer per shape.
 * Every refinement level of all shapes is ONE launch of the persistent decoder kernel; values are bit-identical to n
 * calls of surfd_grid_fill.  No reference counterpart (throughput form). */
int surfd_grid_fill_batch(surfd_grid *const *grids, int n, surfd_decoder *d, const int *samples, float *const *udf,
                          float *const *grads, surfd_stream s);
/* get_udf_and_grads (use_fast_grid_filler=False): all N^3 points, gradients where
 * udf < grad_below (= max_dist - 1e-3 in the reference). */
int surfd_grid_fill_dense(surfd_grid *g, surfd_decoder *d, int sample, float grad_below,
                          float *udf, float *grads, surfd_stream s);
/* host-sync: counters of the last fill on this handle */
int surfd_grid_get_stats(surfd_grid *g, surfd_grid_stats *out, surfd_stream s);
/* host-sync: running totals over every fused fill (surfd_grid_fill / _fill_batch / _fill_dense) on this handle since
 * the last reset — decoder forward queries per level, forward+backward queries, number of fills.  The totals are kept
 * on the device by the fills themselves, so a throughput run can account for every query of hundreds of different
 * shapes without a host read-back per shape (the reference prints nothing of the kind; bench.py's roofline uses it). */
int surfd_grid_get_totals(surfd_grid *g, surfd_grid_stats *out, int64_t *fills, int reset, surfd_stream s);

/* Same algorithm with an arbitrary host callable (the reference's udf_func contract):
 * begin -> for each level { points -> [host evaluates] -> commit } -> grad_points ->
 * [host differentiates] -> grad_commit.  *_points are host-sync (they return a count). */
int surfd_grid_begin(surfd_grid *g, float *udf, float *grads, surfd_stream s);
int surfd_grid_level_points(surfd_grid *g, int level, float *xyz, int64_t capacity, int64_t *n,
                            surfd_stream s);
int surfd_grid_level_commit(surfd_grid *g, int level, const float *values, int64_t n, surfd_stream s);
int surfd_grid_grad_points(surfd_grid *g, float *xyz, int64_t capacity, int64_t *n, surfd_stream s);
int surfd_grid_grad_commit(surfd_grid *g, const float *ngrads, int64_t n, surfd_stream s);

/* Grid-shard mode (no reference counterpart: the reference fills one grid on one device, meshudf/meshudf.py:123-206; this is the
 * north star's "shard the per-sample 512^3 grid evaluation across the GPUs").  Every one of `world` ranks runs, on its own device,
 *   shard_begin -> per level { shard_level_eval -> shard_pack -> [ncclAllGather of the ranks' segments] -> shard_level_commit }
 *               -> shard_grad_eval -> shard_pack -> [all-gather] -> shard_grad_commit
 * with the native decoder: rank r evaluates the 64-point tiles r, r + world, ... of each level's VOXEL-ORDERED point list (the
 * same list on every rank) into vals[point number]; shard_pack compacts exactly those tiles into the rank's SEGMENT of
 * capacity / world points (tile t of the list = tile t / world of rank t % world's segment), the segments are all-gathered into
 * [world][capacity / world] (an all-gather of compact slices — half the bytes of summing zero-filled
 * point-indexed buffers, and nothing to zero), and shard_level_commit(world) reads point e from the gathered layout.  With
 * world = 1 there is no pack and no exchange: commit reads the point-indexed buffer.  All calls are stream-ordered and none reads a count back: list lengths stay on the device, `capacity` (points) bounds what a level may hold —
 * a list longer than its buffer is cut and COUNTED on the device (surfd_grid_shard_overflows; the counts themselves are in
 * surfd_grid_get_stats).  The handle tracks the protocol: a call that names another level than the open fill is at, a commit
 * without an evaluation, or a commit with another capacity than its evaluation returns SURFD_ERR_STATE.
 * With world = 1 the result equals surfd_grid_fill bit for bit. */
int surfd_grid_shard_begin(surfd_grid *g, float *udf, float *grads, surfd_stream s);
int surfd_grid_shard_level_eval(surfd_grid *g, surfd_decoder *d, int sample, int level, int rank, int world, float *vals,
                                int64_t capacity, surfd_stream s);
/* this rank's tiles of the step's point-indexed buffer -> its segment [capacity / world] (x 3 floats for the gradient step, named
 * by level = number of levels); capacity must be whole 64-point tiles of every rank */
int surfd_grid_shard_pack(surfd_grid *g, int level, int rank, int world, const float *vals, int64_t capacity, float *segment,
                          surfd_stream s);
int surfd_grid_shard_level_commit(surfd_grid *g, int level, const float *vals, int64_t capacity, int world, surfd_stream s);
int surfd_grid_shard_grad_eval(surfd_grid *g, surfd_decoder *d, int sample, int rank, int world, float *ngrads, int64_t capacity,
                               surfd_stream s);
int surfd_grid_shard_grad_commit(surfd_grid *g, const float *ngrads, int64_t capacity, int world, surfd_stream s);
/* Exchange buffers that were shorter than the list they carried, over the sharded fills since the last reset (levels and gradient
 * lists; 0 = every grid of that span is complete).  Synchronises the stream (one 8-byte read).  No reference counterpart. */
int surfd_grid_shard_overflows(surfd_grid *g, int64_t *n, int reset, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* UDF marching cubes (host side, no device): udf_mc_lewiner / marching_cubes_udf        */
/* (meshudf/_marching_cubes_lewiner.py:87-154, meshudf/_marching_cubes_lewiner_cy.pyx:1115-1775) */
/* ------------------------------------------------------------------------------------ */
typedef struct surfd_mc surfd_mc;
/* udf[nz,ny,nx] and grads[nz,ny,nx,3] are HOST arrays (the grids of surfd_grid_fill copied back, udf clamped at 0).
 * Meshes the zero set: signs of the cube corners are voted from the gradient field, cubes are triangulated with
 * Lewiner et al.'s case tables.  Output bit-identical to the reference extension.  One shape per call, one thread. */
int surfd_mc_udf(const float *udf, const float *grads, int nz, int ny, int nx, int step, surfd_mc **out);
/* Level-set marching cubes over the whole volume (watertight path: sample/generate_text.py:139-141 extracts the 0.01
 * level with PyMCubes).  classic != 0: the original 256-case triangle table (PyMCubes' algorithm); 0: Lewiner's
 * disambiguated cases.  Same result accessors as surfd_mc_udf. */
int surfd_mc_iso(const float *volume, int nz, int ny, int nx, double level, int classic, int step, surfd_mc **out);
/* Sparse hand-off (reference meshudf/meshudf.py:344-349 copies the whole grid and gradient volume to the
 * host, _marching_cubes_lewiner_cy.pyx:1131,1157-1158 then looks only at cubes whose corners are all <= 1.74 voxel):
 *   device: surfd_band_compact  — voxel index, value (clamped at 0 as meshudf.py:338), gradient of every voxel with
 *           udf <= max_thr, in voxel order, into the handle's device buffers (stream-ordered, no host sync)
 *   host:   surfd_band_fetch    — host-sync on `copy_stream` only: count, then the band, into pinned memory
 *           surfd_mc_udf_band   — scatters the band into a host scratch volume that is "far" everywhere else, runs the
 *           same mesher, takes the band out again: the mesh of surfd_mc_udf on the dense volumes, bit for bit, at a cost
 *           proportional to the band. */
typedef struct surfd_band surfd_band;
typedef struct surfd_mc_scratch surfd_mc_scratch;
int surfd_band_create(int N, int64_t capacity, surfd_band **out);
void surfd_band_destroy(surfd_band *b);
int surfd_band_compact(surfd_band *b, const float *udf, const float *grads, float max_thr, surfd_stream s);
int surfd_band_fetch(surfd_band *b, surfd_stream copy_stream, int64_t *count, const int32_t **index, const float **packed);
int surfd_mc_band_threshold(int n, float *max_thr);          /* float(1.74 * 2 / (n - 1)), as the mesher compares */
int surfd_mc_scratch_create(int n, surfd_mc_scratch **out);  /* host: n^3 x (4 + 12 + 1) bytes, zero pages until touched */
void surfd_mc_scratch_destroy(surfd_mc_scratch *sc);
int surfd_mc_udf_band(surfd_mc_scratch *sc, const int32_t *index, const float *packed /* [count][4]: udf, gx, gy, gz */,
                      int64_t count, int step, surfd_mc **out);
int64_t surfd_mc_num_vertices(const surfd_mc *m);
int64_t surfd_mc_num_faces(const surfd_mc *m);
/* vertices[V,3] in (z,y,x) voxel units, faces[F,3] (winding of gradient_direction="descent"), normals[V,3] (unit),
 * values[V]; any pointer may be NULL */
int surfd_mc_copy(const surfd_mc *m, float *vertices, int32_t *faces, float *normals, float *values);
void surfd_mc_destroy(surfd_mc *m);
/* Wavefront OBJ writer for the meshes above ("v x y z" with 6 decimals, 1-based "f a b c"): the export step of the sample
 * scripts (sample/generate_uncond.py:113-122).  vertices[nv,3] float64, faces[nf,3] int64, host arrays. */
int surfd_write_obj(const char *path, const double *vertices, int64_t nv, const int64_t *faces, int64_t nf);
/* the case tables the library was built with (Lewiner et al. 2003), for tests */
int surfd_mc_lut_count(void);
int surfd_mc_lut(int i, const char **name, const signed char **values, int *ndim, int dims[3]);

/* ------------------------------------------------------------------------------------ */
/* Level-set marching cubes on the device (csrc/mcdevice.hip): the mesh of surfd_mc_iso   */
/* with step 1 from a volume that stays on the GPU (the watertight path,                  */
/* sample/generate_text.py:139-141).  The result equals surfd_mc_iso + surfd_mc_copy on    */
/* the same volume bit for bit: vertex order, face order, every float, -0 / +0.  No step   */
/* > 1, no mask, one volume per call.                                                      */
/* ------------------------------------------------------------------------------------ */
typedef struct surfd_mcd surfd_mcd;
/* A handle for volumes [nz, ny, nx], each extent >= 2 (SURFD_ERR_ARG below), nz ny nx < 2^31 (SURFD_ERR_UNSUPPORTED beyond).
 * Owns 0.31 bytes of device scratch per voxel, plus 24 bytes per active cube of the largest run it has seen.  Reusable for any
 * number of volumes of that shape; no run sees anything of the run before.  One stream and one host thread at a time. */
int surfd_mcd_create(int nz, int ny, int nx, surfd_mcd **out);
void surfd_mcd_destroy(surfd_mcd *h);
/* volume[nz,ny,nx] fp32 on the device, contiguous; it must stay unchanged until surfd_mcd_emit has run.  Finds the cubes the
 * level crosses (corner above iff (double)value - level > 0.0), counts and numbers their triangles and vertices in the scan order
 * of the host mesher.  classic as in surfd_mc_iso.  num_vertices / num_faces (host, nullable): the sizes surfd_mcd_emit fills.
 * More than 2^31 - 1 vertices or faces: SURFD_ERR_UNSUPPORTED, nothing is emitted.  host-sync (the three totals are read back:
 * the one read of the path). */
int surfd_mcd_run(surfd_mcd *h, const float *volume, double level, int classic, surfd_stream s, int64_t *num_vertices, int64_t *num_faces);
/* The mesh of the last surfd_mcd_run (SURFD_ERR_STATE without one), on the same stream: vertices[V,3] fp32 in (z, y, x) voxel
 * units, faces[F,3] int32 (winding of gradient_direction="descent"), normals[V,3] (unit; nullable), values[V] (nullable), device
 * memory, as surfd_mc_copy hands them out.  An empty run (V = F = 0) writes nothing and accepts null pointers.  Does not sync. */
int surfd_mcd_emit(surfd_mcd *h, float *vertices, int32_t *faces, float *normals, float *values, surfd_stream s);
/* no reference counterpart; the number of cubes the level crosses in the last run, for measurements:
 * host memory.  SURFD_ERR_STATE without a run. */
int surfd_mcd_active(const surfd_mcd *h, int64_t *active);
/* no reference counterpart; the first pass of surfd_mcd_run alone, for measurements against the time to stream the volume once:
 * reads the volume, leaves the per-chunk masks and counts in the handle.  It overwrites those of the last run: surfd_mcd_emit is
 * SURFD_ERR_STATE until the next surfd_mcd_run.  Does not sync. */
int surfd_mcd_classify(surfd_mcd *h, const float *volume, double level, int classic, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* CrossAttention over [b, n, c] tokens (modules/attention.py:152-193) — SURVEY §8 a19.  */
/* No Surf-D configuration instantiates the module (use_spatial_transformer is False);    */
/* a standalone op with its own handle, fp32 on the matrix pipe.                           */
/* ------------------------------------------------------------------------------------ */
typedef struct surfd_xattn surfd_xattn;
/* CrossAttention.__init__(query_dim, context_dim=None, heads=8, dim_head=64) (:153-169); context_dim <= 0 means
 * "same as query_dim".  dim_head <= 128. */
int surfd_xattn_create(int query_dim, int context_dim, int heads, int dim_head, surfd_xattn **out);
void surfd_xattn_destroy(surfd_xattn *a);
/* state_dict entries of the reference module, fp32 device pointers: "to_q.weight" [heads*dim_head, query_dim],
 * "to_k.weight" / "to_v.weight" [heads*dim_head, context_dim], "to_out.0.weight" [query_dim, heads*dim_head],
 * "to_out.0.bias" [query_dim] */
int surfd_xattn_set_param(surfd_xattn *a, const char *name, const float *src, const int64_t *shape, int ndim, surfd_stream s);
/* CrossAttention.forward(x, context=None, mask=None) (:171-193): x [B, N, query_dim]; context [B, M, context_dim] or
 * NULL (self-attention, M ignored); mask [B, M] bytes, non-zero = attend, or NULL (masked scores are set to
 * -FLT_MAX exactly as masked_fill_ does, so a fully masked row attends uniformly); out [B, N, query_dim].
 * Dropout (p = 0 in every constructor call of the reference) is the identity.
 * Limits (SURFD_ERR_UNSUPPORTED beyond them): B * heads <= 65535; B * N and B * M <= (2^24 - 1) * 64 = 1 073 741 760 rows. */
int surfd_xattn_forward(surfd_xattn *a, const float *x, const float *context, const unsigned char *mask, float *out,
                        int B, int N, int M, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Point-cloud encoder: Dgcnn (AutoEncoder/models/dgcnn.py:9-115), eval mode.             */
/* Used frozen by AutoEncoder/encdec/export_meshes.py:61-100 and training_loop_single.py  */
/* to turn point clouds into latents.  Plain fp32; bitwise deterministic.                 */
/* ------------------------------------------------------------------------------------ */
typedef struct surfd_dgcnn surfd_dgcnn;
/* Dgcnn(size_latent, k) with aggregate_ops_local = aggregate_ops_global = "max" (AutoEncoder/models/dgcnn.py:27-53); 1 <= k <= 32. */
int surfd_dgcnn_create(int size_latent, int k, surfd_dgcnn **out);
void surfd_dgcnn_destroy(surfd_dgcnn *d);
int surfd_dgcnn_num_params(const surfd_dgcnn *d);
/* keys and shapes exactly as in Dgcnn(size_latent).state_dict() / ckpt["encoder"] (AutoEncoder/trainers/encdec.py:299-305):
 * bn_1..bn_5.{weight,bias,running_mean,running_var,num_batches_tracked}, then conv_1..conv_5.weight */
int surfd_dgcnn_param_info(const surfd_dgcnn *d, int i, const char **key, int64_t shape[4], int *ndim);
/* fp32 device tensors; num_batches_tracked is accepted and ignored (dev_ptr may be NULL for it) */
int surfd_dgcnn_set_param(surfd_dgcnn *d, const char *key, const void *dev_ptr, const int64_t *shape, int ndim, surfd_stream s);
/* after the last set_param: folds BatchNorm (running statistics, eps 1e-5) into a per-channel scale / shift and forms the
 * factorised EdgeConv weights */
int surfd_dgcnn_finalize(surfd_dgcnn *d, surfd_stream s);
/* knn_points(x, x, K=k) (AutoEncoder/models/dgcnn.py:86): pts[B,N,3] -> dists[B,N,k] (squared, fp32; nullable) and idx[B,N,k] (int32), sorted
 * ascending, each point its own first neighbour, ties broken by the lower index.  N < k is SURFD_ERR_ARG. */
int surfd_dgcnn_knn(const surfd_dgcnn *d, const float *pts, int B, int N, float *dists, int32_t *idx, surfd_stream s);
/* Dgcnn.forward(x) (AutoEncoder/models/dgcnn.py:77-115): pts[B,N,3] -> feat[B,size_latent].  Clouds are independent: a cloud's latent has the
 * same bits whichever batch it is encoded in. */
int surfd_dgcnn_forward(surfd_dgcnn *d, const float *pts, int B, int N, float *feat, surfd_stream s);
/* the same, and (when x1234 is not NULL) the per-point features of the four EdgeConv blocks, torch.cat((x1, x2, x3, x4), -1)
 * [B,N,512] (AutoEncoder/models/dgcnn.py:88-100), the input of conv_5 (for tests and feature export) */
int surfd_dgcnn_forward_features(surfd_dgcnn *d, const float *pts, int B, int N, float *feat, float *x1234, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Mesh distance: the exact closest point of a triangle mesh for many query points.       */
/* Stands for open3d's RaycastingScene.compute_closest_points as AutoEncoder/utils.py:223-240 */
/* uses it (compute_udf_and_gradients, under compute_udf_from_mesh, utils.py:268-314, and */
/* AutoEncoder/encdec/preprocess_udfs.py:118-151).  Plain fp32; bitwise deterministic.    */
/* ------------------------------------------------------------------------------------ */
typedef struct surfd_mesh surfd_mesh;
#define SURFD_MESH_BRUTE_FORCE 1   /* flags bit 0: test every (query, triangle) pair, no culling */
/* vertices[V,3] fp32 and triangles[F,3] int32 on the device -> per-triangle records and per-tile bounding spheres (the inputs
 * are not referenced after the call).  F >= 1; every index must lie in [0, V): checked on the device and reported as
 * SURFD_ERR_ARG, never as a fault.  Degenerate triangles are legal and count as the segment or point they are; thin ones are
 * handled at full accuracy (the normals are formed in fp64 once per triangle).  host-sync. */
int surfd_mesh_create(const float *vertices, int V, const int32_t *triangles, int F, surfd_stream s, surfd_mesh **out);
void surfd_mesh_destroy(surfd_mesh *m);
int surfd_mesh_num_triangles(const surfd_mesh *m);
/* RaycastingScene.compute_closest_points as AutoEncoder/utils.py:228-234 calls it:
 * queries[Q,3] -> dist[Q] (fp32), closest[Q,3] (fp32, a point of triangle tri[q]), tri[Q] (int32, index into the triangles given
 * to create); any of the three may be NULL.  The winner of a query is the minimum under (squared distance, triangle index), so
 * its outputs do not depend on the other queries of the call, and the culled path equals SURFD_MESH_BRUTE_FORCE bit for bit.
 * Culling skips tiles of 32 consecutive triangles for waves of 64 consecutive queries; it only pays when both are spatially
 * coherent (e.g. sorted by Morton code, as the Python wrapper does).  skipped_tiles (nullable, int64 on the device) receives
 * the number of (wave, tile) visits the culled path skipped (waves of 64 consecutive queries, ceil(Q / 64) of them).  Q = 0 is a
 * no-op.  The handle keeps the call's partial results in a workspace of its own (grown on demand, which syncs the stream): a
 * handle serves one stream and one host thread at a time; use one handle per stream for concurrent calls. */
int surfd_mesh_closest(const surfd_mesh *m, const float *queries, int Q, int flags, float *dist, float *closest, int32_t *tri,
                       int64_t *skipped_tiles, surfd_stream s);

/* no reference counterpart; an opt-in hierarchy of boxes over the handle's triangles:
 * csrc/meshbvh.hip (63-bit Morton codes of the centroids, a stable radix sort, leaves of 4 triangles, an implicit 4-ary tree
 * without pointers), built on the device from the records the handle holds.  Idempotent.  host-sync. */
int surfd_mesh_build_bvh(surfd_mesh *m, surfd_stream s);
#define SURFD_MESH_COUNT_VISITS 2  /* flags bit 1 of surfd_mesh_closest_bvh: count box tests and pair tests (surfd_mesh_visits) */
/* RaycastingScene.compute_closest_points (utils.py:228-234) through the hierarchy:
 * surfd_mesh_closest with every query walking the tree on its own instead of the tiles; the same arguments, the same outputs bit
 * for bit (the hierarchy decides which pairs are tested, never a pair's result or the order that picks the winner).  flags:
 * SURFD_MESH_BRUTE_FORCE wins and is surfd_mesh_closest's brute-force path; SURFD_MESH_COUNT_VISITS.  Without
 * surfd_mesh_build_bvh: SURFD_ERR_STATE, never a fallback.  skipped_tiles (nullable) is set to 0: there are no tiles. */
int surfd_mesh_closest_bvh(const surfd_mesh *m, const float *queries, int Q, int flags, float *dist, float *closest, int32_t *tri,
                           int64_t *skipped_tiles, surfd_stream s);
/* no reference counterpart; a measurement of the hierarchy:
 * the box tests and pair tests, summed over the lanes, of the last call with SURFD_MESH_COUNT_VISITS, to host memory.
 * host-sync.  Measurement only. */
int surfd_mesh_visits(const surfd_mesh *m, int64_t *box_tests, int64_t *pair_tests, surfd_stream s);
/* no reference counterpart; the hierarchy's shape, for tests:
 * the number of levels, leaves and nodes, and the first min(capacity, levels) level sizes, level 0 (the nodes above the leaves)
 * first; any pointer may be NULL.  SURFD_ERR_STATE without a build. */
int surfd_mesh_bvh_info(const surfd_mesh *m, int *levels, int *leaves, int *nodes, int32_t *level_sizes, int capacity);
/* no reference counterpart; the hierarchy's content, for tests:
 * boxes[nodes,6,4] fp32 (lo.x, lo.y, lo.z, hi.x, hi.y, hi.z of a node's 4 children; an absent child is lo = +inf, hi = -inf;
 * level k starts at the sum of the sizes below it) and leaf_triangles[leaves,4] int32 (indices into the triangles given to
 * create, -1 past the end) are copied to the caller's buffers (device or host; either may be NULL).  host-sync. */
int surfd_mesh_bvh_read(const surfd_mesh *m, float *boxes, int32_t *leaf_triangles, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Ray casting on a mesh: first hit per ray and the number of triangles a ray meets.      */
/* Stands for the ray half of open3d's RaycastingScene (cast_rays, count_intersections)   */
/* and, through the crossing count, for compute_signed_distance as AutoEncoder/utils.py:242-264 */
/* calls it (compute_sdf_and_gradients, under compute_sdf_from_mesh, utils.py:317-363).   */
/* fp32 in, fp64 pair arithmetic; bitwise deterministic.                                  */
/* ------------------------------------------------------------------------------------ */
typedef struct surfd_rayscene surfd_rayscene;
#define SURFD_RAY_BRUTE_FORCE 1     /* flags bit 0: test every (ray, triangle) pair, no culling */
#define SURFD_RAY_COUNT_SKIPPED 2   /* flags bit 1: count the (wave, tile) visits that culling skips (surfd_rayscene_skipped) */
#define SURFD_RAY_BVH 4             /* flags bit 2: walk the hierarchy of surfd_rayscene_build_bvh instead of the tiles */
#define SURFD_RAY_COUNT_VISITS 8    /* flags bit 3: with SURFD_RAY_BVH, count box tests and pair tests (surfd_rayscene_visits) */
/* vertices[V,3] fp32 and triangles[F,3] int32 on the device -> the triangles' corners and per-tile bounding spheres (the
 * inputs are not referenced after the call).  F >= 1; every index must lie in [0, V): checked on the device and reported as
 * SURFD_ERR_ARG, never as a fault.  Degenerate triangles are legal and are never hit.  host-sync. */
int surfd_rayscene_create(const float *vertices, int V, const int32_t *triangles, int F, surfd_stream s, surfd_rayscene **out);
void surfd_rayscene_destroy(surfd_rayscene *m);
int surfd_rayscene_num_triangles(const surfd_rayscene *m);
/* no reference counterpart; open3d's RaycastingScene.cast_rays, of which the reference uses the distance queries only:
 * rays[R,6] (origin, direction; the direction need not have unit length and t counts in units of it) -> per ray the first triangle met with tmin <= t < tmax: t[R] (fp32), tri[R] (int32, index into the triangles given to
 * create), uv[R,2] (the weights of the triangle's second and third corner at the hit), normal[R,3] (the triangle's unit normal
 * by its winding, not turned towards the ray); any of the four may be NULL.  A miss is t = +inf, tri = -1, uv = normal = 0, and
 * so is a ray with a NaN, an Inf or a zero direction.  The pair test is the shear-and-scale form of Woop, Benthin and Wald in
 * fp64, two-sided, with the top-left rule on edges that a ray meets exactly: every operation and its order are fixed (header of
 * csrc/raycast.hip) and the numpy restatement tests/raycast_ref.py gives the same bits.  The winner is the minimum under (bits
 * of t, triangle index), so a ray's outputs do not depend on the other rays of the call, on the order of the triangles other
 * than through that index, or on culling: the culled path equals SURFD_RAY_BRUTE_FORCE bit for bit.  Culling skips tiles of 32
 * consecutive triangles for waves of 64 consecutive rays; it pays when both are spatially coherent (the Python wrapper sorts
 * both by Morton code).  tmin must be finite and >= 0, tmax must not be a NaN (SURFD_ERR_ARG).  R = 0 is a no-op.  The handle
 * keeps the call's partial results in a workspace of its own (grown on demand, which syncs the stream): a handle serves one
 * stream and one host thread at a time. */
int surfd_rayscene_cast(surfd_rayscene *m, const float *rays, int R, float tmin, float tmax, int flags, float *t, int32_t *tri,
                        float *uv, float *normal, surfd_stream s);
/* RaycastingScene.count_intersections, whose parity is the sign of compute_signed_distance at AutoEncoder/utils.py:251:
 * count[R] (int32) = the number of triangles the ray meets with tmin <= t < tmax under
 * the same pair test.  A ray through an edge shared by two triangles, or through a vertex, is counted once where the surface
 * crosses it and 0 or 2 times where the surface folds back, so the parity of the count from a point tells inside from outside
 * on a closed mesh. */
int surfd_rayscene_count(surfd_rayscene *m, const float *rays, int R, float tmin, float tmax, int flags, int32_t *count,
                         surfd_stream s);
/* no reference counterpart; a measurement of the culling:
 * the number of (wave, tile) visits the last call with SURFD_RAY_COUNT_SKIPPED skipped, and how many it had in all (waves of 64
 * consecutive rays, tiles of 32 consecutive triangles), to host memory.  host-sync.  Measurement only. */
int surfd_rayscene_skipped(surfd_rayscene *m, int64_t *skipped, int64_t *total, surfd_stream s);

/* no reference counterpart; an opt-in hierarchy of boxes over the handle's triangles:
 * the same as surfd_mesh_build_bvh's.  Idempotent.  host-sync.  Afterwards SURFD_RAY_BVH on surfd_rayscene_cast / _count makes every ray walk the tree on its own instead of the
 * tiles: the same outputs bit for bit.  SURFD_RAY_BVH without a build is SURFD_ERR_STATE, never a fallback;
 * SURFD_RAY_BRUTE_FORCE wins over it. */
int surfd_rayscene_build_bvh(surfd_rayscene *m, surfd_stream s);
/* no reference counterpart; a measurement of the hierarchy:
 * the box tests and pair tests, summed over the lanes, of the last call with SURFD_RAY_COUNT_VISITS, to host memory.
 * host-sync.  Measurement only. */
int surfd_rayscene_visits(surfd_rayscene *m, int64_t *box_tests, int64_t *pair_tests, surfd_stream s);
/* no reference counterpart; the hierarchy's shape, for tests:
 * as surfd_mesh_bvh_info */
int surfd_rayscene_bvh_info(const surfd_rayscene *m, int *levels, int *leaves, int *nodes, int32_t *level_sizes, int capacity);
/* no reference counterpart; the hierarchy's content, for tests:
 * as surfd_mesh_bvh_read */
int surfd_rayscene_bvh_read(const surfd_rayscene *m, float *boxes, int32_t *leaf_triangles, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Intersection tests between triangles: the self-intersections of one mesh and the       */
/* collisions of two.  No reference counterpart (the reference ships no evaluation code): */
/* the share of self-intersecting faces is the number that work on meshing unsigned       */
/* distance fields reports next to the Chamfer distance.  One fp32 snap per vertex, then  */
/* int64 on int32 differences: exact, no epsilon; results do not depend on any order.     */
/* ------------------------------------------------------------------------------------ */
typedef struct surfd_isect surfd_isect;
#define SURFD_ISECT_BRUTE_FORCE 1     /* flags bit 0: evaluate every pair, no culling */
#define SURFD_ISECT_COUNT_SKIPPED 2   /* flags bit 1: count the (wave, tile) visits that culling skips (surfd_isect_skipped) */
/* no reference counterpart; the snapped triangles of one mesh and their exact integer boxes:
 * vertices[V,3] fp32 and triangles[F,3] int32 on the device (not referenced after the call).  Every coordinate is snapped to
 * q = rint(x * 2^lattice_log2) in fp32; meshes that are to be compared need the same lattice_log2.  F >= 1, V >= 1,
 * |lattice_log2| <= 100.  A vertex with a NaN or with |q| > 2^19 is SURFD_ERR_ARG with the number of such vertices in the text;
 * so is an index outside [0, V), checked on the device and never reported as a fault.  Two vertices with equal snapped
 * coordinates are the same point whatever their indices, so an unwelded mesh behaves as the welded one.  A triangle whose
 * normal is (0, 0, 0) after the snap is degenerate: it is flagged and intersects nothing.  host-sync. */
int surfd_isect_create(const float *vertices, int V, const int32_t *triangles, int F, int lattice_log2, surfd_stream s, surfd_isect **out);
void surfd_isect_destroy(surfd_isect *m);
int surfd_isect_num_triangles(const surfd_isect *m);
/* no reference counterpart; the triangles without area after the snap:
 * flags[F] (uint8, 1 = degenerate) and count (one int64), both on the device, either may be NULL. */
int surfd_isect_degenerate(surfd_isect *m, uint8_t *flags, int64_t *count, surfd_stream s);
/* no reference counterpart; the pairs of triangles of one mesh that have a common point beyond what neighbours share:
 * the pair test is stated in the header of csrc/meshintersect.hip and restated in tests/meshintersect_ref.py.  Closed triangles:
 * touching counts.  Two triangles that share one point intersect when they have another common point (a T-junction counts),
 * two that share an edge only when they are folded flat onto each other, two that share all three points always (duplicates).
 * hits[F] (int32, zeroed by the call): the number of found pairs each triangle belongs to.  count (one int64): the pairs found.
 * pairs[capacity] (int64): the keys i << 32 | j, i < j, of the first pairs to claim a slot, in no specified order; count keeps
 * counting beyond capacity.  All three are device pointers and may be NULL; capacity 0 with pairs NULL is the counting form,
 * capacity > 0 with pairs NULL is SURFD_ERR_ARG.  Indices are those of the triangles given to create.  hits, count and the set of
 * pairs do not depend on the order of the triangles (after mapping back), on the launch geometry or on culling: the culled
 * path equals SURFD_ISECT_BRUTE_FORCE.  Culling works on tiles of 32 and chunks of 256 consecutive triangles; it pays when
 * these are spatially compact (the Python wrapper sorts by Morton code).  No host sync. */
int surfd_isect_self(surfd_isect *m, int flags, int32_t *hits, int64_t *pairs, int64_t capacity, int64_t *count, surfd_stream s);
/* no reference counterpart; the pairs (triangle of a, triangle of b) that have a common point:
 * the closed test on every pair, no sharing rule (a vertex of a lying exactly on b counts).  hits_a[Fa], hits_b[Fb], pairs (keys
 * i_a << 32 | j_b), capacity and count as above.  Handles with different lattice_log2, and a == b, are SURFD_ERR_ARG. */
int surfd_isect_between(surfd_isect *a, surfd_isect *b, int flags, int32_t *hits_a, int32_t *hits_b, int64_t *pairs, int64_t capacity,
                        int64_t *count, surfd_stream s);
/* no reference counterpart; a measurement of the culling:
 * the number of (wave, tile) visits the last call on m (the first handle of a _between) with SURFD_ISECT_COUNT_SKIPPED skipped,
 * and how many the brute-force path has (waves of 64 consecutive triangles, tiles of 32 partners), to host memory.  host-sync. */
int surfd_isect_skipped(surfd_isect *m, int64_t *skipped, int64_t *total, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Generalized winding numbers of a mesh (Jacobson et al. 2013; libigl's winding_number): */
/* the signed solid angle of the mesh seen from a point, over 4 pi.  1 inside and 0       */
/* outside a closed, consistently oriented mesh, and a hole costs only its own solid      */
/* angle, where the crossing parity above flips a whole cone.  No reference counterpart   */
/* (the reference takes its signs from open3d's parity).  fp32 in, fp64 arithmetic; the   */
/* bits of a query's value are a function of the query and the triangle list alone.       */
/* ------------------------------------------------------------------------------------ */
typedef struct surfd_winding surfd_winding;
#define SURFD_WINDING_ONE_SPLIT 1   /* flags bit 0: one workgroup walks the whole triangle range (a test switch; the same bits) */
/* no reference counterpart; the corners of a mesh's triangles, kept for repeated winding-number calls:
 * vertices[V,3] fp32 and triangles[F,3] int32 on the device (not referenced after the call); nine fp32 per triangle are kept
 * in the order given, nothing is sorted.  F >= 1, V >= 1, 3 F < 2^31.  A vertex that holds a NaN or an Inf is SURFD_ERR_ARG with
 * the number of such vertices in the text; so is an index outside [0, V), checked on the device and never reported as a fault.
 * Triangles without area are legal and contribute 0.  host-sync. */
int surfd_winding_create(const float *vertices, int V, const int32_t *triangles, int F, surfd_stream s, surfd_winding **out);
void surfd_winding_destroy(surfd_winding *m);
int surfd_winding_num_triangles(const surfd_winding *m);
/* no reference counterpart; libigl's winding_number(V, F, O):
 * points[Q,3] fp32 -> w[Q] fp64, both on the device.  Per triangle theta = atan2(det, den) by van Oosterom and Strackee's formula
 * in fp64, 0 where det == 0 (a point in the triangle's plane or on a vertex, a triangle without area); w = (sum of theta) / (2 pi).
 * Every operation and the association of the sum (chunks of 256 triangles, groups of 16 chunks, then the groups, each left to
 * right in the caller's order) are fixed in the header of csrc/winding.hip and restated in tests/winding_ref.py: the bits of
 * w[n] do not depend on Q, on the other points of the call, on n or on the launch geometry, and differ from the restatement only
 * through atan2 (|w - w_ref| <= F 2^-50).  w depends on the orientation: a wholly inverted mesh gives -w, one whose faces are not
 * consistently oriented gives values that mean nothing.  A point that holds a NaN or an Inf gets w = NaN.  0 <= Q < 2^31; Q = 0 is
 * a no-op.  The handle keeps the call's partial sums in a workspace of its own (at most 256 MiB; the points are walked in slabs):
 * a handle serves one stream and one host thread at a time. */
int surfd_winding_eval(surfd_winding *m, const float *points, int64_t Q, int flags, double *w, surfd_stream s);
#define SURFD_WINDING_COUNT_VISITS 2   /* flags bit 1 of surfd_winding_eval_fast: count cluster and triangle terms (surfd_winding_visits) */
/* no reference counterpart; the tree of Barill et al.'s fast winding numbers (libigl's fast_winding_number precomputation), dipole only:
 * the box hierarchy of csrc/meshbvh.hip over the handle's triangles (as surfd_rayscene_build_bvh), and for every child slot
 * of every node a record of seven doubles: the area-weighted centre p of what the child holds, its vector area N and the squared
 * distance R2 from p to the farthest corner of the child's box.  The sums behind the records are hierarchical and fixed in the
 * header of csrc/winding.hip; tests/winding_fast_ref.py gives the same bits.  The handle's triangle records and their order do
 * not change.  Idempotent.  host-sync. */
int surfd_winding_build_bvh(surfd_winding *m, surfd_stream s);
/* no reference counterpart; libigl's fast_winding_number(..., beta) with expansion order 0 (the dipole):
 * AN APPROXIMATION of surfd_winding_eval whose cost per point is logarithmic in F: points[Q,3] fp32 -> w[Q] fp64, both on the
 * device.  Every point walks the tree on its own; a child whose centre is farther than beta times its radius (d2 > beta^2 R2)
 * contributes ((N . r) / (d2 sqrt(d2))) / 2 with r = p - point and is not entered, every other leaf contributes the exact terms
 * of its triangles; w = (the sum in walk order) / (2 pi).  beta: a finite number >= 1 or +inf (every triangle exactly, in the
 * tree's order); anything else is SURFD_ERR_ARG.  The bits of w[n] depend on the point, the mesh and beta alone, and differ from
 * the restatement only through the exact terms' atan2 (|w - w_ref| <= max(T, 1) 2^-50, T the point's number of terms).  Measured
 * error against surfd_winding_eval: DESIGN.md section 8.16.  flags: SURFD_WINDING_COUNT_VISITS.  A point that holds a NaN or an
 * Inf gets w = NaN.  0 <= Q < 2^31; Q = 0 is a no-op.  Without surfd_winding_build_bvh: SURFD_ERR_STATE, never a fallback.
 * Does not sync and keeps nothing in the handle's workspace. */
int surfd_winding_eval_fast(surfd_winding *m, const float *points, int64_t Q, double beta, int flags, double *w, surfd_stream s);
/* no reference counterpart; a measurement of the fast path:
 * the cluster terms and triangle terms, summed over the points, of the last surfd_winding_eval_fast with
 * SURFD_WINDING_COUNT_VISITS, to host memory.  host-sync.  Measurement only. */
int surfd_winding_visits(surfd_winding *m, int64_t *cluster_terms, int64_t *triangle_terms, surfd_stream s);
/* no reference counterpart; the hierarchy's shape, for tests:
 * as surfd_mesh_bvh_info */
int surfd_winding_bvh_info(const surfd_winding *m, int *levels, int *leaves, int *nodes, int32_t *level_sizes, int capacity);
/* no reference counterpart; the hierarchy's content, for tests:
 * as surfd_mesh_bvh_read, and records[nodes,4,7] fp64 (nullable): (p.x, p.y, p.z, N.x, N.y, N.z, R2) of every child slot,
 * (0, 0, 0, 0, 0, 0, -1) for a slot that holds nothing */
int surfd_winding_bvh_read(const surfd_winding *m, float *boxes, int32_t *leaf_triangles, double *records, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Mesh topology: edges and their valences, face neighbours, connected components,        */
/* border loops, a consistent orientation of every manifold patch, exact welding.  No     */
/* reference counterpart (the reference leaves these to trimesh / pymeshlab on the host). */
/* Integer work on the index array; every output is a function of the input alone, not    */
/* of launch geometry or of the order in which atomics arrive (csrc/meshtopo.hip states   */
/* the contract and why its lock-free union-find terminates; the tests restate the        */
/* contract sequentially in numpy).                                                       */
/* ------------------------------------------------------------------------------------ */
typedef struct surfd_meshtopo surfd_meshtopo;
#define SURFD_MESHTOPO_VERTEX 0     /* connectivity: faces that share a vertex */
#define SURFD_MESHTOPO_EDGE 1       /* connectivity: faces that share an edge of any valence */
#define SURFD_MESHTOPO_MANIFOLD 2   /* connectivity: faces that share an edge of valence 2 */
/* no reference counterpart; trimesh's edges_unique / face_adjacency, built once and kept:
 * triangles[F,3] int32 on the device (copied; not referenced after the call), V the number of vertices they may name.  Half-edge
 * h = 3 f + c runs from t[f, c] to t[f, (c + 1) % 3]; a face with two equal indices is degenerate and takes part in nothing.
 * One 64-bit key lo << 32 | hi per half-edge, a stable radix sort, run lengths: the edges in ascending (lo, hi) order.
 * F >= 0 (F = 0 gives empty outputs), V >= 0, 3 F < 2^31; an index outside [0, V) is SURFD_ERR_ARG with the first such face in
 * the text, checked on the device and never reported as a fault.  Allocates every workspace the calls below use.  host-sync
 * (the number of edges is read back). */
int surfd_meshtopo_create(const int32_t *triangles, int F, int V, surfd_stream s, surfd_meshtopo **out);
void surfd_meshtopo_destroy(surfd_meshtopo *m);
/* no reference counterpart; the sizes the arrays of surfd_meshtopo_read have:
 * faces F, edges E, degenerate faces, and the vertices that a non-degenerate face names; each nullable, host memory. */
int surfd_meshtopo_counts(const surfd_meshtopo *m, int64_t *faces, int64_t *edges, int64_t *degenerate, int64_t *referenced);
/* no reference counterpart; trimesh's edges_unique, edges_unique_inverse, face_adjacency:
 * device arrays, each nullable: edges[E,2] (lo, hi), valence[E], edge_offsets[E+1] and edge_halfedges[3 (F - degenerate)] (the
 * half-edges of edge e, ascending), face_edges[F,3] (the edge of half-edge 3 f + c; -1 in a degenerate face),
 * face_neighbors[F,3] (the other face across a valence-2 edge, -1 across a border edge and in a degenerate face, -2 across an
 * edge of valence >= 3), degenerate[F] (bytes 0 / 1).  Copies on the stream; does not sync. */
int surfd_meshtopo_read(const surfd_meshtopo *m, int32_t *edges, int32_t *valence, int32_t *edge_offsets, int32_t *edge_halfedges,
                        int32_t *face_edges, int32_t *face_neighbors, unsigned char *degenerate, surfd_stream s);
/* no reference counterpart; trimesh's Trimesh.split / graph.connected_components over face adjacency:
 * labels[F] int32 on the device: the components under the given connectivity, numbered in ascending order of their lowest
 * face; -1 for a degenerate face.  count (host) = the number of components.  A lock-free union-find over an explicit pair list:
 * the larger root is hooked under the smaller, so a component's root is its smallest node whatever the schedule.  host-sync
 * (count is read back).  A handle serves one stream and one host thread at a time (the workspaces are the handle's). */
int surfd_meshtopo_components(surfd_meshtopo *m, int connectivity, int32_t *labels, int64_t *count, surfd_stream s);
/* no reference counterpart; trimesh's Trimesh.outline / pymeshlab's border loops:
 * labels[E] int32 on the device: for every border edge (valence 1) the loop it lies on, loops being the components of the
 * border edges under "share a vertex", numbered in ascending order of their lowest edge; -1 for every other edge.
 * irregular[E] (bytes, nullable): 1 for a border edge with an end point that lies on a number of border edges other than two;
 * a loop is simple when none of its edges is irregular.  count (host) = the number of loops.  host-sync. */
int surfd_meshtopo_border_loops(surfd_meshtopo *m, int32_t *labels, unsigned char *irregular, int64_t *count, surfd_stream s);
/* no reference counterpart; trimesh's repair.fix_normals (fix_winding, then fix_inversion per body):
 * flip[F] (bytes): the one assignment under which the two half-edges of every valence-2 edge run in opposite directions and
 * the lowest face of every manifold component (patch) keeps its winding; 0 throughout a patch that has no such assignment
 * and in degenerate faces.  orientable[F] (bytes, nullable): 0 for the faces of a patch without one.  patch_face[F] (int32,
 * nullable): the lowest face of the face's patch, -1 in a degenerate face.  Components of the double cover (2 F nodes), one run
 * of the union-find however long the patch's diameter.  vertices[V,3] fp32 on the device or NULL; where given, every orientable
 * patch all of whose edges have valence 2 is then turned as a whole so that its signed volume is positive: the volume is the
 * integer sum of llrint(det(v0, v1, v2) 2^30 / M^3), M the power of two >= max |coordinate|, so it has no order of addition; 0
 * leaves the patch.  Patch by patch, no nesting analysis (the shell of a cavity ends up outward too).  Does not sync. */
int surfd_meshtopo_orient(surfd_meshtopo *m, const float *vertices, unsigned char *flip, unsigned char *orientable, int32_t *patch_face,
                          surfd_stream s);
/* no reference counterpart; trimesh's merge_vertices(merge_tex=True, digits_vertex=None), without its rounding:
 * vertices[V,3] fp32 on the device -> vertex_map[V] int32 (the index of every vertex's survivor AFTER compaction) and
 * survivor[V] (bytes: 1 where the vertex stays).  Vertices with equal coordinates become one (-0 == +0; a vertex that holds a NaN
 * equals nothing, itself included); the survivor is the lowest index of its class, survivors keep their order.  No tolerance.
 * count (host) = the number of survivors.  3 V < 2^31.  host-sync. */
int surfd_meshtopo_weld(const float *vertices, int V, int32_t *vertex_map, unsigned char *survivor, int64_t *count, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Mesh smoothing and vertex normals: the vertex-moving steps between the mesh stages.    */
/* Stands for MeshLab's apply_coord_laplacian_smoothing (sample/generate_uncond.py), the   */
/* border smoothing loop of meshudf.py and trimesh's weighted_vertex_normals, which the    */
/* reference runs on the host.  fp64 on the caller's positions, + - * / sqrt (and one      */
/* acos in the angle-weighted normals), no atomics: every output is a function of the      */
/* input alone, and the order of summation per vertex is fixed (csrc/meshsmooth.hip        */
/* states it; tests/meshsmooth_ref.py restates it sequentially in numpy).                  */
/* ------------------------------------------------------------------------------------ */
typedef struct surfd_meshsmooth surfd_meshsmooth;
#define SURFD_MESHSMOOTH_F32 0      /* dtype of the positions given: float */
#define SURFD_MESHSMOOTH_F64 1      /* double */
#define SURFD_MESHSMOOTH_ALL 0      /* umbrella set: every half-edge at the vertex */
#define SURFD_MESHSMOOTH_BORDER 1   /* umbrella set: the border neighbours only; other vertices stay */
#define SURFD_MESHSMOOTH_ANGLE 0    /* normals: unit face normals weighted by the corner angle */
#define SURFD_MESHSMOOTH_AREA 1     /* normals: the unnormalised cross products */
/* no reference counterpart; the neighbourhoods of one connectivity, built once and kept:
 * triangles[F,3] int32 on the device (copied), V the number of vertices they may name.  Half-edge h = 3 f + c runs from t[f, c]
 * to t[f, (c + 1) % 3]; it is a border half-edge iff its unordered vertex pair occurs exactly once among all 3 F half-edges
 * (faces with repeated indices take part: meshproc.border_edge_rows, not the classification of surfd_meshtopo).  Stable radix
 * sorts give, per vertex, the half-edges that leave it and that arrive at it (ascending in h), its border neighbours and its
 * corners (ascending in (c, f)).  F >= 0, V >= 0, 3 F < 2^31; an index outside [0, V) is SURFD_ERR_ARG, found on the device
 * before anything is indexed by it, never a fault.  host-sync (the flag and the two border counts are read back). */
int surfd_meshsmooth_create(const int32_t *triangles, int F, int V, surfd_stream s, surfd_meshsmooth **out);
void surfd_meshsmooth_destroy(surfd_meshsmooth *m);
/* no reference counterpart; what create found, each nullable, host memory: F, V, the border half-edges, the vertices on them. */
int surfd_meshsmooth_counts(const surfd_meshsmooth *m, int64_t *faces, int64_t *vertices, int64_t *border_halfedges, int64_t *border_vertices);
/* pymeshlab's apply_coord_laplacian_smoothing(stepsmoothnum, boundary, cotangentweight) as meshproc.laplacian_smooth restates it:
 * vertices[V,3] on the device, fp32 or fp64 by dtype, -> out[V,3] fp64 (out may be the fp64 input itself; otherwise they must
 * not overlap).  `steps` Jacobi sweeps, one launch each: an inner vertex moves to (p + sum w_h p_h) / (1 + sum w_h) over the
 * half-edges that leave it, then those that arrive, w_h = the cotangent of the angle opposite h (1 without `cotangent`; 0 where
 * the triangle has no area); with `boundary` a vertex on a border half-edge is averaged with itself and its neighbours along
 * the border only.  A vertex whose weights sum to <= 0 stays.  steps = 0 and F = 0 copy the input.  Does not sync; one stream at a time per handle (the position buffers are the handle's). */
int surfd_meshsmooth_laplacian(surfd_meshsmooth *m, const void *vertices, int dtype, int steps, int cotangent, int boundary, double *out,
                               surfd_stream s);
/* the border smoothing loop of meshudf.py (set = BORDER; meshproc.smooth_borders) and Taubin's lambda | mu smoothing (set = ALL):
 * `sweeps` Jacobi sweeps p <- p + k (mean of the neighbours - p), k = k0 in sweeps 0, 2, ... and k1 in sweeps 1, 3, ...; the
 * neighbours are the other ends of every half-edge at the vertex (ALL: leaving, then arriving, a neighbour once per half-edge) or
 * of its border half-edges (BORDER: those above the vertex ascending, then those below); a vertex without neighbours stays.
 * Buffers, dtype and stream as for surfd_meshsmooth_laplacian.  Does not sync. */
int surfd_meshsmooth_umbrella(surfd_meshsmooth *m, const void *vertices, int dtype, double k0, double k1, int sweeps, int set, double *out,
                              surfd_stream s);
/* trimesh's geometry.weighted_vertex_normals (ANGLE; meshproc.vertex_normals_by_angle) and mean_vertex_normals by area (AREA):
 * unit[V,3] and raw[V,3] fp64 on the device, each nullable: raw = the sum over the vertex's corners, in (c, f) order, of the unit
 * face normal times the corner angle (ANGLE) or of the face's cross product (AREA); unit = raw / |raw|, 0 where that is 0.
 * Neither may overlap the positions.  Does not sync. */
int surfd_meshsmooth_vertex_normals(surfd_meshsmooth *m, const void *vertices, int dtype, int weight, double *unit, double *raw, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Mesh cleaning: merge coincident vertices, drop duplicate and flat faces, close holes   */
/* of 3 and 4 edges.  Stands for the trimesh calls of meshudf.py's cleaning loop          */
/* (process, remove_duplicate_faces, remove_degenerate_faces, fill_holes), which the      */
/* reference runs on the host; surfd_amd/meshproc.py restates them in numpy and IS the    */
/* contract: every output equals meshproc's bit for bit and in the same order.  Integer   */
/* sorts and scans plus fp64 + - * / sqrt and one round-to-nearest-even; no result        */
/* depends on launch geometry or on the order in which atomics arrive (csrc/meshclean.hip */
/* states the contract and the passes; tests/meshclean_ref.py restates it sequentially).  */
/* Stateless calls: temporaries live for the call, nothing is kept.  Vertices fp64 [V,3], */
/* faces int32 [F,3], on the device; F >= 0, V >= 0, 3 F < 2^31.  An index outside [0, V) */
/* is SURFD_ERR_ARG: the kernels compare every caller index before they index by it, and  */
/* the flag is read back at the end of the call; never a fault.  EVERY CALL HOST-SYNCS    */
/* ONCE, at its end (its counts and flags are read back on the caller's stream).          */
/* ------------------------------------------------------------------------------------ */
/* meshudf.py's Trimesh(..., process=True, validate=False) as meshproc.cull_and_merge restates it:
 * faces that name a non-finite vertex go; the vertices the other faces name take the key (rint(x scale), rint(y scale),
 * rint(z scale)) as three int64 (ties to even; -0.0 and 0.0 share a key; scale = 1 / tolerance, worked out by the caller) and
 * vertices with equal keys become one: the lowest index of a class stays with its own bits, survivors keep their order, faces
 * keep theirs and are re-indexed.  out_vertices[V,3] and out_faces[F,3] must hold the whole input; counts[5] (host): vertices
 * and faces written, non-finite vertices, finite vertices no remaining face names, vertices merged into a lower one.  F = 0 or
 * V = 0 write nothing.  A finite coordinate with |x scale| >= 2^62 is SURFD_ERR_ARG (beyond the keys; never wrapped).  host-sync. */
int surfd_meshclean_cull_and_merge(const double *vertices, int V, const int32_t *faces, int F, double scale, double *out_vertices,
                                   int32_t *out_faces, int64_t *counts, surfd_stream s);
/* meshudf.py's remove_duplicate_faces as meshproc.drop_duplicate_faces restates it:
 * one face per set of three indices (winding and rotation ignored): the lowest face of each class with its own winding, WRITTEN
 * IN ASCENDING ORDER of (largest, middle, smallest index) whether or not a face goes.  out_faces[F,3]; count (host) = the faces
 * written.  Two stable radix sorts (31 and 63 bits); a negative index is SURFD_ERR_ARG.  host-sync. */
int surfd_meshclean_drop_duplicate_faces(const int32_t *faces, int F, int32_t *out_faces, int64_t *count, surfd_stream s);
/* meshudf.py's remove_degenerate_faces as meshproc.drop_degenerate_faces restates it:
 * keeps, in their order, the faces whose two heights 2 area / |edge| over the edges that leave corner 0 both exceed `height` (a
 * height over an edge no longer than 1e-8 counts as 0; a NaN fails); fp64 in the operation order csrc/meshclean.hip states.
 * out_faces[F,3]; count (host) = the faces written.  host-sync. */
int surfd_meshclean_drop_degenerate_faces(const double *vertices, int V, const int32_t *faces, int F, double height, int32_t *out_faces,
                                          int64_t *count, surfd_stream s);
/* meshudf.py's fill_holes as meshproc.fill_small_holes restates it:
 * a border half-edge is one whose unordered vertex pair occurs once among all 3 F half-edges; a loop of exactly 3 or 4 of them
 * through vertices that one border half-edge leaves is closed against its direction (4 edges: two triangles).  Only the caps are
 * written, caps[cap_rows,3] with cap_rows >= min(V, 3 F / 2), in ascending order of their smallest vertex: the caller appends
 * them to its faces.  counts[3] (host): caps written, loops of 3 edges, loops of 4.  F < 3 writes nothing.  host-sync. */
int surfd_meshclean_fill_small_holes(const int32_t *faces, int F, int V, int32_t *caps, int64_t cap_rows, int64_t *counts, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Hole filling: every border loop of up to max_edges edges is closed by its             */
/* minimum-total-area triangulation (Barequet and Sharir 1995; no reference counterpart:  */
/* the reference and trimesh close loops of 3 and 4 edges only, which is                  */
/* surfd_meshclean_fill_small_holes).  tests/meshfill_ref.py restates the contract        */
/* sequentially in numpy, csrc/meshfill.hip carries its text and the passes; the caps,    */
/* their order, cap_loop and every count equal the restatement bit for bit.  Vertices     */
/* fp64 [V,3], faces int32 [F,3], on the device; F >= 0, V >= 0, 3 F < 2^31.  An index    */
/* outside [0, V) is SURFD_ERR_ARG, found on the device before anything is indexed by it. */
/* fp64 + - * sqrt, integer sorts and scans; no float atomics, no result depends on the   */
/* launch geometry.  One stream at a time per handle.                                     */
/* ------------------------------------------------------------------------------------ */
/* no reference counterpart; the plan of the hole filling (tests/meshfill_ref.py, loops):
 * border half-edges as surfd_meshclean_fill_small_holes; a loop is a cycle of n >= 3 vertices that exactly one border half-edge
 * leaves and exactly one enters, listed from its smallest vertex, numbered in ascending order of that vertex.  Finds the loops,
 * bins those with n <= max_edges (3 .. 1024) by length and copies their points into the handle (the vertex array may go after
 * the call).  counts[7] (host): loops_filled, caps, loops_too_long (n > max_edges), loops_nonfinite (0 here), irregular_border_edges
 * (border half-edges on no loop), border_edges, longest_filled; caps is exact unless a loop turns out non-finite in run.  F = 0
 * or V = 0 give an empty plan.  On a refusal *out stays null.  host-sync (one read). */
typedef struct surfd_meshfill surfd_meshfill;
int surfd_meshfill_plan(const double *vertices, int V, const int32_t *faces, int F, int max_edges, int64_t *counts, surfd_stream s,
                        surfd_meshfill **out);
/* no reference counterpart; the lengths of the hole filling's loops (tests/meshfill_ref.py, hole_sizes):
 * sizes[rows] int32 on the device, rows >= loops_filled + loops_too_long of the plan: the length of every loop in loop order, the
 * too long ones included.  Device to device on the stream; no sync. */
int surfd_meshfill_loop_sizes(const surfd_meshfill *m, int32_t *sizes, int64_t rows, surfd_stream s);
/* no reference counterpart; the triangulation and the caps of the hole filling (tests/meshfill_ref.py, fill_holes):
 * per planned loop the table W[i][j] = min over k of (W[i][k] + W[k][j]) + area(i, k, j) over the reversed listing of its border, the
 * least (sum, k) winning (a number before a NaN); n - 2 rows per loop in preorder of the recursion, loops in ascending number,
 * written to caps[cap_rows,3] with cap_rows >= the planned caps; cap_loop[cap_rows] (nullable): the loop number of every row.  A
 * loop whose total is not finite stays open.  counts[7] (host) as in plan, final.  The handle stays usable.  host-sync (one read;
 * none where nothing was planned). */
int surfd_meshfill_run(surfd_meshfill *m, int32_t *caps, int64_t cap_rows, int32_t *cap_loop, int64_t *counts, surfd_stream s);
void surfd_meshfill_destroy(surfd_meshfill *m);

/* ------------------------------------------------------------------------------------ */
/* Mesh simplification: vertex clustering on a uniform grid with one representative per  */
/* occupied cell (no reference counterpart: the reference writes its meshes at the full   */
/* resolution of the grid).  tests/meshsimplify_ref.py restates the contract sequentially */
/* in numpy; every output equals it bit for bit and in the same order                     */
/* (csrc/meshsimplify.hip states the contract and the passes).  Stateless; no float       */
/* atomics: no result depends on launch geometry.                                         */
/* ------------------------------------------------------------------------------------ */
enum { SURFD_SIMPLIFY_MEAN = 0, SURFD_SIMPLIFY_QUADRIC = 1 };
/* vertices fp64 [V,3] and faces int32 [F,3] on the device.  A face that names a non-finite vertex goes; the vertices the others
 * name take part.  Cell index per axis k = floor((x - origin) / cell), origin (HOST, 3 doubles) or null = the minimum over the
 * vertices that take part; each k must lie in [0, 2^21), anything else is SURFD_ERR_ARG (never a wrapped key).  One cluster per
 * occupied cell, in ascending kx << 42 | ky << 21 | kz, members in ascending index.  representative: SURFD_SIMPLIFY_MEAN = the
 * sum of the members in that order / count; SURFD_SIMPLIFY_QUADRIC = the minimiser of the cell's area-weighted plane quadric
 * relative to the cell centre, eigenvalues below rank_tol times the largest truncated (six Jacobi sweeps), the mean where the point
 * is not finite or leaves the mean by more than a cell on an axis (a fall-back).  Faces are renamed, those with two equal names
 * (collapsed) go, the rest pass through surfd_meshclean_drop_duplicate_faces (its order); clusters no face names go.
 * out_vertices[V,3], out_faces[F,3] must hold the whole input; vertex_map[V] (nullable): the output vertex of every input
 * vertex, -1 without one; counts[6] (host): output vertices, output faces, clusters, collapsed faces, duplicate faces,
 * fall-backs.  F = 0 or V = 0: empty outputs, the map all -1.  3 F >= 2^31: SURFD_ERR_UNSUPPORTED; cell and rank_tol must be
 * positive and finite, the origin finite, an index outside [0, V) is found on the device before anything is indexed by it: all
 * SURFD_ERR_ARG.  HOST-SYNCS 3 TIMES (2 where every face collapses, 1 where none is kept): clusters and kept faces; the duplicate
 * pass's count; the output sizes. */
int surfd_meshsimplify_cluster(const double *vertices, int V, const int32_t *faces, int F, const double *origin, double cell, int representative,
                               double rank_tol, double *out_vertices, int32_t *out_faces, int32_t *vertex_map, int64_t *counts, surfd_stream s);
/* no reference counterpart; open3d's simplify_quadric_decimation(target_number_of_triangles) as rounds of independent collapses:
 * edge-collapse decimation to a target face count with quadric error metrics (no priority
 * queue; tests/meshdecimate_ref.py restates the contract sequentially in numpy, csrc/meshdecimate.hip carries its text and the
 * passes; every output equals the restatement bit for bit).  vertices fp64 [V,3] and faces int32 [F,3] on the device.  A face that
 * names a non-finite vertex or one vertex twice goes.  Every round: the unique edges, a point (the truncated minimiser of
 * Q_lo + Q_hi around the midpoint, eigenvalues below rank_tol times the largest dropped; the cheapest of midpoint, lo, hi where
 * that leaves the edge's enlarged box) and a cost per edge; an edge is valid when its valence is 1 or 2, the link condition
 * holds, it is no interior edge between border vertices, its opposite vertices keep three edges and no face of its two fans
 * turns by more than flip_cos allows; the first spread * ceil((F_now - target_faces) / 2) valid edges in ascending
 * (fp32 cost, hash of seed, round and edge) are candidates; one is selected iff its hashed priority is the least at both end
 * points and all their neighbours, so selected edges touch no common face; at most ceil((F_now - target_faces) / 2) collapse
 * (hi into lo, at the point, Q summed).  Border edges add border_weight times the quadric of the plane through the edge
 * perpendicular to their face.  Stops when F_now <= target_faces (0), when a round selects nothing (1) or after max_rounds (2).
 * out_vertices[V,3], out_faces[F,3] must hold the whole input; vertex_map[V] (nullable): the output vertex every input vertex
 * ended in, -1 where it took no part; counts[12] (host): output vertices, output faces, rounds, collapses, border collapses, stop
 * reason, edges refused in the last round by valence, link, border, opposite vertex, flip, NaN cost.  F = 0 or V = 0: empty
 * outputs, the map all -1.  3 F >= 2^31: SURFD_ERR_UNSUPPORTED; target_faces >= 0, border_weight >= 0, flip_cos in [0, 1),
 * rank_tol > 0, all finite, spread >= 1, max_rounds >= 1, and an index outside [0, V) (found on the device before anything is
 * indexed by it): all SURFD_ERR_ARG.  HOST-SYNCS 2 + 2 PER ROUND. */
int surfd_meshsimplify_decimate(const double *vertices, int V, const int32_t *faces, int F, int64_t target_faces, double border_weight, double flip_cos,
                                double rank_tol, int spread, int max_rounds, uint64_t seed, double *out_vertices, int32_t *out_faces,
                                int32_t *vertex_map, int64_t *counts, surfd_stream s);
/* no reference counterpart; incremental isotropic remeshing to a target edge length (Botsch and Kobbelt 2004) as rounds of independent operations:
 * a handle, because the mesh grows and the caller steps between iterations (the projection onto the input surface is the
 * caller's).  tests/meshremesh_ref.py restates the contract sequentially in numpy, csrc/meshremesh.hip
 * carries its text and the passes; vertices, faces, origin and counts equal the restatement bit for bit.  vertices fp64 [V,3] and
 * faces int32 [F,3] on the device are copied: a face that names a non-finite vertex or one vertex twice goes.  low2 and high2 are
 * the squares of the shortest and the longest edge length aimed at, made once by the caller (0 < low2 < high2, finite); flip_cos
 * in [0, 1) bounds the turn of a face against its standing normal and against the normal it had in the input.  A vertex keeps its
 * index for the life of the handle; new ones are appended.  3 F >= 2^31: SURFD_ERR_UNSUPPORTED; an index outside [0, V) (found on
 * the device before anything is indexed by it; with V = 0 every index of F > 0 faces is one) and the knobs: SURFD_ERR_ARG, *out stays
 * null.  HOST-SYNCS.  One stream at a time. */
typedef struct surfd_meshremesh surfd_meshremesh;
int surfd_meshremesh_create(const double *vertices, int V, const int32_t *faces, int F, double low2, double high2, double flip_cos, uint64_t seed,
                            surfd_stream s, surfd_meshremesh **out);
void surfd_meshremesh_destroy(surfd_meshremesh *m);
/* no reference counterpart; one iteration of the isotropic remeshing (tests/meshremesh_ref.py, Remesher.iterate):
 * up to split_rounds rounds that split every edge longer than high2 at its midpoint (1 + k children per face with
 * k marked half-edges), up to collapse_rounds rounds that collapse independent edges shorter than low2 (the rules of
 * surfd_meshsimplify_decimate, and no neighbour further than high2 from the point), up to flip_rounds rounds that flip independent
 * edges towards valence 6 (4 on a border), relax_sweeps Jacobi sweeps that move interior vertices towards the mean of their
 * neighbours in their tangent plane, relax in (0, 1] of the way.  A stage ends with the round that finds nothing.  counts[24]
 * (host): vertices named by a face, faces, splits, collapses, border collapses, flips, relaxed, relax refusals, split / collapse /
 * flip rounds made, the marks of the last split round, the refusals of the last collapse round by valence, link, border, opposite
 * vertex, long edge, flip and of the last flip round by orientation, equal corners, existing edge, degree, long diagonal, fold.
 * The arrays of the handle grow geometrically in a split round that needs it (the stream is drained first); a result with
 * 3 F >= 2^31 is SURFD_ERR_UNSUPPORTED and leaves the state of before that round.  HOST-SYNCS 1 TO 2 TIMES PER ROUND. */
int surfd_meshremesh_iterate(surfd_meshremesh *m, int split_rounds, int collapse_rounds, int flip_rounds, int relax_sweeps, double relax,
                             int64_t *counts, surfd_stream s);
/* no reference counterpart; the sizes of the isotropic remeshing's state (tests/meshremesh_ref.py, Remesher):
 * the vertex slots (named by a face or not) and the faces the handle holds now: the sizes of the buffers below */
int surfd_meshremesh_sizes(const surfd_meshremesh *m, int64_t *vertices, int64_t *faces);
/* no reference counterpart; the working positions of the isotropic remeshing, for the caller's projection (tests/meshremesh_ref.py, Remesher.X and origin):
 * positions[V_now,3] fp64 and origin[V_now] int32 (either nullable) of every vertex slot: origin is the input index while the
 * vertex is an input vertex at its input position, else -1.  set_positions takes positions[V_now,3] back (the caller changes
 * those of origin -1 only).  Device to device on the stream; no sync. */
int surfd_meshremesh_get_positions(const surfd_meshremesh *m, double *positions, int32_t *origin, surfd_stream s);
int surfd_meshremesh_set_positions(surfd_meshremesh *m, const double *positions, surfd_stream s);
/* no reference counterpart; the compact result of the isotropic remeshing (tests/meshremesh_ref.py, Remesher.emit):
 * out_vertices[V_now,3] (the vertices a face names, in ascending index), out_faces[F_now,3] renamed,
 * out_origin[V_now] (nullable); counts[2] (host): vertices and faces written.  The handle stays usable.  host-sync. */
int surfd_meshremesh_emit(surfd_meshremesh *m, double *out_vertices, int32_t *out_faces, int32_t *out_origin, int64_t *counts, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Point-cloud metrics: nearest neighbours between clouds and the matrix of directed      */
/* Chamfer means between two sets of clouds.  No reference counterpart (the reference     */
/* ships no evaluation code): stands for pytorch3d's knn_points(p1, p2, K=1) /            */
/* chamfer_distance and for the distance matrices of the MMD / COV / 1-NNA protocol of    */
/* Achlioptas et al. 2018 as used in PointFlow.  Plain fp32; bitwise deterministic.       */
/* ------------------------------------------------------------------------------------ */
/* no reference counterpart; pytorch3d's knn_points(a, b, K=1):
 * a[B,Na,3], b[B,Nb,3] -> d2[B,Na] (fp32, nullable), idx[B,Na] (int32 into b's cloud, nullable): for every point of a_i its
 * nearest point of b_i.  d2 = (dx dx + dy dy) + dz dz with diff = a - b, every operation rounded once; the winner is the minimum
 * under (d2, index): ties go to the lower index.  Na, Nb >= 1.  B = 0 is a no-op. */
int surfd_cloud_nn(const float *a, const float *b, int B, int Na, int Nb, float *d2, int32_t *idx, surfd_stream s);
/* no reference counterpart; one direction of pytorch3d's chamfer_distance for every pair of two sets (the matrices behind MMD /
 * COV / 1-NNA):
 * a[M,Na,3], b[R,Nb,3] -> mean[M,R] (fp32): mean[i,j] = (1/Na) * sum over p in a_i of min over q in b_j of |p - q|^2;
 * below[M,R] (int32, nullable): how many points of a_i have that minimum < tau2 (strict; fp32 compare on the fp32 d2).
 * The sum over a cloud's points is taken in fp64, in a fixed order that depends on Na only, and rounded to fp32 once after
 * the division: entry (i,j) has the same bits whatever M and R it is computed in, and under any permutation of b_j's points.
 * The other direction is a second call with the roles swapped. */
int surfd_cloud_nn_matrix(const float *a, int M, int Na, const float *b, int R, int Nb, float tau2,
                          float *mean, int32_t *below, surfd_stream s);
/* no reference counterpart; the launch plan surfd_cloud_nn_matrix takes for M query clouds of Na points and R candidate clouds:
 * P = 1, 2, 4, 8 query points per lane for Na <= 256, <= 512, <= 1024, above; query_tiles = ceil(Na / (256 P)) register tiles
 * of the query cloud (above 1 they are reloaded per candidate cloud); want = min(R, max(1, ceil(2048 / M))), span = ceil(R / want)
 * candidate clouds per workgroup, S = ceil(R / span) workgroups per query cloud (the last range may be shorter).  The same
 * checks of M, Na, R and the same return codes as the launch; no device call; every out pointer may be NULL.  For tests and
 * tools that must know which path a shape takes. */
int surfd_cloud_nn_matrix_plan(int M, int Na, int R, int *P, int *S, int *span, int *query_tiles);

/* ------------------------------------------------------------------------------------ */
/* Farthest point sampling: K points of a cloud, each the one farthest from every pick    */
/* before it, and the squared covering radius after every pick.  No reference counterpart */
/* (the reference samples at random): stands for pytorch3d's sample_farthest_points.      */
/* Plain fp32; the index sequence is bitwise a function of the input.                     */
/* ------------------------------------------------------------------------------------ */
/* no reference counterpart; the scratch size of a farthest-point-sampling call:
 * bytes = 4 B max(0, N - 32768): the running minima of the points beyond the 32 768 a workgroup keeps on chip; 0 for arguments
 * out of range */
int64_t surfd_cloud_fps_workspace_bytes(int B, int N);
/* no reference counterpart; pytorch3d's sample_farthest_points(points, lengths, K):
 * points[B,N,3] -> idx_out[B,K] (int32 into the cloud), cover2_out[B,K] (fp32, nullable).  Per cloud b with n = lengths[b]
 * valid points (lengths int32 [B] on the device, NULL = N everywhere): mind[i] = +inf; s = start[b] (int32 [B] on the device,
 * NULL = 0); for k < K: idx[b,k] = s; mind[i] = min(mind[i], d2(p_i, p_s)) with d2 = (dx dx + dy dy) + dz dz, diff = p_i - p_s,
 * every operation rounded once; s = the i < n with the largest mind[i], the LOWER index on ties; cover2[b,k] = mind[s], the
 * squared covering radius of the first k + 1 picks (non-increasing in k, 0 once every point is taken).  For k >= n:
 * idx[b,k] = -1, cover2[b,k] = 0.  Duplicated points are legal (once mind is 0 everywhere the lowest index is picked again).
 * Clouds are independent: a row has the same bits whichever batch it is computed in.  1 <= K; 1 <= N <= 1 048 576 and
 * B <= 1 048 576 (beyond: SURFD_ERR_UNSUPPORTED); B = 0 is a no-op.  lengths[b] outside 1 .. N and start[b] outside
 * 0 .. n - 1 are the caller's to refuse: the kernel clamps them into range rather than read out of bounds; points beyond
 * lengths[b] are never read; NaN has no place in the order.  workspace: at least surfd_cloud_fps_workspace_bytes(B, N) bytes
 * on the device (NULL when that is 0), contents irrelevant before and after; one workspace serves one stream at a time.
 * Stream-ordered, no host sync, no state kept in the library. */
int surfd_cloud_fps(const float *points, int B, int N, const int32_t *lengths, const int32_t *start, int K, int32_t *idx_out,
                    float *cover2_out, void *workspace, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Normals of point clouds: K nearest neighbours within a cloud, the covariance of every  */
/* neighbourhood and its eigen-decomposition (normal, surface variation).  No reference   */
/* counterpart (the reference ships no evaluation code): stands for open3d's              */
/* estimate_normals / pytorch3d's estimate_pointcloud_normals.  fp32 pair arithmetic,     */
/* fp64 moments and Jacobi sweeps; every output is bitwise a function of the input.       */
/* ------------------------------------------------------------------------------------ */
/* no reference counterpart; pytorch3d's estimate_pointcloud_normals(points, neighborhood_size=K) with its knn_points:
 * x[B,N,3] -> normals[B,N,3], eigenvalues[B,N,3] (fp32, ascending), knn_idx[B,N,K] (int32 into the cloud, nullable).  Per
 * cloud b with n = lengths[b] valid points (int32 [B] on the device, NULL = N everywhere) and per point i < n:
 * (1) d = x_j - x_i per coordinate in fp32, d2 = (dx dx + dy dy) + dz dz, every operation rounded once; (2) the neighbourhood
 * is the K smallest j < n under (d2, j): the point itself is a candidate like any other, ties go to the lower index, knn_idx
 * lists them in that order; (3) in fp64 and rank order s1_a += d_a, s2_ab += d_a d_b, then m = s1 / K, C_ab = s2_ab / K - m_a m_b;
 * (4) six cyclic Jacobi sweeps over (0,1), (0,2), (1,2) in fp64 (+ - * / sqrt only; the formulas are in csrc/cloudnormals.hip);
 * (5) eigenvalues = the three lambda sorted ascending (stably), rounded once to fp32, not clamped; (6) normal = the column of
 * the smallest, rounded once to fp32, not renormalised, negated as a whole if its component of largest magnitude (lowest axis on
 * a tie) is negative; (7) rows i >= n are zeros, and -1 in knn_idx; their input is never read.  Clouds and points are
 * independent: a row has the same bits whichever batch or launch it is computed in.  3 <= K <= 64, K <= N, N <= 1 048 576
 * (beyond: SURFD_ERR_UNSUPPORTED); B = 0 is a no-op.  lengths[b] outside K .. N is the caller's to refuse: the kernel clamps it
 * into 0 .. N and writes a cloud with fewer than K points as padding rather than read out of bounds.  NaN has no place in the
 * order.  Stream-ordered, no host sync, no workspace, no state kept in the library. */
int surfd_cloud_normals(const float *x, int B, int N, const int32_t *lengths, int K, float *normals, float *eigenvalues,
                        int32_t *knn_idx, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Mesh renderer: a two-sided z-buffer rasteriser (depth, barycentrics, normals, masks,   */
/* headlight shading) and contour images, for condition images / sketches, view-based     */
/* evaluation and previews.  No reference counterpart (the reference looks at meshes in   */
/* open3d / pymeshlab windows).  fp32 + integer; bitwise deterministic.                   */
/* ------------------------------------------------------------------------------------ */
typedef struct surfd_raster surfd_raster;
#define SURFD_RASTER_FORCE_SMALL 1   /* flags bit 0: every triangle is rasterised by its set-up lane */
#define SURFD_RASTER_FORCE_LARGE 2   /* flags bit 1: every triangle goes through the list, one wave each (excludes bit 0) */
#define SURFD_RASTER_CAMERA_FLOATS 18
/* no reference counterpart; an offscreen render target of open3d / pymeshlab:
 * the handle owns the 64-bit key buffer [max_views, H, W], the device copy of a call's cameras and a workspace (projected
 * vertices, list of large triangles) that grows on demand.  1 <= H, W <= 2048; 1 <= max_views <= 64.  One stream and one host
 * thread at a time per handle. */
int surfd_raster_create(int H, int W, int max_views, surfd_raster **out);
void surfd_raster_destroy(surfd_raster *r);
/* no reference counterpart; rendering a triangle mesh to per-pixel buffers:
 * vertices[V,3] fp32 and faces[F,3] int32 on the device; vertex_normals[V,3] fp32 (world space) on the device or NULL (geometric
 * face normals); cameras[n_views,18] fp32 on the HOST (copied before the call returns): the row-major 3x4 world->camera
 * matrix (x right, y down, z forward), then mode (0 perspective, 1 orthographic), fx, fy, cx, cy in pixels, near (>= 0; > 0 in
 * perspective mode).  light[3] on the host (camera space; NULL = the headlight (0, 0, -1)); ambient in [0, 1].
 * Outputs on the device, each nullable, [n_views, H, W] row-major (row j = image line, pixel centres at integer + 0.5):
 * face int32 (-1 background), depth fp32 (metric camera z, +inf background), bary fp32 x3 (perspective-correct, in the
 * caller's vertex order), normal fp32 x3 (camera space, unit or zero, turned to the viewer: n_z <= 0), mask uint8,
 * shaded fp32 = ambient + (1 - ambient) |n . light| (0 background); dropped_per_view int32 [n_views]: triangles left out
 * because a vertex has camera z <= near, projects outside +-2^22 / 256 pixels or is an index outside [0, V) (there is no
 * near-plane clipping).  Coverage is exact (integer edge functions on a 1/256-pixel grid, top-left rule, both windings);
 * a pixel's winner is the minimum of (compared depth, face index), so the buffers do not depend on face order beyond exact
 * depth ties, on the batch of views, on flags or on launch geometry.  V, F >= 0 (F = 0 gives the empty image);
 * 1 <= n_views <= max_views; n_views * V and n_views * F < 2^31. */
int surfd_raster_render(surfd_raster *r, const float *vertices, int V, const int32_t *faces, int F, const float *vertex_normals,
                        const float *cameras, int n_views, int flags, const float *light, float ambient,
                        int32_t *face, float *depth, float *bary, float *normal, unsigned char *mask, float *shaded,
                        int32_t *dropped_per_view, surfd_stream s);
/* no reference counterpart; a line drawing of a rendered view:
 * mask / depth / normal [n_views, H, W(, 3)] as surfd_raster_render wrote them -> ink[n_views, H, W] uint8: 1 where the pixel's
 * mask differs from a 4-neighbour's, or both are covered and their depths differ by more than depth_jump (>= 0) or their
 * normals' dot product is below cos_crease (in [-1, 1]).  Neighbours outside the image are background. */
int surfd_raster_contours(const surfd_raster *r, const unsigned char *mask, const float *depth, const float *normal, int n_views,
                          float depth_jump, float cos_crease, unsigned char *ink, surfd_stream s);

/* ------------------------------------------------------------------------------------ */
/* Voxelisation and volumetric IoU: occupancy grids of meshes (surface, solid) and clouds, */
/* and intersection over union between grids.  No reference counterpart (the reference    */
/* ships no evaluation code): stands for the occupancy grids and the IoU of the           */
/* single-view reconstruction protocol (Choy et al. 2016, 3D-R2N2; Mescheder et al. 2019, */
/* Occupancy Networks).  One fp32 step (the snap), then int64: exact and bitwise          */
/* deterministic for any face order, winding, batch, path and launch geometry.            */
/* ------------------------------------------------------------------------------------ */
/* the two flags are test switches (they prove the paths bit-identical); FORCE_SMALL makes one lane walk a triangle's whole box,
 * however large: not for large triangles on fine grids */
#define SURFD_VOXEL_FORCE_SMALL 1   /* flags bit 0: every triangle is voxelised by its set-up lane */
#define SURFD_VOXEL_FORCE_LARGE 2   /* flags bit 1: every triangle goes through the list, one wave each (excludes bit 0) */
#define SURFD_VOXEL_MAX_RESOLUTION 512
/* The grid of every entry below: the cube [lo, hi]^3 cut into R^3 voxels, 1 <= R <= 512, hi > lo; voxel (i, j, k) is the CLOSED
 * box [i, i+1] x [j, j+1] x [k, k+1] in voxel units, axes (x, y, z) = (i, j, k).  bits[R, R, W] uint32 on the device,
 * W = ceil(R / 32): bit k & 31 of word k >> 5 of column (i, j) is voxel k; padding bits are never set.  bits is ACCUMULATED
 * into (atomicOr): the caller zeroes it, several meshes or clouds may be OR-ed into one grid.  A coordinate x is snapped as
 * q = rint((x - lo) * s), s = fp32(256 R / (hi - lo)) (units of 1/256 voxel, ties to even); it is invalid when it is NaN or
 * |q| > 2^19.  R outside 1 .. 512, hi <= lo, both force flags, 3 V or 3 F >= 2^31 and null pointers are SURFD_ERR_ARG, found
 * before any HIP call.
 * The workspace is passed by the caller (the library keeps no handle and no state for these entries): at least
 * surfd_voxel_workspace_bytes(F, R) bytes on the device, contents irrelevant before and after a call; it holds the counters,
 * the list of large triangles and, for the solid fill, the XOR buffer and the crossing parities.  One workspace serves one
 * stream at a time. */
/* no reference counterpart; the scratch size of a voxelisation call:
 * bytes = 4 (16 + F + R R W + R R); 0 for arguments out of range */
int64_t surfd_voxel_workspace_bytes(int F, int R);
/* no reference counterpart; the conservative surface voxelisation of a triangle mesh (binvox -e, trimesh's voxelize):
 * vertices[V,3] fp32, faces[F,3] int32 on the device.  Voxel (i, j, k) is set iff the snapped triangle intersects the closed
 * box: the 13-axis separating-axis test (Akenine-Moller) on integers, an axis separates on strict inequality only, so touching
 * counts.  dropped (int32 on the device, nullable): triangles left out because a vertex is invalid or an index lies outside
 * [0, V) (never a fault); degenerate (nullable): triangles whose snapped doubled area vector is zero (skipped).  F = 0 is legal. */
int surfd_voxel_surface(const float *vertices, int V, const int32_t *faces, int F, float lo, float hi, int R, int flags, void *workspace,
                        uint32_t *bits, int32_t *dropped, int32_t *degenerate, surfd_stream s);
/* no reference counterpart; the parity (ray-stabbing) fill of a closed mesh along +z (binvox's default, trimesh's fill):
 * voxel (i, j, k) is filled iff an odd number of triangles cross the column through (256 i + 128, 256 j + 128) strictly below
 * the voxel centre 256 k + 128.  A column's crossings are decided with integer edge functions and the top-left rule, so one
 * on a shared edge or through a vertex counts once; triangles of zero projected area contribute nothing.  bits |= fill, and
 * also |= the surface voxelisation above when include_surface != 0.  odd_columns (int32 on the device, nullable): the number
 * of columns whose crossing total is odd — 0 exactly when the snapped mesh is closed over the grid's columns.  dropped as above. */
int surfd_voxel_solid(const float *vertices, int V, const int32_t *faces, int F, float lo, float hi, int R, int flags, void *workspace,
                      int include_surface, uint32_t *bits, int32_t *odd_columns, int32_t *dropped, surfd_stream s);
/* no reference counterpart; the occupancy grid of a point cloud:
 * points[P,3] fp32 on the device; a point sets voxel floor(q / 256) per axis, a point exactly on the upper grid face belongs to
 * the last voxel.  outside (int32 on the device, nullable): points outside the grid or invalid (skipped).  No workspace. */
int surfd_voxel_points(const float *points, int P, float lo, float hi, int R, uint32_t *bits, int32_t *outside, surfd_stream s);
/* no reference counterpart; volumetric intersection over union of occupancy grids:
 * a[M, R, R, W], b[N, R, R, W] packed grids on the device.  paired == 0: inter / uni (int32) and iou (fp32) are [M, N], entry
 * (m, n) from a_m and b_n; paired != 0 (M = N): [M], entry m from a_m and b_m.  inter = popcount(a & b), uni = popcount(a | b),
 * iou = fp32(inter) / fp32(uni) rounded once, 1.0 when uni = 0.  Integer sums: an entry has the same bits whatever M and N it
 * is computed in.  All three outputs are required (the counts are the accumulators); the number of pairs must stay below 2^31. */
int surfd_voxel_iou(const uint32_t *a, int M, const uint32_t *b, int N, int R, int paired, int32_t *inter, int32_t *uni, float *iou,
                    surfd_stream s);

#ifdef __cplusplus
}
#endif
#endif /* SURFD_HIP_H */
