/*
 * fluid_amd.h -- C ABI of the MI355X Stable-Fluids step (libfluid_amd.so).
 *
 * Drop-in boundary for the vel_step + dens_step hot path of the reference's
 * project/sequential/FluidSequential.c.  The reference has no library or FFI
 * interface of its own: its boundary is the two calls at FluidSequential.c:305-306
 * with N, DT, VIS, DIFF as compile-time macros (:6-9).  Each entry point below
 * cites the reference lines whose behaviour it reproduces.  Plain C types only.
 *
 * Host arrays ("fields") are what the reference's main() allocates (:277-282):
 * (N+2)*(N+2) floats, row-major, cell (column j, row i) at j + i*(N+2), ghost
 * ring at index 0 and N+1.  The caller owns them; the library owns all device
 * memory and scratch and never allocates per step.
 *
 * Every function returns FLUID_OK (0) or a FLUID_E_* code and never exits or
 * aborts (the reference's CUDA variants exit(EXIT_FAILURE) in their CHECK
 * macro, naivePar/FluidParallelBlockPerElement-Naive.cu:26-35).
 * fluid_last_error() returns a description of the calling thread's last failure.
 *
 * Threading: one context is used by one host thread at a time; different
 * contexts are independent.
 */
#ifndef FLUID_AMD_H
#define FLUID_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLUID_OK        0
#define FLUID_E_INVALID 1 /* bad N, odd or negative sweep count, null pointer, bad field id */
#define FLUID_E_NOMEM   2 /* device or host allocation failed */
#define FLUID_E_HIP     3 /* a HIP runtime call failed */
#define FLUID_E_COMM    4 /* the multi-GPU exchange callback failed or is missing */

/* Field ids of a context = the six arrays of the reference's main()
 * (FluidSequential.c:277-282) plus six library-owned scratch fields: TMP0-2 are the other half of a solve's
 * ping-pong (the reference malloc()s one per diffuse call, :88), TMP3-5 receive `x + dt*s` when add_source runs
 * inside the first launch of the solve that consumes it (FLUID_PARAM_FUSE_ADD_SOURCE). */
enum {
    FLUID_U = 0, FLUID_V = 1, FLUID_DENS = 2,
    FLUID_U_PREV = 3, FLUID_V_PREV = 4, FLUID_DENS_PREV = 5,
    FLUID_TMP0 = 6, FLUID_TMP1 = 7, FLUID_TMP2 = 8,
    FLUID_TMP3 = 9, FLUID_TMP4 = 10, FLUID_TMP5 = 11,
    FLUID_NFIELDS = 12
};

/* Jacobi kernels (identical results, different data paths).  TB = temporally
 * blocked: up to 16 sweeps per launch, same bits as that many single-sweep launches. */
enum { FLUID_JACOBI_STREAM = 0, FLUID_JACOBI_LDS = 1, FLUID_JACOBI_NAIVE = 2, FLUID_JACOBI_TB = 3 };

/* Tuning knobs for fluid_set_param(); none of them changes results with FLUID_STORAGE_F32.  (With FLUID_STORAGE_F16
 * a fused launch rounds once when it stores, so the launch schedule -- TB_MAX_SWEEPS, TB_MIN_CELLS, and the Jacobi
 * variant: FLUID_JACOBI_TB takes the greedy 8 / 4 / 2 sweeps per launch, the others one -- is part of the result there,
 * and so is F16_PRESSURE_SCALE; all other knobs are speed only in both storage types.) */
enum {
    FLUID_PARAM_TB_MAX_SWEEPS = 0, /* most sweeps fused per launch by FLUID_JACOBI_TB: 16 (default), 8, 4 or 2 */
    FLUID_PARAM_TB_ROWS = 1,       /* output rows per wave strip of FLUID_JACOBI_TB; 0 = auto          */
    FLUID_PARAM_HALO = 2,          /* multi-GPU ghost-zone depth (clamped to slab height - 1)          */
    FLUID_PARAM_TB_FAST_DIVISION = 3 /* how FLUID_JACOBI_TB may replace x/beta by an exactly equivalent reciprocal form,
                                      each after proving the equivalence for that beta on all 2^32 float inputs on
                                      the device.  2 (default): one float multiply when beta is a power of two (and
                                      alpha 1), else Markstein's residual correction with the residual scaled by 2^24
                                      (two float multiplies and two fused multiply-adds, exact for every |x| < 2^104; a
                                      wave that stores inf or NaN -- the only thing larger dividends can turn into --
                                      repeats its strip with the double-precision form).  3: the double-precision
                                      multiply for every such beta (the round-2 default).  1: the two-term float
                                      reciprocal fma(x, hi, x*lo) in waves whose right-hand side is nowhere smaller
                                      than beta * 2^-72 (which bounds every dividend away from the range where that
                                      form is one ulp off), the double-precision form elsewhere.  0: always divide */
    ,FLUID_PARAM_TB_EDGE_ROWS_PCT = 5 /* strip height of the two windows that carry the ghost columns, in % of
                                      the interior windows' (default 40; 0 = same): load balance only  */
    ,FLUID_PARAM_TB_LANE_COLUMNS = 6 /* columns per lane of FLUID_JACOBI_TB: 2 (default; thin waves, 4 per SIMD)
                                      or 4 (2 per SIMD): speed only                                      */
    ,FLUID_PARAM_TB_T16_MIN_CELLS = 7 /* 16-sweep launches (fp32 storage, 2-column lanes) on slabs of at least this many
                                      cells, for either form of the solve; -1 (default): the measured rule -- from
                                      8 M cells, the general form only once a field outgrows 96 MiB     */
    ,FLUID_PARAM_TB_AUTOTUNE = 8   /* 1 (default): with TB_ROWS = 0 the strip height of each launch shape is measured
                                      at run time -- the first ~20 launches of a shape try a handful of heights, the
                                      fastest is kept for the process; 0: the closed-form choice.  Speed only.  */
    ,FLUID_PARAM_SLAB_OVERLAP = 10 /* 1 (default): on row slabs fluid_step runs the density diffusion on a second stream
                                      beside the velocity path (a slab's launches leave most of the chip idle), when the
                                      ghost zones cover a whole solve; 0: one stream.  Speed only.                */
    ,FLUID_PARAM_EARLY_ADVECT = 11 /* 1 (default): on row slabs fluid_step starts each advection on the PREVIOUS step's velocity
                                      bound (+25 %) while the new bound is still on its way to the host, and repeats it in
                                      the rare case the bound grew past that (its inputs are still intact then), so the
                                      GPU does not idle while the host reads the bound; 0: wait first.  Speed only. */
    ,FLUID_PARAM_FUSE_DIVERGENCE = 9 /* 1 (default): inside fluid_step / fluid_vel_step on one GPU the divergence of a
                                      projection is computed by the first launch of the pressure solve that consumes it
                                      (no separate pass over u, v); 0: its own kernel first.  Speed only.        */
    ,FLUID_PARAM_FUSE_ADD_SOURCE = 12 /* 1 (default): inside fluid_step / fluid_vel_step / fluid_dens_step a non-zero source is
                                      added by the first launch of the diffusion that consumes the sum (which reads both
                                      operands anyway: the source is its first guess) and stored out of place, instead of
                                      by a pass of its own over the field; 0: add_source as its own kernel.  Speed only. */
    ,FLUID_PARAM_XCHG_OVERLAP = 13 /* 1 (default): on row slabs every exchange is enqueued on a stream of its own, ordered against
                                      the compute stream by events, and the halo exchange that feeds a Jacobi solve is not
                                      waited for at once: the solve's first launch runs the strips that need this slab's own
                                      rows only while the rows travel, and the strips next to the slab's edges behind the
                                      exchange's event.  0: exchanges in line on the context's stream.  Speed only.   */
    ,FLUID_PARAM_F16_PRESSURE_SCALE = 14 /* fp16 storage only.  1 (default): inside a step the divergence and the pressure of a
                                      projection are stored multiplied by 2^(floor(log2 N) - 2) -- plain, they are of the order
                                      h * |velocity| and fall into fp16's subnormal range from a few thousand cells per side
                                      on -- and divided back exactly (in the gradient subtraction; on the host when u_prev /
                                      v_prev are downloaded).  Any other reader -- the add_source of a step with sources
                                      after a step -- gets the field divided back in place and stored again, rounded to
                                      fp16 a second time.  0: plain values.  Changes fp16 results (not fp32 ones).      */
    ,FLUID_PARAM_TB_FILL = 15      /* 1 (default): the fused kernel skips the stage evaluations of each strip's pipeline fill
                                      and drain that no stored row depends on (about T(T+1) of a strip's T(rows + 2T));
                                      0: every stage at every step.  Speed only.                                        */
    ,FLUID_PARAM_TB_MIN_CELLS = 4  /* FLUID_JACOBI_TB fuses sweeps only on slabs of at least this many cells
                                      (default 0: always); smaller ones run one-thread-per-cell sweeps   */
};

typedef struct fluid_ctx fluid_ctx;

const char *fluid_last_error(void);

/* ---- the reference's loop body on host arrays ----------------------------
 * step():     FluidSequential.c:298-306 for z > 0 -- the three *_prev source
 *             arrays are zero, then vel_step(u,v,u_prev,v_prev,visc) and
 *             dens_step(dens,dens_prev,u,v,diff), 40 Jacobi sweeps per solve
 *             (:91).  u, v, dens are updated in place.
 * step_src(): FluidSequential.c:305-306 verbatim, sources supplied by the
 *             caller (the z == 0 step).  On return u_prev holds the last
 *             pressure, v_prev the last divergence and dens_prev the diffused
 *             density, exactly where the reference leaves them (SWAPs at
 *             :201,209,228-229,181,184).  `iters` must be even and >= 0: with an
 *             odd count the reference free()s the caller's array (:100,103).
 * Both keep a per-thread cached context for the last N, upload, run one step
 * on the current HIP device, and download. */
int step(int N, float dt, float diff, float visc, float *u, float *v, float *dens);
int step_src(int N, float dt, float diff, float visc, int iters,
             float *u, float *v, float *dens,
             float *u_prev, float *v_prev, float *dens_prev);
/* Drops the cached context of step()/step_src() (frees its device memory). */
int fluid_release_cached(void);

/* alpha = ((dt*coef)*N)*N, beta = 1 + 4*alpha in float (FluidSequential.c:179-180,199-200). */
int fluid_coefficients(int N, float dt, float coef, float *alpha, float *beta);

/* ---- device-resident context --------------------------------------------- */
typedef struct fluid_config {
    int n;              /* interior size N (grid is (N+2)^2), N >= 1                    */
    int rank, nranks;   /* row-slab decomposition: this context owns slab `rank` of `nranks` */
    int halo;           /* Jacobi ghost-zone depth between exchanges (0 = default)      */
    int jacobi_variant; /* FLUID_JACOBI_*                                               */
    void *stream;       /* hipStream_t to run on, or NULL for a library-owned stream    */
    void *arena;        /* device memory of fluid_arena_bytes_ex(n, storage) bytes, or NULL to hipMalloc */
    size_t arena_bytes;
    int storage;        /* FLUID_STORAGE_F32 (default; bit parity with the reference) or FLUID_STORAGE_F16 */
} fluid_config;

/* Field storage on the device.  F16 (BASELINE config "fp16 fields with fp32 Jacobi accumulate"):
 * fields are IEEE half, every operator widens its inputs to float, computes exactly as the fp32
 * path does, and rounds to nearest once when it stores; the fused Jacobi kernel keeps the
 * intermediate sweeps of a launch in fp32 registers.  Host arrays at this ABI stay float. */
enum { FLUID_STORAGE_F32 = 0, FLUID_STORAGE_F16 = 1 };

size_t fluid_arena_bytes(int N);                       /* fp32 storage */
size_t fluid_arena_bytes_ex(int N, int storage);
/* Device layout of one field: W = N+2 rows of `pitch` elements, column c at
 * element index c + xoff; field f starts f*field_floats elements into the arena.
 * In an ensemble of M members (fluid_create_ensemble) the fields are laid out [field][member]: field f starts
 * f*M*field_floats elements into the arena and holds its M members back to back, member m field_floats*m elements
 * behind the address fluid_field_ptr() returns (which is member 0's) -- one (M, N+2, pitch) array per field. */
int fluid_layout(int N, int *pitch, int *xoff, size_t *field_floats);

int fluid_create(int N, fluid_ctx **out);                      /* 1 GPU, defaults */
int fluid_create_ex(const fluid_config *cfg, fluid_ctx **out);
int fluid_destroy(fluid_ctx *ctx);
int fluid_synchronize(fluid_ctx *ctx);

/* ---- ensembles: M independent simulations of the same size in one context ---------------------------------
 * Every member has its own twelve fields; all members share N, the storage type and every fluid_set_param knob, and --
 * through the classic calls -- the scalar arguments of each call (the _members calls below give each member its own dt,
 * diff and visc).  One call to fluid_step / fluid_vel_step / fluid_dens_step / fluid_op_* / fluid_fill
 * does to every member what it does to a one-member context, in the SAME kernel launches (the member index rides in the
 * launch grid), and member m ends up with exactly the bits a one-member context given m's arrays would hold.
 * `members` in [1, 21845]; cfg->nranks must be 1 when members > 1; cfg->arena, if given, holds
 * fluid_arena_bytes_ensemble() bytes: 12 x members fields plus the 256-byte control block.
 * fluid_create_ensemble(cfg, 1, ..) is fluid_create_ex(cfg, ..).  Argument errors are reported before the device is touched.
 * On a context with more than one member:
 *   - fluid_upload / fluid_download / fluid_upload_rows / fluid_download_rows return FLUID_E_INVALID (they would have to
 *     pick a member or broadcast silently): use the _member calls;
 *   - fluid_residual and fluid_absmax_velocity return the maximum over all members (one value per member, sums and
 *     statistics across the members: the ensemble diagnostics further down);
 *   - fluid_op_diffuse_tol (every member's sweep count would depend on the others), fluid_set_exchange,
 *     fluid_exchange_now and the fluid_exchange_rccl_* calls return FLUID_E_INVALID;
 *   - fluid_timing counts jacobi_field_launches, sweeps and pressure_sweeps once per member, jacobi_launches per launch. */
int fluid_create_ensemble(const fluid_config *cfg, int members, fluid_ctx **out);
size_t fluid_arena_bytes_ensemble(int N, int storage, int members);   /* host logic; 0 on bad arguments */
int fluid_members(fluid_ctx *ctx, int *members);
/* Whole-field copies of one member (host pointer: the (N+2)^2 array).  Synchronous.  An upload first settles whatever the
 * library still owes the field (zeros by definition, a deferred add_source) in ALL members, then replaces this one. */
int fluid_upload_member(fluid_ctx *ctx, int member, int field, const float *host);
int fluid_download_member(fluid_ctx *ctx, int member, int field, float *host);
/* One value PER MEMBER where the calls further down take a scalar (a parameter study in one ensemble): every array is host
 * memory with fluid_members(ctx) entries that the library has finished with when the call returns.  Member m ends up with
 * exactly the bits a one-member context would hold after the same calls with dt[m], diff[m], visc[m] (alpha[m], beta[m]) as
 * its scalars, and a call issues the SAME launches as its scalar twin: the constants travel in a table in device memory
 * (library-owned, outside the arena, allocated at the first such call) that each wave indexes by its member.  Tables are
 * copied on the context's stream from a ring of pinned slots, and one whose contents are already in the ring is not copied
 * again: calls may follow one another with different values without a wait, a loop with the same values uploads nothing.
 * alpha / beta are formed per member by the same arithmetic as fluid_coefficients.  A solve whose members' betas call for
 * different division modes (FLUID_PARAM_TB_FAST_DIVISION) runs in the most general mode proven for all of them -- exact
 * like every mode, only slower.  Each DISTINCT beta is proven on the device once per process (about 2.7 ms and one stream
 * synchronise each): the first step of M distinct viscosities and M distinct diffusivities pays about 2 M proofs.
 * A null context or array, or an entry that is not finite: FLUID_E_INVALID (the message names the call and the member),
 * nothing launched, nothing changed.  Every finite value is accepted (dt <= 0, coefficients 0, betas <= 0 included).
 * With one member (row slabs included) a _members call is the scalar call with element 0.  The residual per member, with
 * each member's own coefficients, is fluid_residual_members (ensemble diagnostics, below); fluid_op_diffuse_tol and the
 * exchange calls stay unavailable on ensembles. */
int fluid_step_members(fluid_ctx *ctx, const float *dt, const float *diff, const float *visc, int iters,
                       int nsteps, int use_sources);
int fluid_vel_step_members(fluid_ctx *ctx, const float *dt, const float *visc, int iters);
int fluid_dens_step_members(fluid_ctx *ctx, const float *dt, const float *diff, int iters);
int fluid_op_add_source_members(fluid_ctx *ctx, int x, int s, const float *dt);
int fluid_op_jacobi_sweep_members(fluid_ctx *ctx, int b, int x, int x0, int out,
                                  const float *alpha, const float *beta);
int fluid_op_diffuse_members(fluid_ctx *ctx, int b, int x, int x0, const float *alpha, const float *beta,
                             int iters);
int fluid_op_advect_members(fluid_ctx *ctx, int b, int d, int d0, int u, int v, const float *dt);

/* Interior rows [*row_lo, *row_hi) owned by this context's slab (1..N+1 for one GPU). */
int fluid_owned_rows(fluid_ctx *ctx, int *row_lo, int *row_hi);
/* Device address of row 0 of a field, valid until the next solver call: a
 * field keeps its id but may trade buffers with TMP0 inside a solve, so the
 * exchange callback must ask every time. */
int fluid_field_ptr(fluid_ctx *ctx, int field, void **dev_ptr);
/* Device address of the 4-byte reduction scalar (a non-negative float) that
 * FLUID_XCHG_MAX_BEGIN reduces in place; it lives in the last 256 bytes of the arena. */
int fluid_scalar_ptr(fluid_ctx *ctx, void **dev_ptr);

/* Host <-> device copies of a whole field, or of rows [row_lo,row_hi) of it
 * (host pointer is always to the full (N+2)^2 array). Synchronous. */
int fluid_upload(fluid_ctx *ctx, int field, const float *host);
int fluid_download(fluid_ctx *ctx, int field, float *host);
int fluid_upload_rows(fluid_ctx *ctx, int field, const float *host, int row_lo, int row_hi);
int fluid_download_rows(fluid_ctx *ctx, int field, float *host, int row_lo, int row_hi);
int fluid_fill(fluid_ctx *ctx, int field, float value);

/* nsteps loop bodies of FluidSequential.c:289-312 on the resident fields.  With
 * use_sources != 0 the first step consumes the resident *_prev fields as
 * sources (z == 0); every other step zeroes them first (:298-302). */
int fluid_step(fluid_ctx *ctx, float dt, float diff, float visc, int iters,
               int nsteps, int use_sources);
int fluid_vel_step(fluid_ctx *ctx, float dt, float visc, int iters);   /* FluidSequential.c:189-241 */
int fluid_dens_step(fluid_ctx *ctx, float dt, float diff, int iters);  /* FluidSequential.c:176-186 */

/* ---- single operators on resident fields (field ids; all in place) -------- */
int fluid_op_set_bnd(fluid_ctx *ctx, int b, int x);                               /* :62-75   */
int fluid_op_add_source(fluid_ctx *ctx, int x, int s, float dt);                  /* :78-82   */
int fluid_op_jacobi_sweep(fluid_ctx *ctx, int b, int x, int x0, int out,
                          float alpha, float beta);                               /* :92-101, one k */
int fluid_op_diffuse(fluid_ctx *ctx, int b, int x, int x0, float alpha, float beta,
                     int iters);                                                  /* :85-104; uses TMP0 */
int fluid_op_advect(fluid_ctx *ctx, int b, int d, int d0, int u, int v, float dt); /* :107-141 */
int fluid_op_divergence(fluid_ctx *ctx, int u, int v, int p, int div);            /* :143-158 */
int fluid_op_subtract_gradient(fluid_ctx *ctx, int u, int v, int p);              /* :161-173 */

/* ---- diagnostics (wavefront reductions; never alter the fields) ----------- */
/* max over owned interior cells of |beta*x - alpha*(L+R+U+D) - x0| */
int fluid_residual(fluid_ctx *ctx, int x, int x0, float alpha, float beta, float *out);
/* max over owned interior cells of max(|u|,|v|) */
int fluid_absmax_velocity(fluid_ctx *ctx, int u, int v, float *out);

/* ---- ensemble diagnostics: looking at an ensemble without taking it apart ---------------------------------
 * M = fluid_members(ctx); all arrays are host memory; every call is synchronous like fluid_residual unless said
 * otherwise; none alters what a later download or step sees (a field's lazy state is settled first, as by
 * fluid_residual, not lost).  The launch count of a call does not depend on M: one kernel per maxima call, two per
 * moments or Gram call, one per statistics call.  Results and scratch are library-owned and outside the arena,
 * allocated at the first call that needs them (the two statistics fields: 2 x field_floats floats) and freed by
 * fluid_destroy; an allocation that fails is FLUID_E_NOMEM and leaves the context usable.
 *
 * Definitions:
 * - fluid_residual_members, fluid_absmax_velocity_members: out[m] = what fluid_residual / fluid_absmax_velocity return
 *   on a one-member context that holds member m's fields, with alpha[m], beta[m] as its coefficients: bit for bit.  The
 *   arithmetic of the scalar calls (|beta*x - alpha*(((L+R)+U)+D) - x0| in float, fmaxf from 0, NaN cells skipped, never
 *   NaN), one result word per member.  A member full of NaN or inf changes no other member's value.  With equal
 *   coefficients for all members, max(out) == fluid_residual(...), exactly.
 * - fluid_member_moments: per member, over the interior cells (rows and columns 1..N): sum[m] = sum of x, sumsq[m] = sum
 *   of x*x, accumulated in double from the stored values widened exactly (x*x is exact in double).  No floating-point
 *   atomics and a fixed order: per-block partial sums stored to a scratch buffer, folded by a second small kernel.  So
 *   the result is the same bits call after call and process after process for the same data, N, M, storage type.
 *   Exactness follows where it can: when every partial sum is representable (dyadic data) the result is the exact sum.
 *   Either pointer may be null, not both.
 * - fluid_ensemble_stats: across the members, per cell, ghost cells included: mean and population variance of a field,
 *   as float fields.  Per cell, all in IEEE double with no contraction: s = (double)x_0; s += (double)x_m for
 *   m = 1 .. M-1 in member order (starting from member 0's value, not from 0.0, so a cell that is -0 in every member has
 *   mean -0); mean_d = s / (double)M; mean = (float)mean_d; d_m = (double)x_m - mean_d; q = d_0*d_0; q += d_m*d_m in
 *   member order; variance = (float)(q / (double)M).  Two passes over the members on purpose: the one-pass form
 *   sum(x^2) - (sum x)^2 / M loses the variance of a field whose spread is small against its mean.  M = 1: the mean is
 *   the field, the variance +0 (NaN where the field is not finite).
 *   mean / variance: host (N+2)^2 arrays in the reference's dense layout, or null.  Both null: the results are only
 *   computed (enqueued on the context's stream, no wait) and stay on the device.
 * - fluid_ensemble_stats_ptr: device addresses of the two library-owned result fields (always float, layout of
 *   fluid_layout(): pitch, xoff; pad columns zero), holding the results of the last fluid_ensemble_stats until the next
 *   one or fluid_destroy.  FLUID_E_INVALID before the first.
 * - fluid_member_gram: the M x M matrix of inner products between the members of a field, or between their anomalies
 *   about the ensemble mean: G = A^T A, what inflation, recentring, an ensemble-space Kalman update, snapshot POD or a
 *   member-similarity check compute the matrix of fluid_transform_members from.  `gram`: M*M doubles.
 *    1. x_k[i][j] is the float fluid_pack_members would show for member k right before the call: the field's lazy state is
 *       settled first, as for fluid_residual, and nothing a later step or download sees is altered; with fp16 storage each
 *       value is widened exactly and a pressure scale divided back in float, exactly as the pack does.
 *    2. centre == 0: a_k = (double)x_k.  centre != 0, per cell: mean_d is exactly the mean_d of fluid_ensemble_stats --
 *       s = (double)x_0; s += (double)x_m for m = 1 .. M-1 in member order; mean_d = s / (double)M, IEEE double, no
 *       contraction -- and a_k = (double)x_k - mean_d, one rounding.  The subtraction is done per cell before any product,
 *       on purpose: the identity G - (G 1)(1^T G) / (M 1^T G 1) loses a spread that is small against the mean, as the
 *       one-pass variance does.
 *    3. gram[k*M + m] = the sum over the interior cells (rows and columns 1..N, as for the moments: the ghost ring is a
 *       mirror and takes no part) of a_k * a_m, accumulated in double.  centre == 0: every product is exact in double
 *       (24 + 24 bits).  centre != 0: a product may be fused into the addition or rounded on its own.
 *    4. No floating-point atomics, no matrix instructions; the order of every addition is fixed by (N, M, storage type,
 *       centre) alone: per-block partial matrices stored to a scratch buffer, folded by a second small kernel in index
 *       order, as for the moments.  So the result is the same bits call after call, context after context, process after
 *       process; and when every partial sum is representable (dyadic data) it is the exact sum.  Every sum starts from
 *       its first term, not from 0.0: a sum that is zero has the sign IEEE addition gives it in that order.
 *    5. gram[k*M + m] and gram[m*M + k] are the same bits: one triangle is computed and mirrored.
 *    6. centre == 0: a non-finite value in member k poisons row k and column k only; every other entry keeps the bits it
 *       has without it.  centre != 0: the mean of such a cell is non-finite, and so is EVERY entry.
 *    7. M = 1: the one entry is the sum of squares; with centre, +0 (NaN if the field is not finite).
 *   M in [1, FLUID_TRANSFORM_MAX_MEMBERS] (below): the consumer of G is the transform, which has that cap, and M*M doubles
 *   per block partial stop being small beyond it.  At most two kernels per call whatever M is (partials, fold).
 * - fp16 storage: every value is widened exactly; results stay float / double.  All calls see a field as
 *   fluid_download_member would show it right after the call (the fp16 pressure scale and pending increments are settled
 *   first, as for fluid_residual).
 * Refusals, all FLUID_E_INVALID with a message that names the call (and the member for a bad entry), found before
 * anything is launched or any state changes: null context, null output where one is required, bad field id, a
 * non-finite alpha[m] / beta[m] (x == x0 is no error, as in fluid_residual).  On a context with one member the two
 * _members maxima are the scalar calls with element 0, row slabs included.  fluid_member_moments, fluid_member_gram,
 * fluid_ensemble_stats and fluid_ensemble_stats_ptr are refused on row slabs (nranks > 1): a sum over ranks needs an
 * exchange kind the callback contract does not have.  fluid_member_gram also refuses M > FLUID_TRANSFORM_MAX_MEMBERS (the
 * message gives both numbers), and finds a null `gram` before the context is looked at.  fluid_residual and
 * fluid_absmax_velocity keep returning the maximum over the members.  The launches of the moments, the Gram matrix and
 * the statistics belong to none of the fluid_timing categories. */
int fluid_residual_members(fluid_ctx *ctx, int x, int x0, const float *alpha, const float *beta, float *out);
int fluid_absmax_velocity_members(fluid_ctx *ctx, int u, int v, float *out);
int fluid_member_moments(fluid_ctx *ctx, int field, double *sum, double *sumsq);
int fluid_ensemble_stats(fluid_ctx *ctx, int field, float *mean, float *variance);
int fluid_ensemble_stats_ptr(fluid_ctx *ctx, void **mean_dev, void **variance_dev);
int fluid_member_gram(fluid_ctx *ctx, int field, int centre, double *gram);

/* ---- moving ensembles: device pack / unpack, bulk host copies, recorded runs -------------------------------
 * M = fluid_members(ctx), W = N + 2.  A DENSE array is always float, one member after the other, each member the
 * reference's W*W row-major array with its ghost ring; member m starts m * member_stride floats behind the base pointer.
 * Dense device arrays need 4-byte alignment only.  All six calls work on a one-member, one-GPU context with M = 1.
 *
 * - fluid_pack_members / fluid_unpack_members: members [first, first + count) of one field <-> a dense DEVICE array, one
 *   kernel launch whatever the count, enqueued on the context's stream, no wait.  count = 0: from `first` to the end.
 *   member_stride = 0: W*W; any other value must be at least W*W (the floats between two members are not touched).
 *   pack writes what fluid_download_member would show right after the call, bit for bit: whatever the library still owes
 *   the field is settled first (zeros by definition, a pending increment, a deferred source), and with fp16 storage the
 *   values are widened exactly and the pressure scale is divided back in float, exactly.  Nothing a later step or download
 *   sees is altered.  unpack stores narrow(dense): with fp16 storage one rounding to nearest even, the same bits
 *   fluid_upload_member's host conversion stores.  An unpack of ALL members replaces the field: nothing is settled first,
 *   whatever the field still owed itself is dropped.  An unpack of a proper sub-range first settles the field for all
 *   members, as fluid_upload_member does, then overwrites the range.  The pad columns of the device layout are neither
 *   read nor written.  The dense memory belongs to the library until the stream has run the launch (fluid_synchronize,
 *   or work of the caller's ordered behind it on the stream given to fluid_create_ex).
 * - fluid_download_members / fluid_upload_members: all members <-> a host array of M*W*W floats, synchronous, ONE wait.
 *   They go through a library-owned dense staging buffer on the device (outside the arena: fluid_arena_bytes_ensemble is
 *   unchanged; allocated by the first such call, freed by fluid_destroy; a failed allocation is FLUID_E_NOMEM and leaves
 *   the context usable) of g = max(1, min(M, 64 MiB / (W*W*4))) members, ceil(M / g) groups in stream order.  Results are
 *   those of M fluid_download_member / fluid_upload_member calls, bit for bit.
 * - fluid_run / fluid_run_members: plan->nsteps steps without the host in the loop, defined as this sequence of existing
 *   calls, bit for bit in every field of every member.  Per step, with plan->sources set: fluid_unpack_members of its three
 *   blocks into U_PREV, V_PREV, DENS_PREV, then fluid_step_members(.., iters, 1, 1) -- a forced run: fluid_step alone zeroes
 *   the sources of every step but the first; without: fluid_step_members with use_sources for the first step only.  After
 *   every `every`-th step: fluid_pack_members of each listed field into its slot of `snapshots`.  No wait anywhere.
 *   *snapshots_written (may be null) = every ? nsteps / every : 0.  fluid_run_members gives each member its own dt, diff,
 *   visc (host arrays of M values, as for fluid_step_members).
 * Refusals, all FLUID_E_INVALID with a message that names the call, found before anything is launched or any state
 * changes, null pointers before the device is touched: null context, device or host pointer, or plan; bad field id;
 * first / count outside [0, M]; a stride below W*W; odd or negative iters; negative nsteps or every; every > 0 with
 * nfields outside [1, 12], null fields / snapshots, or a capacity below snapshots * nfields * M * W*W floats; a non-finite
 * dt[m] / diff[m] / visc[m] (the member is named); a device pointer that is not device memory of the context's device, or
 * whose needed extent does not lie inside one allocation (asked of the runtime on the host: a wrong pointer never reaches
 * a kernel).  On row slabs (nranks > 1) all six calls are refused, as the moments are.
 * The launches belong to none of the fluid_timing categories. */
int fluid_pack_members(fluid_ctx *ctx, int field, int first, int count, void *dst_dev, size_t member_stride);
int fluid_unpack_members(fluid_ctx *ctx, int field, int first, int count, const void *src_dev, size_t member_stride);
int fluid_download_members(fluid_ctx *ctx, int field, float *host);
int fluid_upload_members(fluid_ctx *ctx, int field, const float *host);
typedef struct fluid_run_plan {
    int iters, nsteps, use_sources;
    const void *sources;   /* device, dense [3][M][W*W]: u_prev, v_prev, dens_prev, written before EVERY step, which consumes
                              them (use_sources is then taken as 1 for every step); NULL: fluid_step's rule */
    int every;             /* a snapshot after every `every`-th step; 0: none */
    const int *fields;     /* what a snapshot holds: nfields field ids (host memory) */
    int nfields;
    void *snapshots;       /* device, dense [snapshot][field][member][W*W] */
    size_t capacity;       /* floats behind `snapshots` */
} fluid_run_plan;
int fluid_run(fluid_ctx *ctx, float dt, float diff, float visc, const fluid_run_plan *plan, int *snapshots_written);
int fluid_run_members(fluid_ctx *ctx, const float *dt, const float *diff, const float *visc, const fluid_run_plan *plan,
                      int *snapshots_written);

/* ---- coarse snapshots: block-averaged pack, download, recorded runs ------------------------------------------
 * W = N + 2.  A COARSE FACTOR r is one of 1, 2, 4, 8, 16, 32, 64 and must divide W; C = W / r.  The r x r blocks tile the
 * whole W x W array of a member, ghost ring included -- the array a dense pack writes.  r = 1 is the dense pack, bit for bit.
 * Coarse cell (I, J) of a member is defined from the values x[i][j] that fluid_download_member would show right after the
 * call, in IEEE double with no contraction:
 *  1. per row i of the block, the r values (double)x[i][rJ .. rJ + r - 1] are summed as a pairwise tree over adjacent
 *     columns: level 1 adds columns (0, 1), (2, 3), ..; level 2 adds those results pairwise; log2 r levels give p_i;
 *  2. s = p_0, then s += p_i for i = 1 .. r - 1 in row order -- from p_0, not from 0.0: a block of -0 has the mean -0;
 *  3. out = (float)(s * 2^(-2 log2 r)): the scaling is exact, there is ONE rounding to float, float denormals are kept.
 * With fp16 storage each element is widened exactly and the pressure scale divided back in float, exactly as
 * fluid_pack_members does it, before step 1.  The order is part of the contract: the same bits on every call, for every
 * member count and launch shape; no floating-point atomics.  A NaN or inf poisons only the coarse cells whose block holds it.
 * A COARSE DENSE array is float, member after member, each C*C row-major; member m starts m * member_stride floats behind
 * the base (0: C*C; otherwise at least C*C); 4-byte alignment.
 *
 * - fluid_coarse_size: host logic, no device: *side = (N + 2) / factor.
 * - fluid_pack_members_coarse: everything fluid_pack_members promises -- one kernel launch whatever the count and factor,
 *   on the context's stream, no wait; the field's lazy state is settled first and nothing a later step or download sees is
 *   altered; the floats between two members and everything outside the members' C*C cells are not touched.
 * - fluid_download_members_coarse: all members into a host array of M*C*C floats, synchronous, ONE wait, through the
 *   staging buffer of fluid_download_members (no second buffer), each group as many coarse members as fit in it.
 * - fluid_run_coarse / fluid_run_members_coarse: fluid_run / fluid_run_members in every respect, except that each snapshot
 *   pack is a fluid_pack_members_coarse with `factor`: plan->snapshots is laid out [snapshot][field][member][C*C], and
 *   plan->capacity and its check count coarse floats.  plan->sources stays full resolution.
 * Refusals, all FLUID_E_INVALID with a message that names the call, found before anything is launched or any state
 * changes: those of the dense calls (null context, device pointer, host pointer or plan -- null pointers before the
 * context is looked at; bad field id; first / count out of range; row slabs), a factor that is not one of the seven
 * values, a factor that does not divide N + 2 (fluid_coarse_size: also N < 1; its message names N, the factor and the rule
 * broken), a stride below C*C, a device extent that does not hold the coarse span (asked of the runtime on the host).
 * The launches belong to none of the fluid_timing categories. */
int fluid_coarse_size(int N, int factor, int *side);
int fluid_pack_members_coarse(fluid_ctx *ctx, int field, int first, int count, int factor, void *dst_dev, size_t member_stride);
int fluid_download_members_coarse(fluid_ctx *ctx, int field, int factor, float *host);
int fluid_run_coarse(fluid_ctx *ctx, float dt, float diff, float visc, const fluid_run_plan *plan, int factor,
                     int *snapshots_written);
int fluid_run_members_coarse(fluid_ctx *ctx, const float *dt, const float *diff, const float *visc,
                             const fluid_run_plan *plan, int factor, int *snapshots_written);

/* ---- recombining ensembles: every new member a linear combination of the old ones, in place ---------------------
 * M = fluid_members(ctx), W = N + 2.  Branching a Monte-Carlo set from one member, replacing a member by a copy of
 * another, resampling, inflation, recentring, an ensemble-space Kalman update: X' = X T with an M x M matrix T, per cell.
 *
 * - fluid_transform_members: `weights` is host memory, M*M floats; weights[k*M + m] is the weight of OLD member k in NEW
 *   member m.  `fields`: nfields distinct field ids, host memory.  One kernel launch per listed field whatever M is,
 *   enqueued on the context's stream, no wait; both host arrays belong to the caller again when the call returns.
 *   Definition -- per listed field, per cell of the W x W array (ghost ring included), per new member m; pad columns are
 *   neither read nor written:
 *    1. x_k is the float fluid_pack_members would show for old member k right before the call: the field's lazy state is
 *       settled first; with fp16 storage each value is widened exactly and a pressure scale divided back in float, exactly
 *       as the pack does.
 *    2. The terms are the k in increasing order with weights[k*M + m] != 0.  A zero weight of either sign takes no part:
 *       a NaN or inf member with weight 0 poisons nobody.
 *    3. With no term, y = +0.0f.
 *    4. Otherwise s = (double)x_k * (double)w_k for the first term, then s = s + (double)x_k * (double)w_k for each further
 *       term in member order, and y = (float)s: ONE rounding to nearest even; float denormals are kept, overflow goes to
 *       +-inf.  Every product is exact in double (24 + 24 significand bits fit in 53, the exponent range is ample), so a
 *       fused and an unfused multiply-add give the same bits -- which is why the weights are float and not double.
 *    5. Every new member's cell is stored as fluid_unpack_members of ALL members would store y: narrow(y), with fp16
 *       storage one more rounding to nearest even.  Afterwards the field holds plain values (scale 1) and owes itself
 *       nothing.
 *    6. All M old values of a cell are read before any new value of that cell is stored: the call is in place and means
 *       what an out-of-place one would.
 *    7. A NaN result is a NaN; its sign and payload are not specified.
 *   The order is part of the contract: the same bits on every call, for every launch shape; no matrix instructions, no
 *   atomics.  The ghost ring is transformed cell by cell like the interior: ghost columns and rows stay the exact +-mirror
 *   of their neighbours (rounding is symmetric), the corners need not; fluid_op_set_bnd restores them for a caller who
 *   wants that.
 * - fluid_select_members: new member m := old member source[m], every source[m] in [0, M) (host memory).  It IS
 *   fluid_transform_members with the one-hot matrix, in the same body: new members are bit copies for every non-NaN value,
 *   -0 included.  Branch-from-one, resampling and permutation, in place.
 * Any M in [1, FLUID_TRANSFORM_MAX_MEMBERS] works, one-member contexts included.  Above that the accumulators of a cell no
 * longer fit the register file: fluid_pack_members -> outside code -> fluid_unpack_members remains the route there.
 * The weight tables are library-owned device and pinned memory outside the arena (fluid_arena_bytes_ensemble is unchanged),
 * allocated by the first such call and freed by fluid_destroy; a failed allocation is FLUID_E_NOMEM and leaves the context
 * usable.  Successive calls with different weights need no wait.
 * Refusals, all FLUID_E_INVALID with a message that names the call and, where it applies, the k, m or list position, found
 * before anything is launched or any state changes, null pointers before the context is looked at: a null `fields`,
 * `weights` or `source`, a null context; nfields outside [1, 12]; a bad field id; a field listed twice; a non-finite
 * weight; a source[m] outside [0, M); M > FLUID_TRANSFORM_MAX_MEMBERS (the message gives both numbers); row slabs.
 * The launches belong to none of the fluid_timing categories. */
#define FLUID_TRANSFORM_MAX_MEMBERS 64
int fluid_transform_members(fluid_ctx *ctx, const int *fields, int nfields, const float *weights);
int fluid_select_members(fluid_ctx *ctx, const int *fields, int nfields, const int *source);

/* ---- observing ensembles: point samples of every member, and their Gram matrix -----------------------------------
 * M = fluid_members(ctx); x[i][j] = row i, column j of a member.  A Kalman-type update, a particle-filter weight or a
 * time series from probes need the members as an instrument sees them: H x_m at P points, P a few to 10^5 against N*N
 * cells.  The network of points is resident; "step -> observe -> M x M algebra on the host -> fluid_transform_members" is
 * an assimilation cycle that never takes the ensemble apart.
 *
 * - fluid_set_observation_points: `col`, `row` are host arrays of npoints floats, positions in cell-index coordinates:
 *   cell centres at the integers 1..N, the walls at 0.5 and N + 0.5.  Every coordinate must be finite and lie in
 *   [0.5, N + 0.5], the range the reference's advection clamps a back-trace to (FluidSequential.c:120-123).  The points
 *   are validated on the host and kept in library-owned device memory outside the arena (fluid_arena_bytes_ensemble is
 *   unchanged; 32 bytes per point), freed by fluid_destroy.  The call replaces the previous network; npoints = 0 clears it
 *   and frees the memory (the arrays may then be null).  It may wait for the stream; both arrays are the caller's again on
 *   return.  A failed allocation is FLUID_E_NOMEM and leaves the context usable and the old network in place.
 * - fluid_observation_points: *npoints = P, 0 when no network is set.
 * - The observation h_k[p] of member k at point p = (col, row), ONE definition for all calls, in float with no contraction
 *   -- the interpolant of the solver's own advection:
 *       j0 = (int)col;  i0 = (int)row;
 *       s1 = col - (float)j0;  s0 = 1.0f - s1;
 *       t1 = row - (float)i0;  t0 = 1.0f - t1;
 *       h  = s0 * (t0 * x[i0][j0]   + t1 * x[i0+1][j0])
 *          + s1 * (t0 * x[i0][j0+1] + t1 * x[i0+1][j0+1]);
 *   The taps are the values fluid_pack_members would show right before the call: the field's lazy state is settled first,
 *   as for fluid_member_gram, and nothing a later step or download sees is altered; with fp16 storage each tap is widened
 *   exactly and the pressure scale divided back in float, as the pack does.  The ghost ring is read like any cell; j0 and
 *   i0 are at most N, so every tap exists.  A point at a cell centre returns that cell's value when all four taps are
 *   finite (a zero that results may be +0).  A non-finite tap makes the observation non-finite even under a zero weight,
 *   as in the reference's advect: it affects only that member and only the points whose 2 x 2 stencil holds it.
 * - fluid_observe_members: out_dev[m * member_stride + p] = h_m[p], a dense DEVICE array.  member_stride = 0: P; any other
 *   value must be at least P (the floats in between are not touched).  One kernel launch whatever M and P are, on the
 *   context's stream, no wait.  Any M up to 21845; row and member offsets are 64-bit.
 * - fluid_observe_members_host: the same values into a host array of M*P floats, synchronous, ONE wait, through the
 *   staging buffer of fluid_download_members (no second buffer), in groups of members when M*P exceeds it.
 * - fluid_observation_gram: the observation-space counterpart of fluid_member_gram -- what an ensemble-space update (ETKF,
 *   EnKF) computes its matrix from.  `obs`: P observed values y_p, or null; `inv_sigma`: P values s_p = 1 / sigma_p, or
 *   null for 1.0; both host arrays.  `gram`: M*M doubles; `rhs`: M doubles or null; `dd`: one double or null.
 *    1. h_k[p] as above.
 *    2. centre != 0: mean_d[p] is the member-order chain of fluid_ensemble_stats: s = (double)h_0, then s += (double)h_m
 *       for m = 1 .. M-1, then mean_d = s / (double)M.  centre == 0: mean_d = 0 and the subtraction is skipped.
 *    3. a_k[p] = ((double)h_k - mean_d) * (double)s_p;  d[p] = ((double)y_p - mean_d) * (double)s_p; each operation rounds
 *       once.  A multiplication by 1.0 is exact: a null inv_sigma gives the bits that all ones give.
 *    4. gram[k*M + m] = sum over p of a_k * a_m;  rhs[k] = sum over p of a_k * d;  *dd = sum over p of d * d; accumulated
 *       in double, a product fused into the addition or rounded on its own.  rhs and dd may be null; they MUST be null
 *       when obs is null.
 *    5. No floating-point atomics, no matrix instructions: per-block partials go to library-owned scratch and are folded
 *       by a second small kernel in index order; at most two launches.  The order of every addition is fixed by P, M,
 *       centre and whether obs is given: the same bits call after call and process after process, and the exact sum when
 *       every partial sum is representable.  Every sum starts from its first term.
 *    6. gram is bit-symmetric: one triangle is computed and mirrored.
 *    7. centre == 0: a non-finite h_k poisons row k, column k and rhs[k] only; a non-finite y_p poisons rhs and dd only.
 *       centre != 0: a non-finite h_k at a point poisons everything.
 *    8. M in [1, FLUID_TRANSFORM_MAX_MEMBERS].
 *   Synchronous like fluid_member_gram: two kernels, one copy of M*M + M + 1 doubles (padded), one wait.
 * Refusals, all FLUID_E_INVALID with a message that names the call and, where it applies, the point index or the member,
 * found before anything is launched or any state changes, null pointers before the context is looked at: a null context;
 * a null required pointer (col, row with npoints != 0; npoints; out_dev; host; gram); rhs or dd given with obs null; a bad
 * field id; npoints outside [0, FLUID_OBSERVE_MAX_POINTS]; a coordinate that is not finite or lies outside
 * [0.5, N + 0.5]; no network set, for the three observing calls; a stride below P; a device pointer that is not device
 * memory of the context's device or whose extent does not lie inside one allocation (asked of the runtime on the host,
 * as for a pack); a non-finite inv_sigma[p], named by its index; M > FLUID_TRANSFORM_MAX_MEMBERS for the Gram call (the
 * message gives both numbers); row slabs (nranks > 1), for all five calls.
 * The launches belong to none of the fluid_timing categories. */
#define FLUID_OBSERVE_MAX_POINTS (1 << 20)
int fluid_set_observation_points(fluid_ctx *ctx, const float *col, const float *row, int npoints);
int fluid_observation_points(fluid_ctx *ctx, int *npoints);
int fluid_observe_members(fluid_ctx *ctx, int field, void *out_dev, size_t member_stride);
int fluid_observe_members_host(fluid_ctx *ctx, int field, float *host);
int fluid_observation_gram(fluid_ctx *ctx, int field, int centre, const float *obs, const float *inv_sigma,
                           double *gram, double *rhs, double *dd);

/* ---- typed networks: observation points that each observe their own field -----------------------------------------------
 * A real network on a fluid is mixed: density probes in one place, u and v probes in another.  The matrix of a filter is
 * the sum over ALL its points, of whatever variable: C = sum over p of w_p a_k[p] a_m[p].  A TYPED network gives every point
 * the field it observes, and the five observing calls then read each point from its own field in ONE call.
 *
 * - fluid_set_observation_network is fluid_set_observation_points in every respect -- the same validation of `col` and
 *   `row`, it replaces the previous network, npoints = 0 clears it, a failed allocation is FLUID_E_NOMEM and keeps the old
 *   network, it invalidates the point lists of the lattice calls -- with one addition: `field`, a host array of npoints field
 *   ids in [0, FLUID_NFIELDS), field[p] the field that point p observes.  The network is then typed; its table takes 33
 *   bytes per point, against the 32 of an untyped one.  A null `field` makes the call identical to
 *   fluid_set_observation_points: the network is untyped, as every network set through that call is.
 * - fluid_observation_network_fields: bit f of *mask is set when some point observes field f; *mask = 0 for an untyped
 *   network and when no network is set.  Host logic only.
 * - FLUID_FIELD_OF_POINT for `field` in fluid_observe_members, fluid_observe_members_host, fluid_observation_gram,
 *   fluid_observation_gram_lattice and fluid_analyse_lattice, on a typed network: in rule 1 of each definition h_k[p] is the
 *   same bilinear sample, operation for operation, taken from field field[p] -- the taps are what fluid_pack_members would
 *   show for THAT field.  Everything after rule 1 is untouched: the mean chain over the members at the point, 1 / sigma,
 *   the innovation, the chunks of 64 points and the wave order, the folds, the lattice weights and lists (which do not
 *   depend on the fields: the cache is kept), the solve and the update.  The order of every addition is unchanged: it is
 *   still fixed by the point index, so the results also depend on the per-point fields, and on nothing else that is new.
 * - Every distinct field of the network is settled first, as a pack settles it (zeros by definition, a pending increment,
 *   a deferred source); fields that no point observes are not touched, and nothing a later step or download sees is altered.
 *   With fp16 storage each field that is held at a pressure scale keeps it, and its taps are divided back in float by that
 *   field's OWN scale: the per-field scale of one launch may differ from point to point.
 * - A concrete field id on a typed network behaves exactly as on an untyped network with the same positions: all points
 *   sample that field and the per-point fields are ignored.  On untyped networks nothing changes, bit for bit; those calls
 *   launch kernels without any per-point lookup.
 * - Poisoning.  centre == 0: a non-finite value in member k of field f poisons row k, column k and rhs[k] only, and only
 *   through points that observe f and whose 2 x 2 stencil holds the value -- for the lattice calls only in the nodes those
 *   points take part in.  centre != 0: as before, through such points only.
 * Refusals, all FLUID_E_INVALID with a message that names the call, found before anything is launched or changed, null
 * pointers before the context is looked at: everything fluid_set_observation_points refuses, under
 * fluid_set_observation_network's name; a field[p] outside [0, FLUID_NFIELDS) (the message names p and the value);
 * FLUID_FIELD_OF_POINT with an untyped network (the message says that a typed network is needed) or with no network (the
 * message of the call as before); a null `mask`; a null context; row slabs.  Any other negative or too-large field id is
 * the "bad field id" refusal as before. */
#define FLUID_FIELD_OF_POINT (-2)
int fluid_set_observation_network(fluid_ctx *ctx, const float *col, const float *row, const int *field, int npoints);
int fluid_observation_network_fields(fluid_ctx *ctx, unsigned *mask);

/* ---- localised updates: the increment of a transform under a per-cell taper, over a box of cells ------------------
 * M = fluid_members(ctx), W = N + 2.  With at most FLUID_TRANSFORM_MAX_MEMBERS members against N*N states a global
 * ensemble update is rank-deficient and full of spurious long-range covariances; every practical scheme (LETKF, EnSRF)
 * lets a batch of nearby observations change the state only inside a compactly supported taper around it:
 *     X' = X + g o (X D)
 * per cell, X the ensemble there, D an M x M matrix, g the taper's value at the cell.  One local analysis is
 * fluid_observation_gram -> M x M algebra on the host -> fluid_taper_gaspari_cohn -> fluid_transform_members_local, and the
 * last call costs what the taper's support costs, not what the grid costs.
 *
 * - fluid_transform_members_local: `increments` is host memory, M*M finite floats; increments[k*M + m] is the weight of
 *   OLD member k in the INCREMENT of new member m: an ensemble transform T is D = T - I, formed by the caller (D and not T
 *   keeps every product exact, step 3).  `fields`: nfields distinct field ids, host memory.  `taper_dev`: a dense DEVICE
 *   array of W*W floats, row-major with the ghost ring -- the layout of one member of a dense pack -- shared by all members
 *   and all listed fields, aligned to 4 bytes; null: g = 1 everywhere.  `box`: host memory, four ints {row_lo, row_hi,
 *   col_lo, col_hi}, half-open ranges inside [0, W]; cells outside the box are neither read nor written and the taper is
 *   not read there; null: the whole W x W array.  An empty box is legal: nothing is launched, the fields are still settled.
 *   One kernel launch per listed field whatever M is, its grid the box, enqueued on the context's stream, no wait; the host
 *   arrays belong to the caller again when the call returns, the taper when the stream has passed the launches.  The table
 *   of increments travels through the ring of fluid_transform_members: successive calls with different matrices need no
 *   wait.
 *   Definition -- per listed field, per cell of the box, per new member m; pad columns are neither read nor written:
 *    1. The field's lazy state is settled for all members first, as fluid_pack_members settles it: x_k is the float the
 *       pack would show for old member k right before the call.  With fp32 storage, and with fp16 storage wherever the
 *       field holds plain values (scale 1), that is the stored value widened exactly.  An fp16 field held at a pressure
 *       scale KEEPS it -- dividing it back would be a pass over the whole grid and would round the half denormals of the
 *       cells outside the box -- and x_k is the stored value widened exactly and divided by the scale in float, exactly, as
 *       the pack does.  Cells the call does not store keep their bits and show what the pack showed before the call.
 *    2. The terms are the k in increasing order with increments[k*M + m] != 0.  A zero of either sign takes no part: a NaN
 *       or inf member with increment 0 poisons nobody.  With no term at all, member m is stored nowhere.
 *    3. s_m = (double)x_k * (double)d_k for the first term, then s_m = s_m + (double)x_k * (double)d_k for each further term
 *       in member order.  Every product is exact in double (24 + 24 significand bits), so a fused and an unfused
 *       multiply-add give the same bits, as in fluid_transform_members.
 *    4. g = the taper at the cell (null taper: 1).  g == 0, of either sign: the cell is unchanged in every member -- not
 *       stored, whatever s_m is, non-finite included.
 *    5. Otherwise p = (double)g * s_m, rounded once; y_d = (double)x_m + p, rounded once, the two NOT contracted into one
 *       fused operation; y = (float)y_d.  g = 1 makes p exact.
 *    6. The store is narrow(y): with fp16 storage one more rounding to nearest even, as fluid_unpack_members does.  In a
 *       field held at a scale s (a power of two) the half narrow(y) is stored times s, so that the pack shows narrow(y):
 *       exact, unless |narrow(y)| * s exceeds 65504, the range the library itself keeps that field in; then +-inf.
 *    7. All M old values of a cell are read before any new value of that cell is stored: the call is in place and means
 *       what an out-of-place one would.
 *    8. A NaN result is a NaN; its sign and payload are not specified.  A non-finite g gives non-finite results in that
 *       cell only.
 *   The order is part of the contract: the same bits for every launch shape; no atomics, no matrix instructions.  The
 *   ghost ring is a cell like any other where the box includes it.  M in [1, FLUID_TRANSFORM_MAX_MEMBERS].
 * - fluid_taper_gaspari_cohn: writes the whole dense W x W array `out_dev` (the layout `taper_dev` has), zeros outside the
 *   support, in one launch on the context's stream, no wait.  `col`, `row`: the centre, in the cell-index coordinates of
 *   fluid_set_observation_points, finite and in [0.5, N + 0.5]; `c`: the half-width, finite and > 0; the support is r < 2,
 *   a disc of radius 2c.  Per cell (i, j), in IEEE double, every operation rounded once and none contracted:
 *       dx = (double)j - (double)col;  dy = (double)i - (double)row;
 *       r  = sqrt(dx*dx + dy*dy) / (double)c;
 *       r <= 1:     g = ((((-0.25*r + 0.5)*r + 0.625)*r - 5.0/3.0)*r)*r + 1.0;
 *       1 < r < 2:  g = ((((((1.0/12.0)*r - 0.5)*r + 0.625)*r + 5.0/3.0)*r - 5.0)*r + 4.0) - (2.0/3.0)/r;
 *       r >= 2:     g = 0 exactly;
 *   (Horner's rule, innermost parenthesis first; 5.0/3.0, 1.0/12.0 and 2.0/3.0 are the doubles nearest the quotients) --
 *   the Gaspari-Cohn fifth-order function 1 - 5r^2/3 + 5r^3/8 + r^4/2 - r^5/4 and 4 - 5r + 5r^2/3 + 5r^3/8 - r^4/2 + r^5/12
 *   - 2/(3r).  Then g is clamped to [0, 1] and rounded to float.  g is 1 at a centre that sits on a cell.
 *   `box` (may be null) receives four ints as fluid_transform_members_local takes them, computed on the host by the same
 *   function: it contains every cell with g != 0, and is at most one cell larger on each side than the tight box of the
 *   cells with r < 2 (clipped to the array); {0, 0, 0, 0} when no cell has r < 2.
 * Refusals, all FLUID_E_INVALID with a message that names the call and, where it applies, the k, m, list position or box
 * entry, found before anything is launched or any state changes, null pointers before the context is looked at: a null
 * `fields`, `increments` or `out_dev`, a null context; nfields outside [1, 12]; a bad field id; a field listed twice; a
 * non-finite increment; a box entry outside [0, W] or a lo above its hi; M > FLUID_TRANSFORM_MAX_MEMBERS (the message
 * gives both numbers); row slabs; a `col`, `row` or `c` that is not finite or out of range; a device pointer that is not
 * device memory of the context's device or whose W*W floats do not lie inside one allocation (asked of the runtime on the
 * host, as for a pack).
 * The launches belong to none of the fluid_timing categories. */
int fluid_transform_members_local(fluid_ctx *ctx, const int *fields, int nfields, const float *increments,
                                  const void *taper_dev, const int *box);
int fluid_taper_gaspari_cohn(fluid_ctx *ctx, float col, float row, float c, void *out_dev, int *box);

/* ---- lattice updates: increments given at the nodes of a coarse lattice, blended to every cell in one launch ----------
 * M = fluid_members(ctx), W = N + 2.  A localised filter (LETKF) computes an increment matrix D_b at each of many analysis
 * points, all from the SAME background ensemble, and wants
 *     X' = X + sum over b of phi_b o (X D_b)
 * with every product taken on the old X.  A sequence of fluid_transform_members_local calls cannot say that: the calls are
 * in place, so where two tapers overlap the second multiplies what the first already changed, and it costs one launch per
 * field per analysis point.  The remedy is weight interpolation (Yang et al. 2009): D at the nodes of a coarse lattice,
 * interpolated bilinearly to every cell -- here in one launch per field.
 *
 * - fluid_transform_members_lattice: `increments` is host memory, nodes_row * nodes_col * M * M finite floats;
 *   increments[((a*nodes_col + b)*M + k)*M + m] is the weight of OLD member k in the INCREMENT of new member m at node
 *   (a, b): D = T - I per node, as in fluid_transform_members_local.  Node (a, b) sits on cell row row0 + a*step, column
 *   col0 + b*step; row0 and col0 may be any int, negative or past the array.  `step` is a positive multiple of 8: any
 *   8 x 8 patch of cells aligned to the lattice's origin then lies inside one lattice cell (the launch takes coarser
 *   patches where step allows; the bits do not depend on it).  nodes_row, nodes_col >= 1, nodes_row * nodes_col <=
 *   FLUID_LATTICE_MAX_NODES.  `fields`: nfields distinct field ids, host memory.  Every cell of the W x W array is covered,
 *   ghost ring included; there is no box and no taper.
 *   Definition -- per listed field, per cell (i, j), per new member m; pad columns are neither read nor written:
 *    1. The field's lazy state is settled for all members first, and x_k is read exactly as rule 1 of
 *       fluid_transform_members_local reads it: an fp16 field held at a pressure scale KEEPS it, values are read divided
 *       back and stored times the scale by that call's rule 6, with the same +-inf beyond 65504 / scale.
 *    2. Axis weights.  Along rows, with n = nodes_row, S = step, q = i - row0, in integer arithmetic:
 *         n == 1 or q <= 0:   a = 0,      t1 = 0;
 *         q >= (n-1)*S:       a = n - 2,  t1 = 1;
 *         otherwise:          a = q / S,  t1 = (double)(q - a*S) / (double)S, one rounding;
 *       t0 = 1.0 - t1, one rounding.  Columns are the same with nodes_col, col0, j, giving b, u0, u1.  Cells outside the
 *       lattice's hull take the nearest edge's weights: constant extrapolation.
 *    3. Corners, up to four, in row-major order of the absolute node index: (a, b), (a, b+1), (a+1, b), (a+1, b+1), with
 *       weights phi = t0*u0, t0*u1, t1*u0, t1*u1, each ONE double multiplication rounded once.  A corner past the lattice
 *       (n == 1 on that axis) does not exist.
 *    4. Node sums.  t_c = sum over k of (double)x_k * (double)d_c[k][m], over the k in increasing order with d_c[k][m] != 0,
 *       started from its first term; every product is exact in double, as in fluid_transform_members.  A zero of either
 *       sign takes no part.  A corner whose column m has no term has no t_c.
 *    5. A corner takes part when it exists, phi_c != 0 and t_c exists.  A corner with phi_c == 0 is not evaluated into
 *       the result, whatever it holds, inf and NaN included.  So a cell on a lattice line depends on that line's nodes
 *       only, and a cell on a node gets exactly fluid_transform_members_local's result for that node's D.
 *    6. Blend.  s = phi_c * t_c for the first corner that takes part; for each further one s = s + phi_c * t_c; product and
 *       sum are each rounded once and NOT contracted into one fused operation.
 *    7. y_d = (double)x_m + s, rounded once; y = (float)y_d; the store is narrow(y).  If no corner takes part for (cell,
 *       m), that cell of member m is not stored and keeps every bit.
 *    8. All M old values of a cell are read before any new value of that cell is stored: the call is in place and means
 *       what an out-of-place one would.
 *    9. A NaN result is a NaN; its sign and payload are not specified.
 *   The order is part of the contract: the same bits for every launch shape; no atomics, no matrix instructions.
 *   One kernel launch per listed field whatever M and the node count are, enqueued on the context's stream, no wait for
 *   the fields; increments without a single term anywhere launch nothing, and the fields are still settled.  The node
 *   tables -- the doubles the kernel reads and a word of non-zero bits per node and old member -- are library-owned
 *   device memory outside the arena with a pinned staging twin (fluid_arena_bytes_ensemble is unchanged), allocated or
 *   grown by the first call that needs the room and freed by fluid_destroy; a failed allocation is FLUID_E_NOMEM and
 *   leaves the context usable and nothing changed.  There is ONE table buffer: the device copy is ordered behind earlier
 *   launches by the stream, but a call may wait on an event until the lattice call before it has copied its tables out
 *   of the staging twin, and a call that grows the buffer waits for the stream.  `increments` belongs to the caller again
 *   when the call returns.  M in [1, FLUID_TRANSFORM_MAX_MEMBERS].
 * Refusals, all FLUID_E_INVALID with a message that names the call, found before anything is launched or any state
 * changes, null pointers before the context is looked at: a null `fields` or `increments`, a null context; nfields outside
 * [1, 12]; a bad field id; a field listed twice; M > FLUID_TRANSFORM_MAX_MEMBERS (the message gives both numbers); row
 * slabs; nodes_row or nodes_col below 1; more than FLUID_LATTICE_MAX_NODES nodes (the message gives both numbers); a step
 * below 8 or not a multiple of 8; a non-finite increment (the message names a, b, k and m).
 * The launches belong to none of the fluid_timing categories. */
#define FLUID_LATTICE_MAX_NODES 4096
int fluid_transform_members_lattice(fluid_ctx *ctx, const int *fields, int nfields, const float *increments, int nodes_row,
                                    int nodes_col, int row0, int col0, int step);

/* ---- lattice observations: the localised Gram matrix, right-hand side and innovation norm of every node, in one call ----
 * M = fluid_members(ctx), P = the resident network of fluid_set_observation_points, B = nodes_row * nodes_col.  The D_b of a
 * lattice update come from the Gram matrix of the observations near node b, weighted by a taper about b.  One
 * fluid_observation_gram call per node -- the taper folded into inv_sigma -- observes all P points in all M members B
 * times and waits B times; this call observes every point once and returns every node's matrices after ONE wait, in two
 * kernel launches whatever B, P and M are.  The lattice arguments are fluid_transform_members_lattice's, so result [a][b]
 * lines up with increments[a][b]: node (a, b) has index a * nodes_col + b and sits on cell row row0 + a*step, column
 * col0 + b*step; any int origin, `step` a positive multiple of 8, B <= FLUID_LATTICE_MAX_NODES.  `c`: the localisation
 * half-width, as in fluid_taper_gaspari_cohn, finite and > 0; a node's support is the disc of radius 2c.  All arrays are
 * host memory: `gram` B*M*M doubles, [node][k][m]; `rhs` B*M doubles or null; `dd` B doubles or null; `counts` B ints or
 * null; `obs`, `inv_sigma` as in fluid_observation_gram, P floats each, inv_sigma null for 1.0; rhs and dd MUST be null
 * when obs is null.  Synchronous like fluid_observation_gram.
 * Definition, per node:
 *  1. h_k[p], mean_d[p], a_k[p] and d[p] are exactly rules 1-3 of fluid_observation_gram: the same lazy state is settled
 *     first, fp16 taps are widened and the pressure scale divided back, the mean is over the members at the point whatever
 *     the node.  The operands of a point are the same in every node that sees it.
 *  2. The weight of point p at the node, in IEEE double, every operation rounded once and none contracted:
 *       dx = (double)col_p - (double)node_col;  dy = (double)row_p - (double)node_row;
 *       r  = sqrt(dx*dx + dy*dy) / (double)c;
 *     g = the Gaspari-Cohn value of fluid_taper_gaspari_cohn at r (the same function: the same Horner forms and constants,
 *     0 for r >= 2, clamped to [0, 1]);  w = (double)(float)g.
 *  3. A point takes part in a node when w != 0.  A point with w == 0 is not read for that node: a non-finite observation
 *     or obs value there poisons nothing of that node.
 *  4. Over the participating points: gram[k][m], k <= m, = sum of (w*a_k) * a_m;  rhs[k] = sum of (w*a_k) * d;  dd = sum of
 *     (w*d) * d.  w*a_k and w*d are rounded once; the second product is fused into the addition or rounded on its own.
 *     gram[m][k] is a copy of gram[k][m]: the matrix is bit-symmetric.
 *  5. counts[node] = the number of participating points.  A node with none has every entry of its matrix, its rhs and its
 *     dd equal to +0.0, and count 0.
 *  6. No floating-point atomics, no matrix instructions.  A node's points are taken in increasing point index in chunks of
 *     64, point i of a chunk by wave i mod 4, and the four waves' sums are added in wave order: the order of every addition
 *     is fixed by the network, the lattice arguments, c, M, centre and whether obs is given -- the same bits call after
 *     call and context after context, and the exact sum when every partial sum is representable.  Every sum starts from
 *     its first term.
 *  7. centre == 0: a non-finite h_k at a point poisons row k, column k and rhs[k] of the nodes the point takes part in, and
 *     nothing else; a non-finite y_p poisons rhs and dd of those nodes only.  centre != 0: a non-finite h_k at a point
 *     poisons every entry of those nodes, and no other node.
 *  8. M in [1, FLUID_TRANSFORM_MAX_MEMBERS].
 * Which points a node sees is found on the host at call time, from a host copy of the network's positions (8 bytes per
 * point) and the lattice geometry: only the nodes within 2c of a point are tried.  The lists -- (point index, float weight)
 * pairs per node --, the operands of the points ((M padded + 2) doubles per point) and the results are library-owned device
 * memory outside the arena with pinned twins (fluid_arena_bytes_ensemble is unchanged), allocated or grown by the first
 * call that needs the room and freed by fluid_destroy; a failed allocation is FLUID_E_NOMEM and leaves the context usable.
 * The lists are kept: a call with the same network, lattice arguments and c as the one before rebuilds and uploads none
 * of them; fluid_set_observation_points invalidates them.
 * Refusals, all FLUID_E_INVALID with a message that names the call, found before anything is launched or any state
 * changes, null pointers before the context is looked at: a null `gram`; rhs or dd given with obs null; a null context; a
 * bad field id; no network set; row slabs; M > FLUID_TRANSFORM_MAX_MEMBERS (the message gives both numbers); nodes_row or
 * nodes_col below 1; more than FLUID_LATTICE_MAX_NODES nodes (the message gives both numbers); a step below 8 or not a
 * multiple of 8; a `c` that is not finite or is <= 0; a non-finite inv_sigma[p], named by its index; more than
 * FLUID_LATTICE_GRAM_MAX_ENTRIES (point, node) pairs in total (the message gives both numbers; they are counted before
 * anything is allocated).
 * The launches belong to none of the fluid_timing categories. */
#define FLUID_LATTICE_GRAM_MAX_ENTRIES (1 << 24)
int fluid_observation_gram_lattice(fluid_ctx *ctx, int field, int centre, const float *obs, const float *inv_sigma,
                                   int nodes_row, int nodes_col, int row0, int col0, int step, float c,
                                   double *gram, double *rhs, double *dd, int *counts);

/* ---- one-call analysis: the ETKF solved at every node on the device, and the whole localised update in one call ------------
 * M = fluid_members(ctx), 2 <= M <= FLUID_TRANSFORM_MAX_MEMBERS.  Between the lattice Gram call and the lattice update a
 * localised filter solves one M x M symmetric eigenproblem per node.  fluid_etkf_increments does that for host arrays, every
 * node in ONE kernel launch; fluid_analyse_lattice chains Gram, solve and update on the device without a copy or a wait.
 *
 * The solve, per node, in IEEE double, one definition for both calls:
 *  1. Only gram[k][m] with k <= m is read; the rest is its mirror.  S = mirror(gram) with S_kk = (double)(M-1) / (double)rho
 *     + gram_kk.  `rho` is the multiplicative inflation of Hunt et al. (2007), finite and > 0; 1 means none.
 *  2. S = V L V^T by cyclic Jacobi rotations in the round-robin ordering: with n = M rounded up to even, a sweep is n - 1
 *     steps, step s rotating the disjoint pairs {n-1, s} and {(s+i) mod (n-1), (s-i) mod (n-1)}, i = 1 .. n/2 - 1, together
 *     (a pair with index M, the bye of an odd M, does nothing).  A pair p < q is skipped when |S_pq| <= 2^-53 *
 *     sqrt(S_pp) * sqrt(S_qq); otherwise theta = (S_qq - S_pp) / (2 S_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1))
 *     (1 / (2 theta) once theta^2 would overflow), c = 1 / sqrt(t^2 + 1), s = t c.  A sweep in which every pair was skipped
 *     ends the solve; FLUID_ETKF_MAX_SWEEPS sweeps without one fail the node.
 *  3. l_i = S_ii.  W = V diag(sqrt((M-1) / l_i)) V^T, entry [k][m] the sum over i, in index order, of (V_ki * V_mi) *
 *     sqrt((M-1) / l_i);  w = V diag(1 / l_i) V^T rhs: u_i = (sum over k of V_ki * rhs_k) / l_i, w_k = sum over i of V_ki * u_i.
 *  4. D[k][m] = (W[k][m] - delta_km) + w[k], and the increment is (float)D[k][m]: the weight of OLD member k in the INCREMENT
 *     of new member m, what fluid_transform_members_lattice takes.  For a centred C (C 1 = 0 and rhs . 1 = 0, what centre != 0
 *     produces) and rho = 1 this equals the ETKF increment 1 1^T / M + A (W + w 1^T) - I with A = I - 1 1^T / M: 1 is then
 *     an eigenvector of S with eigenvalue M-1, so W 1 = 1 and w . 1 = 0, and A drops out.  With rho != 1 that eigenvalue is
 *     (M-1) / rho and W 1 = sqrt(rho) 1: D exceeds the centred form by (sqrt(rho) - 1) / M in every entry, that is, the
 *     inflation acts on the ensemble mean as well as on the anomalies.  A caller who wants the anomalies alone inflated
 *     subtracts that constant from the increments of fluid_etkf_increments; fluid_analyse_lattice applies D as defined.
 *  5. Status per node: 0 solved.  1 empty: `counts` is given and counts[node] == 0; the node is neither read nor solved and
 *     D = +0 everywhere -- the background is kept.  2 failed: a non-finite operand, an l_i that is not finite and > 0, the
 *     sweep cap reached, or a D entry that is not finite as a float; D = +0 everywhere.  A failed node changes nothing of
 *     any other node.
 *  6. No eigenvector order or sign is specified; W depends on neither.  A node's M*M floats depend on (M, rho, its upper
 *     triangle, its rhs) alone: the same bits for any node count and node index, call after call and context after
 *     context.  No atomics, no matrix instructions; every rotation order and every order of summation is fixed by M.
 *  7. gram = 0, rhs = 0 and rho = 1 give D == 0 in every entry.
 *
 * - fluid_etkf_increments: all arrays are host memory -- `gram` nodes*M*M doubles, `rhs` nodes*M doubles, `counts` nodes ints
 *   or null (no node is empty), `increments` nodes*M*M floats, increments[(node*M + k)*M + m], `status` nodes ints or null.
 *   Synchronous: one upload, one kernel launch whatever `nodes` is, one download, one wait.  It touches no field.  The
 *   buffers are library-owned device memory outside the arena with pinned twins (fluid_arena_bytes_ensemble is unchanged),
 *   grown on demand and freed by fluid_destroy; a failed allocation is FLUID_E_NOMEM and leaves the context usable.
 *   Refusals, all FLUID_E_INVALID with a message that names the call, found before anything is launched, null pointers
 *   before the context is looked at: a null `gram`, `rhs` or `increments`; a null context; nodes outside [1,
 *   FLUID_LATTICE_MAX_NODES]; M < 2 or M > FLUID_TRANSFORM_MAX_MEMBERS (the message gives both numbers); a rho that is not
 *   finite or is <= 0; a non-finite gram[k <= m] or rhs entry of a node that is not empty (the message names node, k and
 *   m); row slabs.
 * - fluid_analyse_lattice is, bit for bit in every listed field of every member, the sequence
 *       fluid_observation_gram_lattice(ctx, field, 1, obs, inv_sigma, nodes_row .. step, c, gram, rhs, dd, counts);
 *       fluid_etkf_increments(ctx, nodes_row * nodes_col, gram, rhs, counts, rho, increments, status);
 *       fluid_transform_members_lattice(ctx, fields, nfields, increments, nodes_row .. step);
 *   but nothing crosses to the host and nothing waits: the call enqueues the two Gram launches, the solve -- reading their
 *   results and the lists' point counts where they lie, writing the node tables of the lattice update in place -- and one
 *   lattice launch per listed field, and returns.  The lattice launch is always the general one (whether every increment
 *   is non-zero is not known on the host; the bits do not depend on it).  A node without points and a failed node have no
 *   term and store nothing; if every node is like that the launches store nothing and every bit is kept.  The point
 *   lists are built, cached and invalidated exactly as fluid_observation_gram_lattice's -- they are the same lists.
 *   `obs` is required; `field` may or may not be among `fields`.  Refusals: the union of the three calls', under this
 *   call's name.
 * - fluid_analyse_lattice_status waits for the stream and returns how many nodes of the last fluid_analyse_lattice ended
 *   in each status (any of the three pointers may be null): the solve leaves one word per node, folded on the host.
 *   FLUID_E_INVALID before the first analysis of the context.
 * FLUID_ETKF_MAX_SWEEPS: a model of the kernel's ordering and threshold (tests/test_gpu_etkf.py: jacobi_model) needed at
 * most 14 sweeps, the last one without a rotation, over that file's inputs at M = 2 .. 64 (14 at M = 64 on a rank-39 matrix,
 * whose 25 equal eigenvalues keep rotating among themselves at rounding level; 9 to 11 on the others; 9 at M = 33, 7 at
 * M = 9); the cap is twice that and not below 16.
 * The launches belong to none of the fluid_timing categories. */
#define FLUID_ETKF_MAX_SWEEPS 28
int fluid_etkf_increments(fluid_ctx *ctx, int nodes, const double *gram, const double *rhs, const int *counts, float rho,
                          float *increments, int *status);
int fluid_analyse_lattice(fluid_ctx *ctx, int field, const float *obs, const float *inv_sigma, int nodes_row, int nodes_col,
                          int row0, int col0, int step, float c, float rho, const int *fields, int nfields);
int fluid_analyse_lattice_status(fluid_ctx *ctx, int *solved, int *empty, int *failed);

/* ---- relaxation to prior spread: keeping a cycled ensemble from collapsing, per cell --------------------------------------
 * M = fluid_members(ctx), M >= 2, W = N + 2.  The `rho` of the solve is one number for the whole grid and acts only where a
 * node saw observations (and on the mean: one-call analysis, rule 4).  Relaxation to prior spread (RTPS, Whitaker & Hamill
 * 2012) rescales each cell's anomalies after the analysis so that the ensemble standard deviation moves a fraction alpha of
 * the way back to what it was before:
 *     x'_m = mean + (1 + alpha * (sd_b - sd_a) / sd_a) * (x_m - mean)
 * per cell, per field, over all M members.  A cycle is fluid_member_spread -> fluid_analyse_lattice -> fluid_relax_spread,
 * nothing crossing to the host.  Both calls take ANY M >= 2 the context has: they are NOT capped at
 * FLUID_TRANSFORM_MAX_MEMBERS, the kernels walk the members in a loop as the statistics do.
 *
 * `fields`: nfields distinct field ids, host memory, nfields in [1, FLUID_NFIELDS].  `out_dev` / `prior_dev`: nfields dense
 * DEVICE arrays of W*W floats each, row-major with the ghost ring -- the layout `taper_dev` has --, the array of fields[i]
 * starting i * field_stride floats behind the pointer; field_stride = 0: W*W; any other value must be at least W*W (the
 * floats in between are not touched).  Alignment: 4 bytes.  One kernel launch per listed field whatever M is, enqueued on the
 * context's stream, no wait; `fields` belongs to the caller again when the call returns, the device arrays when the stream
 * has passed the launches.  All arithmetic below is IEEE double, every operation rounded once, none contracted.
 *
 * - fluid_member_spread, per listed field, per cell of the W x W array (ghost ring included; pad columns are neither read
 *   nor written):
 *    1. The field's lazy state is settled for all members first, as fluid_pack_members settles it: x_k is the float the
 *       pack would show for member k right before the call -- with fp16 storage the stored value widened exactly, a
 *       pressure scale divided back in float.  Nothing a later step or download sees is altered.
 *    2. mean_d, d_m and q are exactly those of fluid_ensemble_stats: s = (double)x_0; s += (double)x_m in member order;
 *       mean_d = s / (double)M; d_m = (double)x_m - mean_d; q = d_0*d_0; q += d_m*d_m in member order.
 *    3. sd = sqrt(q / (double)(M - 1)): one division, one correctly rounded square root -- the SAMPLE standard deviation,
 *       the normalisation of the ETKF (fluid_ensemble_stats gives the population variance, q / M).
 *    4. out[i][j] = (float)sd.
 *    5. A non-finite x_k makes that cell NaN and affects no other cell.
 * - fluid_relax_spread, per listed field, per cell, in place:
 *    1. x_k is read as rule 1 of fluid_transform_members_lattice reads it and stored by its rule 6 (rule 6 of
 *       fluid_transform_members_local): an fp16 field held at a pressure scale KEEPS the scale, values are read divided
 *       back and stored as narrow(y) times the scale, with the same +-inf beyond 65504 / scale.
 *    2. mean_d, d_m and q as above.
 *    3. q == 0: the cell keeps every bit in every member -- there is no spread to scale; a cell that is -0 everywhere stays
 *       -0.
 *    4. Otherwise sa = sqrt(q / (double)(M - 1)); sb = (double)prior[i][j]; t = sb - sa; t = (double)alpha * t; t = t / sa;
 *       f = 1.0 + t.
 *    5. f == 1.0: the cell keeps every bit in every member.  So alpha = 0 with finite priors is the identity, bit for bit.
 *    6. Otherwise, per member m: p = f * d_m; y_d = mean_d + p -- product and sum each rounded once and NOT contracted into
 *       one fused operation --; y = (float)y_d; the store is narrow(y).
 *    7. A member's new value depends on mean_d, f and its own old value only; all M old values of a cell are read for
 *       mean_d and q before any is stored.
 *    8. A NaN result is a NaN of unspecified sign and payload.  A non-finite x_k makes that cell non-finite in every member
 *       and touches no other cell.  A non-finite or negative prior value gives what rules 4-6 give, in that cell only.
 *   `alpha` is finite and >= 0; values above 1 are legal.
 * The order of operations is part of the contract: the same bits for every launch shape; no atomics, no matrix
 * instructions, no LDS.
 * Refusals, all FLUID_E_INVALID with a message that names the call and, where it applies, the list position, found before
 * anything is launched or any state changes, null pointers before the context is looked at: a null `fields`, `out_dev` or
 * `prior_dev`, a null context; nfields outside [1, FLUID_NFIELDS]; a bad field id; a field listed twice; M < 2 (the message
 * gives M); a field_stride that is neither 0 nor at least W*W; an alpha that is not finite or is negative; a device pointer
 * that is not device memory of the context's device, or whose whole extent, (nfields - 1) * field_stride + W*W floats, does
 * not lie inside one allocation (asked of the runtime on the host, as for a pack); row slabs.
 * The launches belong to none of the fluid_timing categories. */
int fluid_member_spread(fluid_ctx *ctx, const int *fields, int nfields, void *out_dev, size_t field_stride);
int fluid_relax_spread(fluid_ctx *ctx, const int *fields, int nfields, const void *prior_dev, size_t field_stride, float alpha);

/* ---- ensemble noise: reproducible randomness on the device, set or added in place -----------------------------------------
 * M = fluid_members(ctx), M >= 1, W = N + 2.  What makes one member differ from the next -- initial perturbations, additive
 * inflation or model error between cycles (`rho` and RTPS only rescale the spread that is left), the stochastic forcing the
 * *_PREV sources carry, the observation noise of a twin experiment or of a perturbed-observation filter -- is drawn here,
 * on the device, by a counter-based generator with a contract exact to the bit: the noise of (seed, sequence, field,
 * member, cell) is the same bits for every M, every launch shape and every process.  A cycle is fluid_noise_members ->
 * fluid_member_spread -> fluid_analyse_lattice -> fluid_relax_spread -> fluid_run_members, nothing crossing to the host.
 *
 * Random word.  Philox4x32-10 (Salmon, Moraes, Dror & Shaw 2011): multipliers 0xD2511F53 and 0xCD9E8D57, key increments
 * 0x9E3779B9 and 0xBB67AE85, ten rounds.  Known answers (counter; key -> output, hexadecimal words):
 *     0 0 0 0; 0 0                                                  -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *     ffffffff ffffffff ffffffff ffffffff; ffffffff ffffffff        -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *     243f6a88 85a308d3 13198a2e 03707344; a4093822 299f31d0        -> d16cfe09 94fdcceb 5001e420 24126ea1
 * Addressing.  key = (low, high 32 bits of the 64-bit `seed`).  For the cell in row i, column j of a member of a field,
 * counter = (j, i, (field id << 16) | member id, `sequence`), member id = member_offset + m for member m of the context:
 * `member_offset` lets an ensemble split over several contexts draw the noise of one big ensemble.  The ghost ring is a
 * cell like any other; the pitch and the pad columns take no part.
 * Value.  From the four output words: S = the sum of their eight 16-bit halves, an integer in [0, 524280]; z = (double)(S -
 * 262140) * C, C = 0x1.3988e1412ed76p-16 = 1 / sqrt(8 * (2^32 - 1) / 12), one rounding.  z is Irwin-Hall with n = 8: mean 0,
 * variance 1, excess kurtosis -0.15, |z| <= 4.899 -- APPROXIMATELY normal, not normal: the tails end.  No transcendental
 * function appears, on purpose: the device and a numpy model agree to the bit.
 *
 * - fluid_noise_members: `fields`: nfields distinct field ids, host memory, nfields in [1, FLUID_NFIELDS]; `amplitude`: M
 *   finite host floats, a_m for member m.  One kernel launch per listed field whatever M is, enqueued on the context's
 *   stream, no wait; the host arrays belong to the caller again when the call returns.  All arithmetic is IEEE double, every
 *   operation rounded once, none contracted.  Per listed field, per cell of the W x W array (pad columns are neither read
 *   nor written), per member m:
 *    FLUID_NOISE_SET: y = (float)((double)a_m * z); the store is narrow(y).  The field is REPLACED in all members: nothing is
 *       settled first, what the field owed itself is dropped, and afterwards it holds plain values (scale 1), as after a
 *       fluid_unpack_members of all members.
 *    FLUID_NOISE_ADD: x is read as rule 1 of fluid_transform_members_local reads it -- the field is settled first, and an
 *       fp16 field held at a pressure scale KEEPS the scale --; p = (double)a_m * z; y = (float)((double)x + p), product and
 *       sum each rounded once and NOT contracted into one fused operation; the store follows that call's rule 6: narrow(y)
 *       times the scale, +-inf beyond 65504 / scale.  A member with a_m == 0, of either sign, is not stored and keeps every
 *       bit.  A non-finite x stays non-finite in that cell only.
 *   Any M >= 1 works, one-member contexts included: there is NO cap at FLUID_TRANSFORM_MAX_MEMBERS.
 * - fluid_noise_dense writes `count` floats to a dense DEVICE array, aligned to 4 bytes: out[q] = (float)((double)amplitude *
 *   z), z of the counter (low 32 bits of q, high 32 bits of q, (15 << 16) | stream_id, sequence) -- tag 15 is no field id,
 *   so no field cell shares a counter with it.  stream_id in [0, 65535].  One launch, no wait; count = 0 launches nothing.
 *   This is the observation noise for `obs`, or the perturbed observations of a stochastic EnKF.
 * - fluid_noise_value: host logic only, no context and no device, like fluid_coefficients: *z = the z of the counter (c0, c1,
 *   (tag << 16) | member_id, sequence) under `seed`; tag in [0, 15], member_id in [0, 65535].  The kernels and this function
 *   share one body.
 * Correlated noise needs nothing new: an implicit diffusion solve applied to white noise is the standard correlation model
 * (Weaver & Courtier 2001), and fluid_op_diffuse_members is that solve.  The recipe: FLUID_NOISE_SET into a scratch field,
 * fluid_op_diffuse_members from it into a second one, fluid_op_add_source_members with the amplitudes as `dt`.  Smoothing
 * shrinks the variance: measure it once with fluid_member_moments and rescale the amplitudes.
 * Refusals, all FLUID_E_INVALID with a message that names the call and, where it applies, the list position or the member,
 * found before anything is launched or any state changes, null pointers before the context is looked at: a null `fields`,
 * `amplitude`, `out_dev` or `z`, a null context; nfields outside [1, FLUID_NFIELDS]; a bad field id; a field listed twice; a
 * mode that is neither of the two; a non-finite amplitude; member_offset < 0 or member_offset + M > 65536; a stream_id,
 * member_id or tag out of range; an `out_dev` that is not device memory of the context's device, or whose `count` floats
 * do not lie inside one allocation (asked of the runtime on the host, as for a pack); row slabs.
 * The launches belong to none of the fluid_timing categories. */
enum { FLUID_NOISE_SET = 0, FLUID_NOISE_ADD = 1 };
int fluid_noise_members(fluid_ctx *ctx, const int *fields, int nfields, int mode, const float *amplitude, unsigned long long seed,
                        unsigned int sequence, int member_offset);
int fluid_noise_dense(fluid_ctx *ctx, void *out_dev, size_t count, float amplitude, unsigned long long seed, unsigned int sequence,
                      int stream_id);
int fluid_noise_value(unsigned long long seed, unsigned int sequence, int tag, int member_id, unsigned int c0, unsigned int c1, double *z);

/* ---- asynchronous observations: record H x during a run, analyse from the record -------------------------------------------
 * M = fluid_members(ctx), P = the points of the resident network.  Everything above takes every observation at the analysis
 * time: the observing calls sample the fields as they are now.  Real networks report all through the forecast window; the
 * standard answer is 4D-LETKF (Hunt et al. 2004, 2007): apply the observation operator to every member at the time each
 * observation was taken, during the forecast, keep those values H x, and at the end of the window form the same M x M
 * problem from the kept values and apply its weights to the state at the end of the window.  Nothing in the algebra
 * changes, only where h_k[p] comes from.  A 4D cycle is fluid_noise_members -> fluid_member_spread -> fluid_run_window ->
 * fluid_analyse_lattice_recorded -> fluid_relax_spread, nothing crossing to the host.
 *
 * A RECORD is a dense DEVICE float array: record[m * member_stride + p] = h_m[p].  member_stride = 0: P; any other value
 * must be at least P (the floats in between are not touched).  Alignment: 4 bytes.  Its extent is (M - 1) * member_stride +
 * P floats inside one allocation.  This is exactly the out_dev of fluid_observe_members.
 *
 * - fluid_observe_members_range is fluid_observe_members for the points [first, first + count) only: for those p and every
 *   member, record[m * member_stride + p] gets the bits fluid_observe_members would write there -- the same definition of h,
 *   the same settling, the same fp16 scale; FLUID_FIELD_OF_POINT on a typed network is allowed.  Every other float of the
 *   record keeps its bits.  One kernel launch whatever M and count are, on the context's stream, no wait; count = 0
 *   launches nothing.
 * - fluid_run_window: the caller orders the network by report time; a SLOT is a contiguous range of points, slot s the points
 *   [slot_first[s], slot_first[s + 1]), observed after slot_step[s] steps of the run.  The call is defined as a sequence of
 *   existing calls, bit for bit in every field of every member, every snapshot and the record: it is fluid_run_members when
 *   factor == 0 and fluid_run_members_coarse with that factor otherwise; before the first step it observes the slots with
 *   slot_step[s] == 0, in slot order; after step t, behind that step's snapshot packs if any, the slots with slot_step[s] ==
 *   t, in slot order.  Each observation is fluid_observe_members_range(ctx, window->field, slot_first[s], slot_first[s + 1] -
 *   slot_first[s], record_dev, member_stride).  Empty slots launch nothing; points in no slot are never written; several
 *   slots may share a step; slots need not be in time order.  No wait anywhere.  nslots == 0 is the plain run, bit for bit, but not
 *   the plain call: the window is checked whatever nslots is, so a network must be set and record_dev must be a record of
 *   full extent even when nothing will be written to it.  The host
 *   arrays and the struct belong to the caller again when the call returns.
 * - fluid_observation_gram_recorded, fluid_observation_gram_lattice_recorded and fluid_analyse_lattice_recorded are their
 *   namesakes with rule 1 replaced by h_k[p] = record[k * member_stride + p].  The float is read in stream order: a record
 *   written earlier on the context's stream needs no wait.  Everything after rule 1 is untouched, operation for operation:
 *   the mean chain, 1 / sigma and the innovation, the chunks of 64 points and the wave order, the folds, the point lists and
 *   their cache (the same cache, shared with the direct calls), the weights, the solve, the lattice update and the status
 *   words (fluid_analyse_lattice_status serves both).  So:
 *    1. A record that fluid_observe_members just wrote gives the direct call's bits.
 *    2. No field is settled or read by the two Gram calls; fluid_analyse_lattice_recorded settles and updates only the listed
 *       `fields` -- the state at the END of the window, which is the point of the method.
 *    3. The network must be set: it supplies the positions and P.  Whether it is typed does not matter.
 *    4. Poisoning follows the namesakes, "a non-finite h_k" meaning a non-finite float in the record.
 *   The library does not know which points were recorded.  For points that were left out: zero-fill the record first and
 *   give such points inv_sigma 0.
 * Refusals, all FLUID_E_INVALID with a message that names the call and, where it applies, the slot or the point, found
 * before anything is launched or any state changes, null pointers before the context is looked at: whatever the namesake
 * refuses, under the new name; a null record_dev, window, plan, dt, diff or visc; a null slot_first or slot_step with
 * nslots > 0; nslots outside [0, FLUID_WINDOW_MAX_SLOTS] (the message gives both numbers); first, count or first + count
 * outside [0, P]; a slot_first that decreases, starts below 0 or ends above P (the slot is named); a slot_step[s] outside
 * [0, nsteps] (the slot is named); a stride below P; a record that is not device memory of the context's device or whose
 * extent does not lie inside one allocation (asked of the runtime on the host, as for a pack); no network set;
 * FLUID_FIELD_OF_POINT on an untyped network; M > FLUID_TRANSFORM_MAX_MEMBERS for the three recorded calls; row slabs.
 * The launches belong to none of the fluid_timing categories. */
#define FLUID_WINDOW_MAX_SLOTS 65536
typedef struct fluid_obs_window {
    int field;              /* field id or FLUID_FIELD_OF_POINT */
    int nslots;             /* 0 .. FLUID_WINDOW_MAX_SLOTS */
    const int *slot_first;  /* host, nslots + 1 ints: slot s holds points [slot_first[s], slot_first[s+1]) */
    const int *slot_step;   /* host, nslots ints in [0, plan->nsteps]: slot s is observed after that many steps */
    void *record_dev;
    size_t member_stride;
} fluid_obs_window;
int fluid_observe_members_range(fluid_ctx *ctx, int field, int first, int count, void *record_dev, size_t member_stride);
int fluid_run_window(fluid_ctx *ctx, const float *dt, const float *diff, const float *visc, const fluid_run_plan *plan, int factor,
                     const fluid_obs_window *window, int *snapshots_written);
int fluid_observation_gram_recorded(fluid_ctx *ctx, const void *record_dev, size_t member_stride, int centre, const float *obs,
                                    const float *inv_sigma, double *gram, double *rhs, double *dd);
int fluid_observation_gram_lattice_recorded(fluid_ctx *ctx, const void *record_dev, size_t member_stride, int centre, const float *obs,
                                            const float *inv_sigma, int nodes_row, int nodes_col, int row0, int col0, int step, float c,
                                            double *gram, double *rhs, double *dd, int *counts);
int fluid_analyse_lattice_recorded(fluid_ctx *ctx, const void *record_dev, size_t member_stride, const float *obs, const float *inv_sigma,
                                   int nodes_row, int nodes_col, int row0, int col0, int step, float c, float rho, const int *fields,
                                   int nfields);

/* ---- screening observations: departures, ranks and a background check, on the device ---------------------------------------
 * M = fluid_members(ctx), 2 <= M <= FLUID_TRANSFORM_MAX_MEMBERS; P = the points of the resident network.  Between "H x is
 * known" and "the weights are formed" every operational filter checks its observations against the background: a report
 * whose departure from the ensemble mean is many times what the spread and its own error explain is dropped, or it wrecks
 * every node within 2c of it.  The six Gram and analysis calls read 1 / sigma from a device buffer, and a point with
 * inv_sigma 0 takes no part; a check that runs on the device and writes that buffer needs no host algebra and no wait.
 *
 * Definitions, per point p, shared by everything below.  All arithmetic is IEEE double, every operation rounded once, none
 * contracted.
 *    1. h_k[p]: rule 1 of fluid_observation_gram, or record[k * member_stride + p] for the _recorded calls: the same
 *       observation, the same settling, the same fp16 scale per field, FLUID_FIELD_OF_POINT on a typed network.
 *    2. s = (double)h_0, then s += (double)h_m for m = 1 .. M-1;  mean_d = s / (double)M;  e_m = (double)h_m - mean_d;
 *       q = e_0 * e_0, then q += e_m * e_m in member order, each product rounded and then added;  var = q / (double)(M - 1).
 *       These are the chains of fluid_ensemble_stats and fluid_member_spread.
 *    3. sg = (double)inv_sigma[p], 1.0 for a null inv_sigma;  dep = (double)y_p - mean_d;  d = dep * sg -- bit for bit the
 *       d[p] of fluid_observation_gram with centre != 0.
 *    4. lhs = d * d;  vs = var * sg, then vs = vs * sg;  bound = 1.0 + vs;  t2 = (double)threshold * (double)threshold;
 *       lim = t2 * bound;  the point is REJECTED when threshold != 0 and lhs > lim.  A comparison with a NaN is false: a NaN
 *       h, y or sigma rejects nothing, and the poisoning rules of the Gram calls hold unchanged.  The gate is NO guard
 *       against non-finite values: a rejected y = inf still gives inf * 0 = NaN in the Gram call.  A point that arrives
 *       with inv_sigma 0 has d = 0 and is never rejected.
 *    5. rank[p] = the number of k with h_k[p] < y_p, compared as floats: 0 .. M, the bin of the Talagrand histogram.  A NaN
 *       on either side counts as "not below".
 *
 * - fluid_observation_departures / fluid_observation_departures_recorded: synchronous like fluid_observation_gram.  Host
 *   outputs of P entries each, any of them null: mean[p] = (float)mean_d, spread[p] = (float)sqrt(var), departure[p] =
 *   (float)dep, rank[p], flag[p] (1: rejected).  `obs` may be null: then departure, rank, flag and sums must be null and
 *   threshold 0.  sums[3], over the points that are NOT rejected: their count as a double, the sum of d * d, the sum of vs.
 *   A caller estimates the multiplicative inflation its ensemble lacks from them, E[d * d] = 1 + v: (sums[1] - sums[0]) /
 *   sums[2].  Order of each sum: within a chunk of 64 consecutive points in increasing point index, from the first term
 *   (-0.0 for a chunk without one); lane j of 16 then chains the chunks j, j + 16, .. from -0.0 and the 16 are added in index
 *   order, as fluid_observation_gram folds its partials.  No atomics: the same bits call after call, and the exact sum when
 *   every partial sum is representable.  At most two launches whatever P and M, one copy back, one wait; the results pass
 *   through library-owned scratch outside the arena.  The resident gate below and its last result are not touched.
 * - fluid_set_observation_qc / fluid_observation_qc: the resident gate, a threshold kept in the context; 0, the default, is
 *   off, any finite value >= 0 is accepted, and it survives fluid_set_observation_points / _network.  While it is above 0,
 *   fluid_observation_gram, fluid_observation_gram_lattice, fluid_analyse_lattice and their _recorded namesakes, whenever
 *   their `obs` is non-null, first run rule 4 on the h they are about to use -- with the mean of rule 2 whatever the call's
 *   own `centre` -- and then proceed BIT FOR BIT as the same call with the gate off and inv_sigma[p] replaced by +0.0f at
 *   the rejected points, a null inv_sigma counting as all ones.  One more launch on the context's stream and no wait; the
 *   lists, their cache, the counts, the solve and the status words are as before.  A node whose points are all rejected
 *   has a zero Gram, not an empty list: its status is "solved" and D = 0 at rho = 1.  A call with `obs` null checks
 *   nothing and leaves the last result in place.  With the gate off no call changes its bits or its launches.
 * - fluid_observation_qc_result: waits for the stream; flags[p] of the last gated call (P bytes), *checked = P, *rejected =
 *   the number of flags set; any pointer may be null.
 * Refusals, all FLUID_E_INVALID with a message that names the call, found before anything is launched or any state changes,
 * null pointers before the context is looked at: whatever fluid_observation_gram[_recorded] refuses, under the new names;
 * M < 2 or M > FLUID_TRANSFORM_MAX_MEMBERS (the message gives both numbers); a threshold that is not finite or is
 * negative; departure, rank, flag or sums given with obs null; a non-zero threshold with obs null; a null `threshold`
 * pointer; fluid_set_observation_qc on a one-member context or on row slabs; fluid_observation_qc_result before the first
 * gated call, and again after the network is replaced.
 * The launches belong to none of the fluid_timing categories. */
int fluid_observation_departures(fluid_ctx *ctx, int field, const float *obs, const float *inv_sigma, float threshold, float *mean,
                                 float *spread, float *departure, unsigned char *rank, unsigned char *flag, double *sums);
int fluid_observation_departures_recorded(fluid_ctx *ctx, const void *record_dev, size_t member_stride, const float *obs,
                                          const float *inv_sigma, float threshold, float *mean, float *spread, float *departure,
                                          unsigned char *rank, unsigned char *flag, double *sums);
int fluid_set_observation_qc(fluid_ctx *ctx, float threshold);
int fluid_observation_qc(fluid_ctx *ctx, float *threshold);
int fluid_observation_qc_result(fluid_ctx *ctx, unsigned char *flags, int *checked, int *rejected);

/* ---- verifying ensembles: CRPS, RMSE against spread and the rank histogram against a truth field, on the device -------------
 * M = fluid_members(ctx), 2 <= M <= FLUID_TRANSFORM_MAX_MEMBERS, W = N + 2.  The cycle perturbs, forecasts, observes, screens,
 * analyses and re-inflates in stream order; whether it WORKS is judged in field space, against a truth a twin experiment has
 * as one more context's pack: the error of the ensemble mean beside the ensemble variance, the continuous ranked probability
 * score, the rank histogram over the cells.  fluid_verify_members reads the members once, enqueues on the context's stream
 * and does not wait; nothing crosses to the host.
 *
 * `fields`: nfields distinct field ids, host memory, nfields in [1, FLUID_NFIELDS].  `truth_dev`: nfields dense DEVICE arrays of
 * W*W floats each, the layout and the field_stride rules of the `prior_dev` of fluid_relax_spread (0: W*W; the floats in
 * between are not read).  `crps_dev`: null, or nfields such arrays at the same stride: the per-cell CRPS as a float, written
 * inside the box only -- cells outside it and the floats between fields are not touched.  `scores_dev`: device memory,
 * 8-byte aligned, nfields rows of FLUID_VERIFY_ROW doubles.  `box`: host memory, {row_lo, row_hi, col_lo, col_hi}, half-open
 * ranges inside [0, W] as fluid_transform_members_local takes them; null: the interior, [1, N+1) x [1, N+1); an empty box is
 * legal.  `flags`: 0 or FLUID_VERIFY_FAIR.  At most two kernel launches per listed field whatever M and the box are; the
 * per-block partial results pass through library-owned scratch outside the arena, which grows with the box (a growth the
 * device refuses is FLUID_E_NOMEM and leaves the context usable).  `fields` and `box` belong to the caller again when the call
 * returns, the device arrays when the stream has passed the launches.
 *
 * Per listed field, per cell of the box.  All arithmetic is IEEE double, every operation rounded once, none contracted.
 *    1. x_k is what rule 1 of fluid_member_spread reads: the field is settled as a pack settles it, an fp16 value widened
 *       exactly, a pressure scale divided back in float.  Nothing a later step or download sees is altered.  y is the float
 *       of `truth_dev`.
 *    2. mean_d, d_m and q are exactly the chains of fluid_ensemble_stats, in member order (rule 2 of fluid_member_spread).
 *       var = q / (double)(M - 1);  e = mean_d - (double)y;  se = e * e.
 *    3. For the CRPS only, every x_k and y is first replaced by v + 0.0f: -0 counts as +0.  s_1 <= .. <= s_M are the x_k
 *       sorted ascending as floats -- after the replacement equal values are identical bits, so the sequence is unique.
 *       a = |(double)s_1 - (double)y|, then a += |(double)s_i - (double)y| in increasing i;
 *       g = (double)(1 - M) * (double)s_1, then g += (double)(2i - M - 1) * (double)s_i in increasing i (every product exact);
 *       t1 = a / (double)M;  t2 = g / (double)(M*M), or g / (double)(M*(M-1)) with FLUID_VERIFY_FAIR (Ferro 2014);
 *       crps = t1 - t2.  This is the energy form (1/M) sum |x_m - y| - (1/2M^2) sum sum |x_m - x_k|, the pair sum written over
 *       the order statistics.
 *    4. rank = the number of k with x_k < y, compared as floats, as rule 5 of "screening observations": 0 .. M.  A NaN on
 *       either side counts as "not below".
 *    5. If any x_k or y of the cell is not finite, crps is a NaN of unspecified sign and payload; e, se and var are what
 *       their chains give.  The cell poisons the sums it enters and no other cell's map value.
 *    6. crps_dev[i][j] = (float)crps.
 * The score row of a field: [0] the number of cells in the box, as a double; [1] sum e; [2] sum se; [3] sum var; [4] sum
 * crps; [5 + r], r = 0 .. M: the number of cells with rank r, as a double; beyond [5 + M]: +0.0.  The caller derives
 * bias = [1] / [0], rmse = sqrt([2] / [0]), spread = sqrt([3] / [0]) and the mean CRPS = [4] / [0]; a calibrated ensemble has
 * rmse^2 ~ (M + 1) / M * [3] / [0] and a flat histogram.
 * Counts are integers until the end and exact.  Order of each of the four sums: the cells of the box are numbered row by
 * row, t = (row - row_lo) * (col_hi - col_lo) + (col - col_lo); B = min(ceil(cells / 256), 2048) blocks of 256 lanes; lane L
 * of the 256 * B chains the terms of the cells L, L + 256 * B, .. in increasing t, from -0.0 (a sum starts from its first
 * term); the 64 lanes of a wave are added by a butterfly, lane j taking lane j ^ 32's, then ^ 16, 8, 4, 2, 1; a block's four
 * waves in wave order; then lane j of 64 chains the blocks j, j + 64, .. from -0.0 and the same butterfly adds the 64.  So the
 * order depends on (N, box, M, storage type, flags) and on nothing else -- not on the device, not on the call before: no
 * floating-point atomics, the same bits call after call and process after process, and the exact sum whenever every
 * partial sum is representable.  An empty box gives count 0, zero sums (of either sign) and zero bins.  No matrix instructions.
 * Refusals, all FLUID_E_INVALID with a message that names the call, found before anything is launched or any state changes,
 * null pointers before the context is looked at: a null `fields`, `truth_dev` or `scores_dev`, a null context; whatever
 * fluid_member_spread refuses of its list, its stride and its device array, under this call's name (M < 2 among it);
 * M > FLUID_TRANSFORM_MAX_MEMBERS (the message gives both numbers); a box entry outside [0, W] or a lo above its hi; unknown
 * flag bits; a `scores_dev` that is not 8-byte aligned, or whose nfields * FLUID_VERIFY_ROW doubles do not lie inside one
 * allocation of the context's device; a `crps_dev` whose extent, that of `truth_dev`, does not; row slabs.
 * The launches belong to none of the fluid_timing categories. */
#define FLUID_VERIFY_SUMS 5
#define FLUID_VERIFY_ROW  (FLUID_VERIFY_SUMS + FLUID_TRANSFORM_MAX_MEMBERS + 1)   /* 70 doubles */
#define FLUID_VERIFY_FAIR 1   /* flags: the CRPS's pair term over M(M-1) in place of M*M (Ferro 2014) */
int fluid_verify_members(fluid_ctx *ctx, const int *fields, int nfields, const void *truth_dev, size_t field_stride, const int *box,
                         int flags, void *crps_dev, void *scores_dev);

/* ---- ensemble products: quantile fields and exceedance probabilities, per cell across the members, on the device -------------
 * M = fluid_members(ctx), W = N + 2.  What an ensemble FORECAST hands to its user beside the mean and the variance
 * (fluid_ensemble_stats, fluid_member_spread): order statistics per cell -- the median, the quartiles, the 5 % / 95 % envelope,
 * minimum and maximum -- and exceedance probabilities, the fraction of members above or below a threshold per cell.  Both
 * calls read the members once, in place: no M*W*W dense copy, no second pass.
 *
 * Common to both device calls.  Each call handles ONE field.  `out_dev`: nlevels (nthresholds) dense DEVICE arrays of W*W
 * floats each, row-major with the ghost ring -- the layout of the `out_dev` of fluid_member_spread --, array l starting
 * l * level_stride floats behind the pointer; level_stride = 0: W*W; any other value must be at least W*W (the floats in
 * between are not touched).  Alignment: 4 bytes.  Every cell of the W x W array is computed; pad columns are neither read nor
 * written.  ONE kernel launch per call whatever M and the level count are, enqueued on the context's stream, no wait; the host
 * arrays belong to the caller again when the call returns, `out_dev` when the stream has passed the launch.  The field's
 * lazy state is settled first, as fluid_member_spread settles it: x_k is the float the pack would show for member k right
 * before the call -- with fp16 storage the stored value widened exactly, a pressure scale divided back in float.  Nothing a
 * later step or download sees is altered.  No atomics, no LDS, no matrix instructions: the same bits for every launch shape.
 *
 * - fluid_quantile_position: host logic only, no context and no device, like fluid_coefficients and fluid_noise_value.
 *   `members` in [1, FLUID_TRANSFORM_MAX_MEMBERS], `level` finite and in [0, 1].  In IEEE double: h = (double)level *
 *   (double)(members - 1) -- the product is exact, 24 + 7 bits --; *lo = floor(h); *frac = h - *lo, also exact.  If *lo >=
 *   members - 1: *lo = members - 1 and *frac = 0.  This is numpy's default ("linear", Hyndman & Fan 1996 type 7) position.
 *   fluid_member_quantiles and this function share one body.
 * - fluid_member_quantiles: 1 <= M <= FLUID_TRANSFORM_MAX_MEMBERS; M = 1 is legal.  `levels`: nlevels host floats, nlevels in
 *   [1, FLUID_QUANTILE_MAX_LEVELS]; they may repeat and need not be ordered.  Per cell:
 *    1. Every x_k is replaced by x_k + 0.0f: -0 counts as +0, as in rule 3 of fluid_verify_members.  s_0 <= .. <= s_{M-1} are
 *       the values sorted ascending as floats -- after the replacement equal values are identical bits, so the sequence is
 *       unique.
 *    2. Per level l: (lo, frac) = fluid_quantile_position(M, levels[l]), computed once on the host.  frac == 0: out = s_lo, a
 *       bit copy.  Otherwise d = (double)s_{lo+1} - (double)s_lo; t = frac * d; q = (double)s_lo + t -- each of the three
 *       rounded once, none contracted --; out = (float)q.
 *    3. If any x_k of the cell is not finite, every level's value in that cell is a NaN of unspecified sign and payload.  No
 *       other cell is affected.
 *    4. So level 0 is the minimum, 1 the maximum, 0.5 the median; with M even the median is the midpoint under rule 2.
 * - fluid_member_exceedance: ANY M >= 1 the context has, NOT capped at FLUID_TRANSFORM_MAX_MEMBERS: the kernel walks the
 *   members in a loop, as the spread does.  `thresholds`: nthresholds finite host floats t_l, nthresholds in [1,
 *   FLUID_QUANTILE_MAX_LEVELS].  Per cell and per threshold l:
 *    1. count = the number of k with x_k > t_l (FLUID_EXCEED_ABOVE) or with x_k < t_l (FLUID_EXCEED_BELOW), compared as
 *       floats: -0 equals +0, a NaN member counts as neither, +-inf compare as they do.
 *    2. out = (float)((double)count / (double)M).
 *    3. The members are read once for all thresholds.
 * Refusals, all FLUID_E_INVALID with a message that names the call and, where it applies, the list index, found before
 * anything is launched or any state changes, null pointers before the context is looked at: a null `levels`, `thresholds`,
 * `out_dev`, `lo` or `frac`, a null context; a count outside [1, FLUID_QUANTILE_MAX_LEVELS]; a bad field id; a level that is not
 * finite or lies outside [0, 1]; a threshold that is not finite; a mode that is neither of the two; `members` outside [1,
 * FLUID_TRANSFORM_MAX_MEMBERS] for the position; M > FLUID_TRANSFORM_MAX_MEMBERS for the quantiles (the message gives both
 * numbers); a level_stride that is neither 0 nor at least W*W; an `out_dev` that is not device memory of the context's device,
 * or whose whole extent, (count - 1) * level_stride + W*W floats, does not lie inside one allocation (asked of the runtime on
 * the host, as for a pack); row slabs.
 * The launches belong to none of the fluid_timing categories. */
#define FLUID_QUANTILE_MAX_LEVELS 16
enum { FLUID_EXCEED_ABOVE = 0, FLUID_EXCEED_BELOW = 1 };
int fluid_quantile_position(int members, float level, int *lo, double *frac);
int fluid_member_quantiles(fluid_ctx *ctx, int field, const float *levels, int nlevels, void *out_dev, size_t level_stride);
int fluid_member_exceedance(fluid_ctx *ctx, int field, const float *thresholds, int nthresholds, int mode, void *out_dev,
                            size_t level_stride);

int fluid_set_jacobi_variant(fluid_ctx *ctx, int variant);
/* How FLUID_JACOBI_TB divides by `beta` in a solve with these coefficients (diagnostic; runs the on-device proof
 * if this beta has not been seen): 0 true division, 2 double-precision reciprocal, 3 two-term float reciprocal
 * where the right-hand side allows it (else as 2), 4 exact float reciprocal (beta a power of two, alpha 1), 5 float
 * reciprocal with scaled residual correction. */
int fluid_division_mode(fluid_ctx *ctx, float alpha, float beta, int *mode);
/* The launch depths FLUID_JACOBI_TB uses for one solve of `iters` sweeps on a grid (or slab) of `rows` x N cells: host
 * logic only (no device needed) -- `pressure_form`: alpha 1 / beta 4; `max_sweeps`, `t16_min_cells` as the parameters of the
 * same names (-1: default rule).  Writes up to `capacity` depths and the number of launches. */
int fluid_plan_sweeps(int N, int rows, int storage, int pressure_form, int iters, int max_sweeps, int t16_min_cells,
                      int *depths, int capacity, int *count);
/* Launch shapes whose strip height is still being measured (FLUID_PARAM_TB_AUTOTUNE), process-wide: a benchmark runs
 * untimed steps until this reaches 0. */
int fluid_autotune_pending(fluid_ctx *ctx, int *shapes_open);
int fluid_set_param(fluid_ctx *ctx, int key, int value);

/* ---- timing: HIP events on the context's stream around every operator -------
 * Categories are the reference's per-kernel timers (timeSource, timeDiffusion,
 * timeDivergence, timeProjection, timeAdvection: FluidSequential.c:16,192-234). */
enum {
    FLUID_TIME_SOURCE = 0, FLUID_TIME_DIFFUSION = 1, FLUID_TIME_DIVERGENCE = 2,
    FLUID_TIME_PROJECTION = 3, FLUID_TIME_ADVECTION = 4, FLUID_TIMING_CATEGORIES = 5
};
typedef struct fluid_timing {
    double jacobi_ms;      /* device time inside Jacobi solves since the last reset (= category DIFFUSION) */
    long long sweeps;      /* Jacobi sweeps executed in those solves                */
    long long solves;
    double category_ms[FLUID_TIMING_CATEGORIES];
    long long category_calls[FLUID_TIMING_CATEGORIES];
    long long jacobi_launches;        /* Jacobi kernel launches in those solves                              */
    long long jacobi_field_launches;  /* the same, counting a launch once per field it sweeps (a batched launch
                                         sweeps up to three, in every member of an ensemble): x12 B x cells = the
                                         launches' compulsory bytes */
    double pressure_ms;               /* the part of jacobi_ms spent in the pressure solves of fluid_step /
                                         fluid_vel_step (alpha 1, beta 4, b 0: FluidSequential.c:222,240)     */
    long long pressure_sweeps;
} fluid_timing;
int fluid_timing_enable(fluid_ctx *ctx, int on);
int fluid_timing_read(fluid_ctx *ctx, fluid_timing *out, int reset);

/* ---- opt-in extension (changes results: NOT the reference's fixed 40 sweeps) -
 * Jacobi in blocks of `check_every` (even) sweeps until the max-norm residual
 * max|beta*x - alpha*(L+R+U+D) - x0| <= tol, or max_iters.  The report proposes
 * a convergence-aware solve as future work (document/main.tex:356). */
int fluid_op_diffuse_tol(fluid_ctx *ctx, int b, int x, int x0, float alpha, float beta,
                         float tol, int max_iters, int check_every,
                         int *iters_done, float *residual);

/* ---- multi-GPU: row slabs, one context (and one process) per GPU ----------
 * The solver calls back whenever rows must move between slabs; the host layer
 * implements it with RCCL (torch.distributed) on the context's stream.
 *   FLUID_XCHG_HALO  : for each listed field, send `depth` owned rows at each
 *                      slab edge to that neighbour and receive its rows into
 *                      the rows just outside the owned range.
 *   FLUID_XCHG_GATHER: all-gather the owned rows (end slabs: plus the ghost
 *                      row) of each listed field, so every rank holds the full field.
 *   FLUID_XCHG_MAX   : *scalar = max over ranks of *scalar (host value, synchronous).
 *   FLUID_XCHG_MAX_BEGIN / _END: the same reduction split so the solver can keep the GPU busy
 *                      while it is in flight.  BEGIN (scalar == NULL): enqueue, on the context's
 *                      stream, an in-place MAX over ranks of the device scalar (fluid_scalar_ptr);
 *                      the solver then copies it to the host asynchronously.  END: *scalar holds
 *                      that host copy; a transport that cannot reduce on the device leaves BEGIN
 *                      empty and replaces *scalar by the max over ranks here.
 * Return 0 on success. */
enum { FLUID_XCHG_HALO = 0, FLUID_XCHG_GATHER = 1, FLUID_XCHG_MAX = 2, FLUID_XCHG_MAX_BEGIN = 3,
       FLUID_XCHG_MAX_END = 4 };
typedef int (*fluid_exchange_fn)(void *user, int kind, const int *fields, int nfields,
                                 int depth, float *scalar);
int fluid_set_exchange(fluid_ctx *ctx, fluid_exchange_fn fn, void *user);
/* The stream (hipStream_t) an exchange callback should enqueue on, asked from INSIDE the callback: with
 * FLUID_PARAM_XCHG_OVERLAP the library runs its exchanges on a stream of their own (already ordered behind the kernels that
 * produced the rows; the library orders the consumers behind it).  A callback that keeps using the stream given to
 * fluid_create_ex stays correct -- it is merely not overlapped with compute. */
int fluid_exchange_stream(fluid_ctx *ctx, void **stream);
/* Jacobi launches so far that ran as interior strips + edge strips around an exchange in flight (diagnostic). */
int fluid_split_launches(fluid_ctx *ctx, long long *count);
/* Runs the installed exchange now for the listed fields (HALO with `depth` rows, or GATHER): how a caller collects a
 * whole field on every rank, and how the transport can be exercised on its own. */
int fluid_exchange_now(fluid_ctx *ctx, int kind, const int *fields, int nfields, int depth);

/* ---- the library's own exchange: RCCL over xGMI, no host in the path ------------------------------------
 * north_star: "one-row ghost cells exchanged via RCCL Sendrecv over xGMI" (the reference is single-device:
 * naivePar/FluidParallelBlockPerElement-Naive.cu:351-355 only ever selects device 0).  Halo rows travel as grouped
 * ncclSend/ncclRecv between neighbouring slabs, the advect fall-back as grouped ncclBroadcast, the velocity bound
 * as an in-place ncclAllReduce(max) on the device scalar; everything is enqueued on the context's stream.
 * librccl is bound at run time ($FLUID_RCCL_LIB if set; else an RCCL the process already holds; else the
 * system's), so single-GPU users need none.
 *   fluid_rccl_available():       FLUID_OK if librccl could be loaded and every entry point bound in THIS process (no
 *                                 communication): all ranks agree on it (e.g. a MIN all-reduce over the transport that
 *                                 carries the id) BEFORE anyone enters the collective attach -- a rank that cannot load
 *                                 the library would otherwise leave its peers waiting inside ncclCommInitRank
 *   fluid_rccl_unique_id():       one rank calls it and hands the FLUID_RCCL_ID_BYTES bytes to all others (any way)
 *   fluid_exchange_rccl_attach(): every rank, with its context (rank / nranks from fluid_create_ex) and that id, on
 *                                 the thread whose current HIP device is the context's: creates the communicator,
 *                                 runs one all-reduce and one send/receive probe, installs the exchange
 *   ..._attach_comm():            the same on a communicator (ncclComm_t) the caller owns
 *   ..._detach():                 removes it (and destroys a communicator the library created)
 *   ..._calls():                  exchanges issued so far: halo, gather, max                                  */
#define FLUID_RCCL_ID_BYTES 128
int fluid_rccl_available(void);
int fluid_rccl_unique_id(void *id, size_t bytes);
int fluid_exchange_rccl_attach(fluid_ctx *ctx, const void *id, size_t bytes);
int fluid_exchange_rccl_attach_comm(fluid_ctx *ctx, void *nccl_comm);
int fluid_exchange_rccl_detach(fluid_ctx *ctx);
int fluid_exchange_rccl_calls(fluid_ctx *ctx, long long *halo, long long *gather, long long *max);

#ifdef __cplusplus
}
#endif
#endif /* FLUID_AMD_H */
