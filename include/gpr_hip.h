/*
 * gpr_hip.h -- C ABI of libgpr_hip.so, the MI355X (gfx950) exact-GP engine.
 *
 * Drop-in boundary for the dense hot path of GaussianProcessRegression.jl
 * (reference snapshot 2025-03-21).  The reference has no FFI of its own: its extension
 * seams are Julia multiple dispatch on the output-array type (kernel!(::AbstractGPUArray)
 * src/covar_gpu.jl:1) and on the cache type (update_cache!/loss/grad!/predict!,
 * src/cost.jl:40-126, src/predict.jl:29-101, src/split_predict.jl:5-53).  Each entry point
 * below names the reference function it replaces; INTEGRATION.md shows the Julia
 * `ccall` methods a maintainer adds on those seams.
 *
 * Conventions (all of them Julia's, so a Julia caller passes its arrays unchanged):
 *   - fp64 everywhere; matrices are COLUMN-MAJOR with an explicit leading dimension.
 *   - x is d x n column-major (each sample's d features contiguous), like md.x.
 *   - A kernel is described by `kinds[nk]` (GPR_SE / GPR_M32 / GPR_M52 / GPR_PER / GPR_WN, in `+` order)
 *     and the flat hyper-parameter vector `hp` (HOST pointer) of length sum(dim_hp) -- SE, M32,
 *     M52: d+1 ([sigma, l_1..l_d]), PER: 2d+1 ([sigma, l_1..l_d, p_1..p_d]), WN: 1 ([sigma_n])
 *     -- exactly split(hp, dims)
 *     (src/compose_covar.jl:21-28).  A GPR_MUL entry between two stationary parts multiplies them
 *     (product terms, below); it counts in nk and owns no hyper-parameters.
 *   - Pointers named d* are DEVICE pointers (from gpr_malloc, hipMalloc, or a torch
 *     tensor); all other pointers are host pointers.  No pointer is retained after a call
 *     returns.
 *   - Every op is enqueued on the context's stream.  Ops that return host scalars/vectors
 *     (info, mll, grad) synchronise the stream before returning; the others are async.
 *   - A context is not thread-safe: one context (one stream) per host thread.
 *
 * Return codes: 0 ok; >0 LAPACK-style info (gpr_potrf_upper: order of the leading minor
 * that is not positive definite, like dpotrf / Julia's PosDefException(info));
 * <0 errors (GPR_E_*), with a message from gpr_last_error(ctx).
 */
#ifndef GPR_HIP_H
#define GPR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPR_SE 1 /* SquaredExp  src/covariance.jl:15 */
#define GPR_WN 2 /* WhiteNoise  src/covariance.jl:17 */
#define GPR_M32 3 /* Matern-3/2 (no counterpart in the reference: defined below) */
#define GPR_M52 4 /* Matern-5/2 */
#define GPR_PER 5 /* Periodic (no counterpart in the reference: defined below) */
#define GPR_MUL 6 /* product marker between two stationary factors (defined below) */

#define GPR_OK 0
#define GPR_E_ARG (-1)      /* bad argument (message names it)                      */
#define GPR_E_HIP (-2)      /* HIP runtime error                                    */
#define GPR_E_NOMEM (-3)    /* device allocation failed                             */
#define GPR_E_UNSUP (-4)    /* unsupported configuration (e.g. an eigen-reduction size) */

/* Kernel descriptions (kinds, nk, hp, d): any input dimension d >= 1 and any number of parts,
 * in any order, with at least one stationary part (GPR_SE, GPR_M32, GPR_M52, GPR_PER).  For SquaredExp /
 * WhiteNoise parts this is the reference's envelope (src/covariance.jl:85-95,
 * src/compose_covar.jl:9-28,47-61).
 *
 * The stationary parts share one hp layout, [sigma, l_1..l_d], and one distance: with
 *   D = sum_k (l_k (x_k - x'_k))^2,   r = sqrt(max(D, 0)),
 *   GPR_SE   k = sigma^2 exp(-D)                                          (the reference's)
 *   GPR_M32  k = sigma^2 (1 + sqrt(3) r) exp(-sqrt(3) r)
 *   GPR_M52  k = sigma^2 (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r)
 * The l_k are MULTIPLIERS (inverse length-scales), as in the reference's SquaredExp (exp(-D),
 * no 1/2): the textbook Matern length-scale is 1 / l_k.  Derivatives follow the shape of
 * src/deriv_covar.jl:20-29 with W = -dk/dD (finite at r = 0):
 *   dK/dsigma = (2 / |sigma|) K_p   (K_p with eps on a same-object diagonal, as for SE)
 *   dK/dl_k   = -2 l_k W (x_k - x'_k)^2 on raw x,
 *   W_SE = k,  W_M32 = sigma^2 (3/2) exp(-sqrt(3) r),
 *   W_M52 = sigma^2 (5/6) (1 + sqrt(5) r) exp(-sqrt(5) r).
 * Every rule the reference states per SquaredExp part holds per stationary part: eps once per
 * stationary part on a same-object diagonal, the noise of the first WhiteNoise, the diagonal-
 * variance prior sum over ALL parts of hp_part[1]^2, LogScale when a stationary part is present.
 *
 * GPR_PER, hp of the part [sigma, l_1..l_d, p_1..p_d] (2d + 1 values):
 *   D = sum_k (2 l_k sin(pi (x_k - x'_k) / p_k))^2,   k = sigma^2 exp(-D)
 * MacKay's periodic kernel as a product over dimensions, textbook length-scale 1 / (sqrt(2) l_k);
 * the l_k are multipliers as for SquaredExp, k is even in every p_k.  A period that is zero, NaN
 * or infinite returns GPR_E_ARG (the message names the part and the dimension; nothing is
 * computed or written).  It is evaluated as SquaredExp on the 2d embedded features
 * [l_k cos(2 pi x_k / p_k) | l_k sin(2 pi x_k / p_k)] (2 l sin(pi r / p) is the chord between two
 * such points), so a description with a Periodic part takes the K-assembly paths of feature
 * width 2d.  Derivatives, with r_k = x_k - x'_k on raw x:
 *   dK/dsigma = (2 / |sigma|) K_p   (K_p with eps on a same-object diagonal, as for SE)
 *   dK/dl_k   = -2 l_k K (2 sin(pi r_k / p_k))^2          (eps meets r = 0 only)
 *   dK/dp_k   = (4 pi l_k^2 / p_k^2) K r_k sin(2 pi r_k / p_k)
 * Every per-stationary-part rule above holds for a Periodic part unchanged (LogScale's G .*= hp
 * covers the p entries).
 *
 * Derivatives with respect to an input (gpr_predict_grad), for the cross kernel k(x*, x) of a
 * test point x* and a training point x, r_k = x*_k - x_k on raw x:
 *   dk/dx*_k = -W dD/dx*_k,
 *   GPR_SE / GPR_M32 / GPR_M52   dD/dx*_k = 2 l_k^2 r_k
 *   GPR_PER                      dD/dx*_k = (4 pi l_k^2 / p_k) sin(2 pi r_k / p_k)
 * with W as above (GPR_PER: W = k).  A Matern part at a coincident point has a finite W and
 * r = 0, so the term is 0.  A WhiteNoise part contributes nothing: the cross kernel has no noise.
 *
 * Product terms (GPR_MUL, no counterpart in the reference).  A kernel is a sum of TERMS; a term is
 * one GPR_WN or the product of 1 to 4 stationary factors.  GPR_MUL is an infix marker inside
 * kinds[]: {GPR_SE, GPR_MUL, GPR_PER, GPR_WN} is SE * PER + WN.  A description without a marker
 * means exactly what it meant before (every part a term of its own).  hp stays the concatenation
 * of the parts' own layouts in order, markers skipped: each factor keeps its [sigma, l_1..l_d]
 * (GPR_PER: [sigma, l.., p..]), so a product of F factors has F sigmas of which only the product
 * is identifiable -- accepted; nothing is tied and there is no "constant" kind.
 * With k_f = sigma_f^2 f_f(D_f) the factor's value without eps:
 *   T = prod_f k_f, plus eps ONCE PER TERM on a same-object diagonal (the rule "eps once per
 *   stationary part" with "part" read as "summand"; a term of one factor is unchanged bit for bit);
 *   K = the terms added in order; the noise is the first GPR_WN's sigma_n^2 in the GPR_SELF form;
 *   the diagonal-variance prior is the sum over terms of prod_f sigma_f^2 (GPR_WN: sigma_n^2).
 * Derivatives, for factor f of term T with the cofactor C_f = prod_{g != f} k_g (formed as a
 * product, never as T / k_f, which underflows):
 *   dK/dsigma_f = (2 / |sigma_f|) T           (T with its eps on a same-object diagonal)
 *   dK/dl_k, dK/dp_k, dk/dx*_k: factor f's own formula above with W_f C_f for W_f; dk/dx*_k of a
 *   term is the sum of these over its factors.  LogScale is unchanged (G .*= hp).
 * Refused before anything is computed or written -- GPR_E_ARG, the message names the position in
 * kinds[]: a marker first, last or doubled, a marker next to GPR_WN; GPR_E_UNSUP: a term of more
 * than 4 factors.  `*` is not distributed over `+` (that would duplicate hyper-parameters).
 *
 * Calls built on SquaredExp's separability or its closed-form erf integrals refuse a description
 * with a Matern or Periodic part or a product marker -- GPR_E_UNSUP, the message names the part, nothing is computed or written:
 * gpr_split_predict, gpr_split_predict_rows, gpr_split_predict_shard, gpr_split_predict_mgpu,
 * gpr_split_factors, gpr_integrate, gpr_integrate_noise.  (gpr_antideriv_se takes no kinds: it
 * is SquaredExp's integral of whatever hp it is given.) */

/* predict modes (src/predict.jl:14-25) */
#define GPR_PREDICT_MEAN 0  /* predict_mean  src/predict.jl:6-12                     */
#define GPR_PREDICT_DIAG 1  /* predict(...; diagonal_var=true)                       */
#define GPR_PREDICT_FULL 2  /* predict(...; diagonal_var=false)                      */

/* cross-validation losses (src/loss_grad.jl:12-30) */
#define GPR_COST_MSE 1         /* MSE:  sum((y - yp)^2) / length(y)                   */
#define GPR_COST_CHISQ 2       /* ChiSq: sum((y - yp)^2 / Sigma_p[i, i])              */
#define GPR_COST_MAHALANOBIS 3 /* Mahalanobis: ||L^{-1}(y - yp)||^2, Sigma_p = L L^T   */
/* leave-one-out only (gpr_loo, gpr_loo_grad; gpr_cv_batch / gpr_cv_kfold refuse it): the negative
 * log predictive density, 0.5 log var + (y - yp)^2 / (2 var) + 0.5 log 2pi  (R&W eq. 5.10) */
#define GPR_COST_LOGPRED 4

typedef struct gpr_ctx* gpr_ctx_t;

/* ---- context & memory ------------------------------------------------------------- */
/* stream: a hipStream_t to run on (NULL = the context creates its own non-blocking one). */
int gpr_ctx_create(int device, void* stream, gpr_ctx_t* out);
int gpr_ctx_destroy(gpr_ctx_t ctx);
const char* gpr_last_error(gpr_ctx_t ctx);
const char* gpr_version(void);
int gpr_sync(gpr_ctx_t ctx);
void* gpr_ctx_stream(gpr_ctx_t ctx);
int gpr_malloc(gpr_ctx_t ctx, size_t bytes, void** dptr);
int gpr_free(gpr_ctx_t ctx, void* dptr);
int gpr_upload(gpr_ctx_t ctx, void* dst, const void* src, size_t bytes);   /* sync H2D */
int gpr_download(gpr_ctx_t ctx, void* dst, const void* src, size_t bytes); /* sync D2H */
/* Inner panel width of the blocked factorisations: 64 or 128 (default 128). */
int gpr_set_block(gpr_ctx_t ctx, int nb);
/* Outer panel width = K of the big MFMA trailing updates (default 1024, multiple of nb). */
int gpr_set_outer_block(gpr_ctx_t ctx, int nb2);
/* Per-kernel-class timing with HIP events on the context stream (bench instrumentation).
 * class: 0 K-assembly, 1 POTRF trailing update (SYRK), 2 POTRF panel (diag+TRSM),
 *        3 TRSM trailing GEMM, 4 other (call-site classes), 5 every launch of the
 *        pipelined MFMA GEMM kernel (kernel-level, overlaps 1-4), 6 tile-DAG factorisation
 *        launches (with any right-hand sides they solve), 7 solve-only tile-DAG launches
 *        (U^{-T} B from a finished factor: C5's variance rows, POTRI's Z), 8 / 9 the mean /
 *        variance pass of gpr_predict_grad (its kernels and their fixed-order sum), 10 the solve
 *        that makes its Q (call-level: the launches inside it also count in their own classes),
 *        11 the append's skinny solve (V = U^{-T} K(x, x_new) of gpr_fit_append, whichever route
 *        takes it; call-level too; the flops slot carries n0^2 m), 12 the rank-r update of
 *        gpr_fit_remove (its W rows and every launch of either route; call-level), 13 / 14 the
 *        fold Grams / per-fold solves of gpr_cv_kfold, 15 the small kernels of the leave-one-out
 *        entries (diag K^{-1}, per-point terms, b = P f_alpha, row scaling, pre-fill, mirror),
 *        16 gpr_loo_grad's SYRK (call-site class; the flops slot carries n^2 (n + 1)).
 *        Returns accumulated ms, launch count, flops (bytes for class 0). */
/* Knobs: the library's run-time switches.  Each is a GPR_* environment variable read ONCE,
 * when a context is created, and can be changed on a live context with gpr_set_knob (values
 * are doubles, integer knobs truncate).  None of them changes a result beyond rounding: they
 * pick between equivalent code paths or size workspaces.  Unknown names: GPR_E_ARG.
 *   GPR_DAG            1  factorisations as one persistent tile-DAG launch; 0: the blocked
 *                         two-stream factorisation (inner nb, outer nb2)
 *   GPR_DAG_TAIL   12288  blocked path: the last <= this many columns go to the tile-DAG (0 off)
 *   GPR_DAG_SOLVE     -1  solves from a finished factor as solve-only tile-DAG launches
 *                         (-1 auto: n >= 8192 with >= n right-hand sides; 0 never; 1 always)
 *   GPR_DAG_GRAM       1  gpr_fit_kinv: K^{-1} = Z^T Z as gram tasks of the DAG launch
 *   GPR_DAG_ZLAG       4  DAG: Z = U^{-T}'s row i scheduled after A's row i + lag
 *   GPR_DAG_RGROUP     4  DAG ticket order of plain launches (factorisation with general
 *                         right-hand sides, solve-only): tile rows taken 1 (row order), 2 or 4
 *                         at a time (other values round down), a group's tasks merged by column
 *                         so the readers of a column panel run together; lower-triangular /
 *                         gram / batched launches keep row order.  Results are bit for bit the
 *                         same for every value.  Measured, C3 job: 293.0 (1) -> 286.0 ms (4)
 *   GPR_DAG_RSKEW      0  ... member r of a group r * skew column slots behind member 0
 *                         (every skew > 0 measured slower)
 *   GPR_DAG_RGROUP_MIN 32 ... first grouped tile row (rounded up to a multiple of the group;
 *                         launches of fewer tile rows keep row order)
 *   GPR_FUSED_RHS     -1  gpr_fit_predict: [K(x, xp) | y] solved inside the factorisation
 *                         (-1 auto, 0 after it, 1 own stream, 2 main stream; blocked path)
 *   GPR_FUSE_Y         1  gpr_fit: z = U^{-T} y inside the factorisation
 *   GPR_FUSE_KINV     -1  gpr_fit_kinv: Z (1) and Z^T Z (2) inside the factorisation (-1 = 2)
 *   GPR_KBUILD_UPPER   1  fits assemble only what dpotrf 'U' reads (the DAG mirrors the rest)
 *   GPR_KBUILD_EXACT   0  1: K by the reference's difference form instead of the Gram form
 *   GPR_KBUILD_GRAM_MAXD 1073741824  largest input dimension d whose K takes the Gram form on
 *                         FP64 MFMA (d <= 20: kernels compiled per ceil(d/4); above: the
 *                         runtime-d tile); 20: the difference form for every d > 20
 *   GPR_KBUILD_COLSTORE 1 single-part (SE) upper builds store 1-KB column segments through LDS;
 *                         0: the MFMA D layout (4 columns x 128 B per store instruction)
 *   GPR_KBUILD_TILES   0  1: a single SquaredExp part's symmetric K by the mirrored 64 x 64 tiles
 *                         every other description takes, instead of its column build (A/B runs:
 *                         bench_matern.py times SE and Matern through the same kernels)
 *   GPR_CV_BATCH       1  gpr_cv_batch: every fold in one batched launch; 0: per fold
 *   GPR_CV_BATCH_GB   16  device-memory budget of one batched cross-validation launch
 *   GPR_CV_KFOLD_GRAM -1  gpr_cv_kfold: a fold's block P_FF of K^{-1} as the Gram of the fold's columns
 *                         of Z = U^{-T} (1: the full K^{-1} is never formed), or gathered from the
 *                         full K^{-1} = Z^T Z of gpr_fit_kinv's route (0: the plain statement of the
 *                         method, kept as the cross-check); -1 auto: the Grams for folds of up to
 *                         128 points, the gather above.  The two agree within rounding.  Measured at
 *                         n = 8192, Gram vs gather: 64 folds of 128 9.8 vs 11.7 ms, 10 folds of 819
 *                         (one SYRK per fold) 27.0 vs 20.1 ms; n = 16384, 256 folds of 64 50.2 vs 68.5
 *   GPR_CV_STREAMS     4  child contexts of the per-fold / per-column paths (<= 8)
 *   GPR_QUAD_EIGEN    -1  gpr_integrate_noise: -1 auto (measured cost model), 0 per-column
 *                         factorisations, 1 tridiagonal reduction + per-column tridiagonal
 *                         solves, 3 full eigendecomposition (reduction + divide and conquer),
 *                         4 the same by block Jacobi (2, rocSOLVER dsyevd as a timing
 *                         comparator, exists only in the test build libgpr_hip_testing.so)
 *   GPR_QUAD_BATCH_GB 16  device-memory budget of one batched quadrature launch
 *   GPR_QUAD_SEQ       0  1: the per-column factorisations one at a time (no batch)
 *   GPR_PGRAD_SLAB  1024  gpr_predict_grad: training points per workgroup (the slab whose partial
 *                         sums a workgroup writes; rounded up to a multiple of 64, at least 64).
 *                         Changes how the sum over the training points is cut, nothing else
 *   GPR_PGRAD_SOLVE   -1  gpr_predict_grad, want_var: Q = K^{-1} K(x, xp) by gpr_potrs_upper's
 *                         sweeps (0: one pass over U per two columns) or by Z = U^{-T} and two
 *                         MFMA products, Q = Z^T (U^{-T} K(x, xp)) (1: n^2 + n m doubles of
 *                         workspace); -1 auto: the products for m > max(16, n / 512).  Measured at
 *                         n = 32768, m = 8192: 26.7 s by the sweeps, 535 ms by the products
 *   GPR_APPEND_SWEEP  -1  gpr_fit_append: V = U^{-T} K(x, x_new) by the single-launch skinny sweep
 *                         (1: for m <= 128 with the default 128 block, one pass over U per 16
 *                         columns) or by the GEMM-based solve of gpr_trsm_upper_trans (0); -1 auto:
 *                         the sweep for m <= 48.  Measured at n0 = 32768 - m, sweep vs the GEMM
 *                         route: m = 1 1.78 vs 10.4 ms, 16 2.36 vs 9.0, 48 7.05 vs 9.1, 64 9.39 vs 9.18
 *   GPR_REMOVE_SWEEP  -1  gpr_fit_remove: the rank-r update of the factor as one persistent launch per
 *                         group of 8 removed points (1: a workgroup per 128-column block, the
 *                         rotations handed from block to block inside the launch) or as one diagonal
 *                         and one panel launch per 128-row block (0); -1 auto: the launch chain,
 *                         which measured faster at n0 = 32768 (r = 1 oldest: 16.1 vs 19.1 ms per update,
 *                         r = 128: 316 vs 427).  The two agree bit for bit
 * A gpr_mgpu handle has knobs of its own, read from the environment once at gpr_mgpu_create
 * and changed with gpr_mgpu_set_knob / gpr_mgpu_get_knob (below):
 *   GPR_MGPU_STREAM   -1  1: stream U out during device 0's fit; 0: after it (-1 auto: only
 *                         for one device)
 *   GPR_MGPU_CHUNKS   16  tile-row chunks of the broadcast (>= 1)
 *   GPR_MGPU_RESERVE_CU 8 CUs the streamed fit's launch leaves to the chunks' packs and RCCL
 * Fault injection (forced wait timeouts, failed unpacks, a one-device handle broadcasting to
 * itself) exists only in the test build libgpr_hip_testing.so. */
int gpr_set_knob(gpr_ctx_t ctx, const char* name, double value);
int gpr_get_knob(gpr_ctx_t ctx, const char* name, double* value);
int gpr_timing_enable(gpr_ctx_t ctx, int on);
int gpr_timing_get(gpr_ctx_t ctx, int cls, double* ms, long long* launches, double* flops);
int gpr_timing_reset(gpr_ctx_t ctx);

/* ---- a2/a3: kernel matrices --------------------------------------------------------- */
/* `same` argument of gpr_kernel: which of the reference's kernel! forms is meant.        */
#define GPR_CROSS 0       /* kernel!(K, cov, hp, x, xp), x !== xp: no eps, no noise         */
#define GPR_SELF 1        /* kernel!(K, cov, hp, x) (4-arg): eps per stationary part + sigma_n^2 of */
                          /* the first WhiteNoise part (add_noise!, src/compose_covar.jl:73) */
#define GPR_SAME_OBJECT 2 /* kernel!(K, cov, hp, x, xp) with x === xp (5-arg): eps per stationary */
                          /* part, NO noise (src/compose_covar.jl:47-61, covariance.jl:52-56)*/

/* K[n x m] (ldk) = kernel(cov, hp, x, xp).  same = GPR_SELF or GPR_SAME_OBJECT: dXp is
 * ignored and m must equal n (the symmetric matrix is written in full).  For a single
 * SquaredExp the two same-object forms coincide (eps only); they differ for composed
 * kernels with a WhiteNoise part, where only the 4-arg form adds sigma_n^2.
 * Replaces kernel!(kern, ::SquaredExp, hp, x, xp) src/covariance.jl:49-58,85-95,
 * kernel!(kern::AbstractGPUArray, ...) src/covar_gpu.jl:1-18 and
 * kernel!(kern, ::ComposedKernel, hp, x[, xp]) src/compose_covar.jl:47-77. */
int gpr_kernel(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
               const double* dX, int n, const double* dXp, int m, int same, double eps,
               double* dK, int ldk);

/* a4: dK/dtheta_i (1-based i) materialised, n x n.  WN part: writes 2*sigma_n*I; a stationary
 * part: the rules above with its own W.
 * Replaces grad!(::SquaredExp, DK, i, hp, x, K) src/deriv_covar.jl:20-32 and the
 * composed index mapping src/compose_covar.jl:109-123. */
int gpr_kernel_grad(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                    const double* dX, int n, int i, double eps, double* dDK, int ld);

/* ---- a5-a7: factor / solve --------------------------------------------------------- */
/* In-place upper Cholesky of the SPD matrix in dA (n x n, lda): upper triangle <- U with
 * K = U^T U, strict lower triangle untouched.  *info = 0 or the order of the failing
 * minor.  Replaces cholesky!(Hermitian(K)) = dpotrf('U') (src/cost.jl:77,87,104,
 * src/predict.jl:31).  The context keeps the inverses of the diagonal blocks for the
 * following gpr_potrs/gpr_trsm/gpr_potri calls on the same factor.
 * Implementation: one persistent tile-DAG launch (128 x 128 tile tasks); n and lda
 * multiples of 16 with a 128-B aligned dA are factored in place, other shapes on a padded
 * device copy (n rounded up to 16: an extra ~8 n^2 bytes of device memory, same result);
 * the knob GPR_DAG=0 selects the blocked two-stream factorisation. */
int gpr_potrf_upper(gpr_ctx_t ctx, double* dA, int n, int lda, int* info);

/* The context caches the factor's block inverses (and the outer squares' inverses) after a
 * factorisation or a first solve, keyed on the factor's device pointer and shape.  A factor
 * written into a buffer by anything other than this context (a broadcast, a copy, another
 * context) must be announced with gpr_forget_factor, or a following solve on the same pointer
 * reuses inverses of the previous contents. */
int gpr_forget_factor(gpr_ctx_t ctx);

/* B <- K^{-1} B for K = U^T U (dU from gpr_potrf_upper), B n x nrhs (ldb).
 * Replaces ldiv!(alpha, kchol, y) = dpotrs (src/cost.jl:79,89,106, src/predict.jl:32). */
int gpr_potrs_upper(gpr_ctx_t ctx, const double* dU, int n, int ldu, double* dB, int nrhs,
                    int ldb);

/* B <- U^{-T} B (left, upper, transposed triangular solve).  With B = K(x, xp)^T this is
 * rdiv!(Kxp, kchol.U) (src/predict.jl:84,90,98) in the transposed layout. */
int gpr_trsm_upper_trans(gpr_ctx_t ctx, const double* dU, int n, int ldu, double* dB,
                         int nrhs, int ldb);

/* Full symmetric K^{-1} (n x n, ldk) from the factor.  Replaces
 * K^-1 = I ; ldiv!(kchol, K^-1) (src/cost.jl:90-92,107-109). */
int gpr_potri_upper(gpr_ctx_t ctx, const double* dU, int n, int ldu, double* dKinv, int ldk);

/* ---- a8/a9: marginal likelihood ------------------------------------------------------ */
/* *out = 0.5 (y.alpha + 2 sum log U_ii + n log 2pi)  (src/loss_grad.jl:39-41). */
int gpr_mll(gpr_ctx_t ctx, const double* dU, int n, int ldu, const double* dy,
            const double* dalpha, double* out);

/* grad[D] (host) of the negative log-marginal-likelihood w.r.t. hp, fused over all D
 * hyper-parameters in one pass over the upper triangle of K^{-1} (never materialising
 * dK): g_i = -0.5 sum_ab (alpha_a alpha_b - Kinv_ab) dK_i,ab.  Replaces the grad! loop of
 * src/cost.jl:119-126 with src/loss_grad.jl:43-52 and src/deriv_covar.jl:20-32.  Any d (d <= 32:
 * the row point and its d sums in registers; above: per tile the 16 weights first, then the
 * length-scale sums 32 dimensions at a time) and any number of parts.
 * log_scale != 0 applies G .*= hp (src/cost.jl:60-70). */
int gpr_mll_grad(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                 const double* dX, int n, const double* dKinv, int ldk,
                 const double* dalpha, double eps, int log_scale, double* grad);

/* One-call fit = update_cache!(MllLossCache / GPRPredictCache) (src/cost.jl:74-81,
 * src/predict.jl:29-34): dK (n x n, ldk) <- kernel, then in-place POTRF, then
 * dalpha <- K^{-1} dy (nrhs columns, ldy).  Returns info > 0 if not PD. */
int gpr_fit(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
            const double* dX, int n, const double* dy, int nrhs, int ldy, double eps,
            double* dK, int ldk, double* dalpha, int* info);

/* Condition a fitted model on m more observations without refactoring it (no counterpart in the
 * reference, whose only route is update_cache! on all points).  dX: d x (n0 + m), the m new points
 * its last m columns; dy: (n0 + m) x nrhs (ldy).  dK (ldk >= n0 + m): on entry its leading n0 x n0
 * is what gpr_fit left for the first n0 points under the same kinds, hp and eps (U in the upper
 * triangle, K strictly below).  dalpha0: the old K^{-1} y, n0 x nrhs with leading dimension n0,
 * read only; dalpha: (n0 + m) x nrhs with leading dimension n0 + m, receives the new K^{-1} y and
 * must be distinct from dalpha0.
 * On return with *info = 0 the leading (n0 + m) x (n0 + m) of dK is what gpr_fit on all n0 + m
 * points would have left (within rounding): the factor in the upper triangle, K in the GPR_SELF
 * form strictly below (the new diagonal block with eps per stationary part and the first
 * WhiteNoise's sigma_n^2, the cross block the plain cross kernel); the old n0 x n0 block is not
 * rewritten.  With B = K(x, x_new), V = U^{-T} B, S = K_new - V^T V = R^T R the new factor is
 * [U V; 0 R], and alpha by the block formula: alpha_tail = S^{-1} (y_new - B^T alpha0),
 * alpha_head = alpha0 - U^{-1} (V alpha_tail) -- O(n0^2 m) work.  V for m <= 128 by one
 * persistent launch per 16 columns that reads the upper triangle of U once (GPR_APPEND_SWEEP),
 * wider appends by the GEMM-based solve of gpr_trsm_upper_trans; V^T V summed over slabs of n0 in
 * a fixed order (no atomics): two calls on the same inputs agree bit for bit.
 * The context's factor cache is left valid for the extended factor (the block inverses from block
 * n0 / 128 on are recomputed; a cached factor other than this buffer is established first, as any
 * solve does): gpr_predict, gpr_predict_grad, gpr_mll, gpr_potrs_upper, gpr_mvn_sample on
 * (dK, n0 + m, ldk) follow with no gpr_forget_factor.
 * A Schur complement that is not positive definite: *info = n0 + j (j the order of its failing
 * minor -- what dpotrf on the whole matrix gives), also the return value; the leading n0 x n0 of dK
 * and dalpha0 are untouched, the old model stays usable.  GPR_E_ARG for m < 1, n0 < 1,
 * ldk < n0 + m, ldy < n0 + m, nrhs < 1, a NULL pointer or dalpha == dalpha0: the message names the
 * argument, nothing is written.  Every kind, any d, any number of parts, any n0 and m >= 1.
 * Synchronises for info, as gpr_fit. */
int gpr_fit_append(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                   const double* dX, int n0, int m, const double* dy, int nrhs, int ldy,
                   double eps, double* dK, int ldk, const double* dalpha0, double* dalpha,
                   int* info);

/* Take r observations out of a fitted model without refactoring it (no counterpart in the
 * reference, whose only route is update_cache! on the remaining points).  dK (n0 x n0, ldk): what
 * gpr_fit left (U in the upper triangle, K strictly below); read only, left bit for bit as it was:
 * the old model stays usable.  idx: r HOST indices, 0-based, strictly ascending.  dy: the y of the
 * KEPT points, (n0 - r) x nrhs (ldy).  dKout (ldo >= n0 - r) must not overlap dK; its leading
 * (n0 - r) x (n0 - r) receives what gpr_fit on the kept points would have left (within rounding): U'
 * in the upper triangle, K strictly below (the old entries, compacted); nothing else is written.
 * dalpha: (n0 - r) x nrhs with leading dimension n0 - r, receives K'^{-1} y by the two sweeps of
 * gpr_potrs_upper on dKout.  No kinds, hp or X: nothing is evaluated, so every kernel description
 * is served.
 * With keep the remaining indices, T = U[keep, keep] and W = U[D, keep] (entries left of a removed
 * point's own column masked to zero), K[keep, keep] = T^T T + W^T W: U' is T after a rank-r positive
 * update by Givens rotations (rows ascending, removed points ascending within a row, 8 removed
 * points per pass over the triangle) -- O(n^2 r) work, no pivot can fail, hence no info.  Rows above
 * the first removed point's 128-row block are copied; removing only the newest points is a pure
 * copy.  Two routes (GPR_REMOVE_SWEEP) with the same arithmetic on every element: they, and two
 * calls of one route, agree bit for bit.
 * The context's factor cache is left valid for dKout: gpr_predict, gpr_predict_grad, gpr_mll,
 * gpr_potrs_upper, gpr_mvn_sample, gpr_fit_append on (dKout, n0 - r, ldo) follow with no
 * gpr_forget_factor.
 * GPR_E_ARG for r < 1, r >= n0, nrhs < 1, ldk < n0, ldo < n0 - r, ldy < n0 - r, a NULL pointer, idx
 * not strictly ascending or outside [0, n0), dKout overlapping dK: the message names the argument,
 * nothing is written.  Synchronises before it returns. */
int gpr_fit_remove(gpr_ctx_t ctx, const double* dK, int n0, int ldk, const int* idx, int r,
                   const double* dy, int nrhs, int ldy, double* dKout, int ldo, double* dalpha);

/* ---- a10/a11: posterior ------------------------------------------------------------ */
/* Posterior at m test points from a fitted factor (dU, dwt = K^{-1} y with nrhs cols).
 * mode GPR_PREDICT_MEAN: dmu (m x nrhs, ldmu=m).  GPR_PREDICT_DIAG: + dvar[m] =
 * prior - ||U^{-T} k_j||^2 (prior sigma^2 or sum of all parts' hp[1]^2, no eps:
 * src/predict.jl:51-71,89-95).  GPR_PREDICT_FULL: + dvar (m x m, ldv) = K(xp,xp) -
 * V^T V (src/predict.jl:42-49,83-87).  dwork: optional device scratch of n*m doubles
 * (NULL: the context allocates it).  Replaces predict!/predict_mean! src/predict.jl.
 * Same-object rule: dXp == dX (with m == n) is the C analogue of `xp === md.x`; then
 * K(xp, x) takes the reference's same-object branch of kernel!(Kxp, covar, hp, xp, md.x)
 * (src/predict.jl:37,43): eps once per SE part on its diagonal, no noise
 * (src/covariance.jl:52-56, src/compose_covar.jl:47-61).  Any other dXp: cross kernel. */
int gpr_predict(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                const double* dX, int n, const double* dU, int ldu, const double* dwt,
                int nrhs, const double* dXp, int m, int mode, double eps, double* dmu,
                double* dvar, int ldv, double* dwork);

/* Gradients of the posterior w.r.t. the test inputs, from a fitted factor (as gpr_predict).
 * dgmu : d x m x nrhs, column-major, leading dimension d (a test point's gradient is
 *        contiguous, as the point itself is in dXp);  dgmu[k, j, c] = d mu_c(xp_j) / d xp_kj
 * dgvar: d x m (want_var != 0, else may be NULL): d sigma^2(xp_j) / d xp_kj of the DIAG variance
 * dwork: optional n*m doubles (want_var; NULL: the context allocates)
 * No counterpart in the reference.  With alpha = dwt and Q = K^{-1} K(x, xp) (the cross build and a
 * solve from the factor, want_var only: GPR_PGRAD_SOLVE), one fused pass each, never
 * materialising a dK matrix:
 *   dgmu[k, j]  =      sum_p sum_i alpha_i (-W_p(xp_j, x_i)) dD_p/dxp_kj     (per column of dwt)
 *   dgvar[k, j] = -2   sum_p sum_i Q_ij    (-W_p(xp_j, x_i)) dD_p/dxp_kj
 * over the stationary parts p (the rules are in the opening comment).  Every kind, any d >= 1 and
 * any number of parts (d <= 32 without a Periodic part: the test point and its d sums in
 * registers; else 32 dimensions at a time, Periodic 16).
 * ALWAYS the cross kernel: the gradients are those of the smooth function x* -> (mu, sigma^2), so
 * dXp == dX gets NO same-object treatment here (unlike gpr_predict) -- the same-object eps is a
 * point mass on the diagonal and has no derivative.  eps is taken only to build the description.
 * The sum over i is cut into slabs of GPR_PGRAD_SLAB training points whose partial sums are added
 * in a fixed order (no atomics): two calls on the same inputs agree bit for bit.  Asynchronous.
 * Argument errors: GPR_E_ARG, the message names the argument, nothing is written. */
int gpr_predict_grad(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                     const double* dX, int n, const double* dU, int ldu, const double* dwt,
                     int nrhs, const double* dXp, int m, int want_var, double eps,
                     double* dgmu, double* dgvar, double* dwork);

/* ---- a5/a6/a7 fused: update_cache!(::MllGradCache) = K, cholesky!, alpha, K^{-1} --------- */
/* src/cost.jl:83-111 in one call: K into dK (upper -> U, lower keeps K), alpha = K^{-1} y
 * (n x nrhs), dKinv = full symmetric K^{-1} (ldkinv).  Z = U^{-T} and K^{-1} = Z^T Z are
 * computed inside the factorisation: as right-hand-side and gram tile tasks of the one
 * tile-DAG launch (n a multiple of 16, 128-B aligned dK), else in the blocked
 * factorisation's lookahead bubbles (GPR_FUSE_KINV=1: Z alone inside, 0: both after it).
 * Device workspace: n^2 doubles for Z.  >0: LAPACK info. */
int gpr_fit_kinv(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                 const double* dX, int n, const double* dy, int nrhs, int ldy, double eps,
                 double* dK, int ldk, double* dalpha, double* dKinv, int ldkinv, int* info);

/* ---- a5/a6/a10/a11 fused: predict(md, xp; diagonal_var) from scratch ---------------- */
/* The reference's predict (src/predict.jl:14-25 -> update_cache!(pc, md) :29-34 = K, cholesky!,
 * ldiv!(wt, kchol, md.y), then predict! :36-71) in one call: K(x, x) into dK (upper
 * overwritten by U, lower keeps K, as gpr_fit), posterior mean/variance at m test points as
 * gpr_predict.  With mode DIAG/FULL the triangular solve of [K(x, xp) | y] runs inside the
 * factorisation (right-hand-side tile tasks of the tile-DAG launch; on the blocked path outer
 * block s is solved once panel s of U is final), mu = V^T z with
 * V = U^{-T} K(x, xp), z = U^{-T} y; dalpha (optional, n x nrhs) = K^{-1} y.  dwork: optional
 * n*(m+nrhs) doubles.  Returns >0 (LAPACK info) for a non-PD K.  dXp == dX: the
 * same-object rule of gpr_predict (K(xp, x) gets eps per SE part, no noise). */
int gpr_fit_predict(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                    const double* dX, int n, const double* dy, int nrhs, int ldy, double eps,
                    double* dK, int ldk, double* dalpha, const double* dXp, int m, int mode,
                    double* dmu, double* dvar, int ldv, double* dwork, int* info);

/* ---- sampling: NormalDistribution / GaussianProcess / sample (src/distributions.jl) ---- */
/* dZ[i] = element (offset + i) of the standard-normal stream of `seed`, i < count.  In place
 * of randn(rng, dim) (src/distributions.jl:27); Julia's Xoshiro / ziggurat stream is NOT
 * reproduced: a caller who needs the reference's numbers uploads its own z.  The stream is
 * counter-based, so an element depends on (seed, offset + i) alone, never on how a range is
 * cut into calls: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9,
 * 0xBB67AE85), counter (lo32(g >> 1), hi32(g >> 1), 0, 0) and key (lo32(seed), hi32(seed)) for
 * global index g; from the output words w0..w3, u1 = (((w1 << 32 | w0) >> 11) + 0.5) 2^-53, u2
 * likewise from (w3, w2), r = sqrt(-2 ln u1); element g = r cos(2 pi u2) for even g,
 * r sin(2 pi u2) for odd g.  Asynchronous. */
int gpr_randn(gpr_ctx_t ctx, uint64_t seed, uint64_t offset, double* dZ, size_t count);

/* S (n x ns, lds) = mu 1^T + U^T Z: s .= N.Sigma_ch.L * s .+ N.mu (src/distributions.jl:28) for
 * ns draws at once.  U = the upper triangle of the factor buffer dU (n x n, ldu; from
 * gpr_potrf_upper, gpr_fit, gpr_mvn_factor, ...): whatever lies below its diagonal -- K after a
 * fit -- is masked while the diagonal tiles are staged, never multiplied (a NaN there does not
 * reach S), and row tile t of the product reads k < min(n, 128 (t + 1)) only.  Z: n x ns (ldz);
 * dmu: device n-vector or NULL (zeros).  FP64 MFMA; any n, ns >= 1, ldu, ldz, lds >= n.  dS
 * overlapping dZ, dU or dmu: GPR_E_ARG.  Asynchronous. */
int gpr_mvn_sample(gpr_ctx_t ctx, const double* dU, int n, int ldu, const double* dmu,
                   const double* dZ, int ns, int ldz, double* dS, int lds);

/* NormalDistribution(mu, Sigma) (src/distributions.jl:20-23): Sigma_ch = cholesky(Sigma .+ 1e-7),
 * the shift added to EVERY element of the matrix that is factored, not to its diagonal.  dA
 * (n x n, lda) holds the symmetric Sigma; on return its upper triangle holds U with
 * U^T U = Sigma .+ shift, its strict lower triangle is untouched.  Returns *info > 0 (the order
 * of the failing minor, PosDefException) otherwise 0; synchronises for info. */
int gpr_mvn_factor(gpr_ctx_t ctx, double* dA, int n, int lda, double shift, int* info);

/* sample(gp(x, hp)) (src/distributions.jl:33,41-45 + :20-30) in one call: K = kernel!(K, cov,
 * hp, x) (the GPR_SELF form: eps per SE part + noise) into dK, K .+= shift, dpotrf 'U' in
 * place, S = mu 1^T + U^T Z (dmu = f_mu.(eachcol(x)) or NULL; Z n x ns, ldz; S n x ns, lds).  dK
 * ends as gpr_fit leaves it -- U in the upper triangle, the factored matrix (K .+ shift) in the
 * strict lower one -- and serves gpr_mvn_sample for further draws.  Returns *info > 0 for a
 * non-PD matrix (nothing is written to dS then); synchronises for info. */
int gpr_sample_prior(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                     const double* dX, int n, const double* dmu, double shift, double eps,
                     const double* dZ, int ns, int ldz, double* dK, int ldk, double* dS, int lds,
                     int* info);

/* ---- 8(f) rank 3: Bayesian quadrature of the posterior (src/integrate.jl) ------------- */
/* antideriv!(k1, SquaredExp(), x, hp, a, b) and antideriv2 (src/integrate.jl:16-46): dk1[n]
 * = sigma^2 (sqrt(pi)/2)^d prod(1/l) prod_i erf(l_i (a_i - x_i), l_i (b_i - x_i)) on the
 * device, *k2 = sigma^2 prod_i erf_integ(l_i, a_i, b_i) (host); hp[0] = sigma, hp[1..d] = l
 * (the first d + 1 entries, as the reference indexes md.params).  a, b: host d-vectors;
 * dk1 or k2 may be NULL. */
int gpr_antideriv_se(gpr_ctx_t ctx, int d, const double* hp, const double* dX, int n,
                     const double* a, const double* b, double* dk1, double* k2);
/* integrate(md, hp, a, b; sample_noise=nothing) (src/integrate.jl:48-167): fit (K into dK ->
 * U, dwt = K^{-1} y, n x ny), Iout[ny] = wt' k1, *var = k2 - ||U^{-T} k1||^2 (host outputs).
 * The sample_noise path (syevr + diagonal updates, :71-104) is gpr_integrate_noise below. */
int gpr_integrate(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                  const double* dX, int n, const double* dy, int ny, int ldy, const double* a,
                  const double* b, double eps, double* dK, int ldk, double* dwt, double* Iout,
                  double* var);

/* cv_batch(md, cost, x, y, (trn, tst)) (src/crossval.jl:13-35): for each fold f, fit the
 * model on the training points trn[f*ntrn .. +ntrn) of (dX, dy) and predict the test points
 * tst[f*ntst .. +ntst) with the FULL posterior covariance (cv_step!, :46-51 = update_cache!
 * + predict!), then lss[f] = loss(cost, ytst, yp, Sigma_p) with cost GPR_COST_*.
 * trn/tst: host arrays of 0-based point indices (< n), fold-major; lss: host, nfold.
 * dX: d x n column-major, dy: n.  Returns info > 0 if a training K (or, for Mahalanobis,
 * Sigma_p) is not positive definite -- the reference's PosDefException. */
int gpr_cv_batch(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                 const double* dX, int n, const double* dy, const int* trn, int ntrn,
                 const int* tst, int ntst, int nfold, int cost, double eps, double* lss);

/* Cross-validation of complementary folds from ONE factorisation of all n points.
 * Fold f tests tst[f*ntst .. +ntst) (host, 0-based, distinct within a fold) and trains on ALL
 * other points of (dX, dy).  lss[nfold] (host) = what gpr_cv_batch returns for trn[f] = the
 * complement of tst[f], within rounding.  mu, var: optional host arrays nfold*ntst, fold-major:
 * the posterior mean at the fold's test points and the diagonal of its Sigma_p.
 * With K the GPR_SELF matrix of all points, P = K^{-1} and alpha = K^{-1} y:
 * Sigma_p = (P_FF)^{-1} and y_F - yp = (P_FF)^{-1} alpha_F, exactly (Sigma_p is the Schur
 * complement of K_TT in K).  Folds may overlap and need not cover the points; any kernel
 * description, any d, n >= 2, 1 <= ntst < n; ntst = 1 over all points is leave-one-out
 * (mu_i = y_i - alpha_i / P_ii, var_i = 1 / P_ii).  Both routes (GPR_CV_KFOLD_GRAM) lose about
 * cond_2(K) u, as the reference's own Sigma_p = K_FF - V^T V does by cancellation.
 * GPR_E_ARG (naming the argument, nothing written) for a NULL pointer other than mu / var, an
 * index out of range, an index twice in a fold, ntst >= n, an unknown cost.  Returns info > 0
 * when K is not positive definite (dpotrf's info, as gpr_cv_batch) or a fold's P_FF fails to
 * factor in rounding; nothing is written then either. */
int gpr_cv_kfold(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                 const double* dX, int n, const double* dy, const int* tst, int ntst, int nfold,
                 int cost, double eps, double* lss, double* mu, double* var);

/* ---- leave-one-out training criteria (no counterpart in the reference, which ships only
 * MarginalLikelihood on its AbstractLoss seam, src/cost.jl) ------------------------------- */
/* With K the GPR_SELF matrix of all n points, P = K^{-1} and alpha = K^{-1} y (gpr_cv_kfold's
 * identities for one-point folds: yp_i = y_i - alpha_i / P_ii, var_i = 1 / P_ii) a criterion is
 * L = sum_i f(alpha_i, P_ii), crit one of
 *   GPR_COST_LOGPRED      f = -0.5 log P_ii + alpha_i^2 / (2 P_ii) + 0.5 log 2pi
 *   GPR_COST_MSE          f = (alpha_i / P_ii)^2
 *   GPR_COST_CHISQ        f = alpha_i^2 / P_ii      (GPR_COST_MAHALANOBIS on one point: the same)
 * the last three the SUM (not the mean) over the n one-point folds of gpr_cv_kfold's losses.
 *
 * One-call fit for the value alone: dK (n x n, ldk) <- kernel, in-place POTRF (upper U, strict
 * lower K, as gpr_fit), dalpha <- K^{-1} dy (one column), dpdiag[n] (device) <- diag(K^{-1}) as
 * the column norms of Z = U^{-T}, P_ii = sum_{k >= i} Z_ki^2: no Gram of Z is formed.  Z rides in
 * the factorisation as in gpr_fit_kinv (device workspace: n^2 doubles).  The front half of
 * gpr_cv_kfold.  Returns info > 0 if not PD; synchronises.  GPR_E_ARG as below. */
int gpr_fit_loo(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                const double* dX, int n, const double* dy, double eps, double* dK, int ldk,
                double* dalpha, double* dpdiag, int* info);

/* *out = L for crit, from alpha and P_ii = dp[i * incp]: incp = 1 reads gpr_fit_loo's dpdiag,
 * incp = ldkinv + 1 the diagonal of gpr_fit_kinv's dKinv.  One launch, the sum in a fixed order. */
int gpr_loo(gpr_ctx_t ctx, int crit, const double* dp, int incp, const double* dalpha, int n,
            double* out);

/* grad[D] (host) of L w.r.t. hp and, where value is not NULL, *value = L, from what gpr_fit_kinv
 * left: dKinv (n x n, ldk, symmetric in full) and dalpha are read only.  With b = P f_alpha,
 * s_i = sqrt(-f_P,i) (f_P <= 0 for every criterion) and S = diag(s) P:
 *   dL/dtheta_j = -sum_ab dK_j,ab [ 0.5 (b_a alpha_b + alpha_a b_b) - (S^T S)_ab ]
 * (R&W eq. 5.13 summed over the points; they quote O(n^3) PER hyper-parameter).  Here: the
 * per-point terms, b (one pass over P), S, then M = 2 S^T S - (b alpha^T + alpha b^T) on the
 * upper triangle by ONE SYRK on the pipelined FP64 MFMA GEMM, and the fused pass of gpr_mll_grad
 * with a = 0 and M in K^{-1}'s place -- all D components of every kind of part for one extra n^3
 * product.  log_scale != 0 applies G .*= hp.  Device workspace: two n^2 buffers of the context (S
 * where gpr_fit_kinv kept Z, and M).  Every sum in a fixed order: two calls on the same inputs
 * agree bit for bit.  Synchronises.
 * GPR_E_ARG for a NULL pointer other than value, n < 1, ldk < n, incp < 1 or an unknown crit:
 * the message names the argument, nothing is written. */
int gpr_loo_grad(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                 const double* dX, int n, const double* dKinv, int ldk, const double* dalpha,
                 double eps, int crit, int log_scale, double* value, double* grad);

/* integrate(md, hp, a, b; sample_noise = noise::Vector) (src/integrate.jl:71-100,149-162):
 * per column j of y (ny columns, noise[j] host), Iout[j] = k1' (K + noise_j I)^{-1} y_j and
 * var[j] = k2 - k1' (K + noise_j I)^{-1} k1.  The reference decomposes K = P Lambda P' once
 * (LAPACK syevr) and then only updates a diagonal per column.  Here, by default, one of:
 *  - the tridiagonal reduction K = Q T Q' (syevr's first stage, gpr_sytrd_apply, with
 *    C = Q' [y | k1] formed inside the reduction), then per column one pivoted tridiagonal
 *    solve: Iout[j] = C[:, j]' (T + noise_j I)^{-1} C[:, ny] -- any shift, no factorisation,
 *    never info > 0 (an indefinite K + noise_j I gives the reference's indefinite solve);
 *  - the K + noise_j I factored per column, all in one batched tile-DAG launch that also solves
 *    U_j^{-T} [y_j | k1] (same result within rounding), while that is measured to cost less
 *    (ny below ~175 at n = 4096, ~220 at 2048, ~330 at 1100, ~700 at 512, ~140 at 8192;
 *    always beyond the reduction's bound n > 16384); a factorisation that fails (a shift at or
 *    below -lambda_min(K)) hands the call to the reduction, so the default never returns
 *    info > 0 up to that bound.  A reduction whose cooperative launch the runtime refuses (its
 *    workgroups cannot all be resident) falls back to the factorisations.
 * GPR_QUAD_EIGEN forces a route: 1 the reduction; 3 the reference's full decomposition
 * (reduction + divide and conquer, gpr_syev_apply) and its diagonal updates; 0 always the
 * factorisations (positive definite shifts only; info > 0 -- PosDefException -- otherwise);
 * 2 rocSOLVER dsyevd -- a timing comparator compiled into the test build libgpr_hip_testing.so
 * only (GPR_E_ARG here). */
int gpr_integrate_noise(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                        const double* dX, int n, const double* dy, int ny, int ldy,
                        const double* a, const double* b, const double* noise, double eps,
                        double* Iout, double* var);

/* The symmetric eigendecomposition behind the sample_noise quadrature (LAPACK.syevr! at
 * src/integrate.jl:75), applied instead of returned: A (n x n, ld lda, device, read only,
 * symmetric) = P diag(lam) P'; on return dlam[n] (device) holds the eigenvalues -- in no
 * particular order -- and dB (n x m, ld ldb, device) holds P' B, its rows in the order of
 * dlam.  FP64, as dsyevd: the tridiagonal reduction (gpr_sytrd_apply, B <- Q' B) then Cuppen's
 * divide and conquer on T (deflation, secular equations, Gu-Eisenstat vectors; Z never formed:
 * B <- Z' B merge by merge).  n > 16384, or a reduction whose cooperative launch is refused:
 * two-sided block Jacobi (32-wide blocks, parallel ordering).  *sweeps (may be NULL) = merge levels (Jacobi: sweeps used).  GPR_E_HIP if Jacobi
 * does not converge within 60 sweeps. */
int gpr_syev_apply(gpr_ctx_t ctx, const double* dA, int n, int lda, double* dB, int m, int ldb,
                   double* dlam, int* sweeps);

/* The first stage of that decomposition on its own (LAPACK dsytrd, inside syevr): A (n x n,
 * ld lda, device, read only, symmetric -- both triangles read) = Q T Q^T with T tridiagonal:
 * dd[n] its diagonal, de[n-1] its off-diagonal (device), and, when m > 0, dB (n x m, ld ldb)
 * <- Q^T dB.  One persistent launch (the unblocked two-sided Householder reduction, columns
 * dealt round-robin over the CUs; for m <= 1024 Q^T B is formed inside it), else the
 * back-transform by 64-reflector blocks on the MFMA GEMM.  The launch is cooperative (every
 * workgroup resident or refused up front: GPR_E_UNSUP, nothing touched); below n = 5376 its
 * step vectors sit in LDS and every step updates every trailing column; from 5376 on the
 * updates are deferred by panels of 16 steps (later columns only read per step, flushed per
 * panel by an MFMA GEMM).  n <= 16384 (GPR_E_UNSUP beyond). */
int gpr_sytrd_apply(gpr_ctx_t ctx, const double* dA, int n, int lda, double* dB, int m, int ldb,
                    double* dd, double* de);

/* ---- a12-a15: split-kernel block prediction ---------------------------------------- */
/* Test grid x_{e,q} = xe_e + xq_q (Cmap(+, xe, xq), src/split_kernel.jl:1-17).
 * dmu: ne x nq column-major (index e + q*ne, src/split_predict.jl:10-19).
 * dvar: ne*nq diagonal; entries (e*nq + q) for e in [var_lo, var_hi) (0-based,
 * half-open; the reference default var_range=1:3 is [0,3)) get prior - ||U^{-T} k||^2,
 * every other entry is set to the prior (src/split_predict.jl:39-53).
 * e_lo/e_hi restrict the call to grid rows [e_lo, e_hi) (multi-GPU sharding: each rank
 * passes its own row range; dmu/dvar still index the FULL grid layout, only the rows in
 * range are written).  dwt is the 1-column K^{-1} y.
 * Replaces kernel!(::SplitKernel,...) src/split_kernel.jl:137-159 and
 * predict_split_mean_impl!/predict_covar_impl! src/split_predict.jl:5-53. */
int gpr_split_predict(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                      const double* dX, int ns, const double* dU, int ldu,
                      const double* dwt, const double* dXe, int ne, const double* dXq,
                      int nq, int e_lo, int e_hi, int var_lo, int var_hi, double eps,
                      double* dmu, double* dvar);

/* gpr_split_predict over several pieces of grid rows at once: pieces = host array of
 * npieces sorted, disjoint half-open ranges {lo_0, hi_0, lo_1, hi_1, ...} (a rank's shard:
 * an even share of the variance rows plus an even share of the rest, gpr_shard_pieces).  The
 * ns x nq C factor is built once per call instead of once per piece; dmu / dvar index the
 * full grid layout as in gpr_split_predict, only the rows in the pieces are written. */
int gpr_split_predict_rows(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                           const double* dX, int ns, const double* dU, int ldu, const double* dwt,
                           const double* dXe, int ne, const double* dXq, int nq, const int* pieces,
                           int npieces, int var_lo, int var_hi, double eps, double* dmu,
                           double* dvar);

/* gpr_split_predict_rows with outputs sized to the shard, not to the grid: the pieces' R rows
 * concatenated in piece order (row e of piece k at r = off_k + e - lo_k, off_k = rows of the
 * pieces before it).  dmu: R x nq column-major, leading dimension ldmu >= R (index r + q*ldmu);
 * dvar: R*nq (index r*nq + q).  What a rank of a multi-GPU split prediction allocates
 * (R ~ ne / ngpu rows instead of ne). */
int gpr_split_predict_shard(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                            const double* dX, int ns, const double* dU, int ldu,
                            const double* dwt, const double* dXe, int ne, const double* dXq,
                            int nq, const int* pieces, int npieces, int var_lo, int var_hi,
                            double eps, double* dmu, int ldmu, double* dvar);

/* Split factors for inspection/tests (src/split_kernel.jl:151-159), SE part `part`
 * (0-based among SE parts): dA ne x nq, dB ne x ns, dC ns x nq (column-major,
 * leading dims = row counts). */
int gpr_split_factors(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                      const double* dX, int ns, const double* dXe, int ne,
                      const double* dXq, int nq, int part, double* dA, double* dB,
                      double* dC);

/* ---- 8(e): split prediction sharded over the GPUs of one node, one host process ------- */
/* Row pieces of grid row count n for `rank` of `world`: an even share of the variance rows
 * [v_lo, v_hi) plus an even share of the others, as at most 3 sorted, disjoint, merged
 * half-open ranges written to pieces[0..5] ({lo, hi} pairs).  Returns their number (or < 0).
 * Host-only helper (no device work); the same partition as gpr_amd.distributed.shard_pieces. */
int gpr_shard_pieces(int n, int world, int rank, int v_lo, int v_hi, int* pieces);

/* The upper triangle of a column-major n x n factor packed by 128-column blocks (block
 * [j0, j1) keeps rows [0, j1) of its columns): gpr_packed_upper_len(n) ~ n^2/2 + 64 n doubles,
 * half the bytes of U for a broadcast.  Unpacking leaves the rest of dU untouched (no solve
 * reads it).  A Julia MPI caller broadcasting pc.Kxx between processes uses these pairs, then
 * gpr_forget_factor on the receivers. */
size_t gpr_packed_upper_len(int n);
int gpr_pack_upper(gpr_ctx_t ctx, const double* dU, int n, int ldu, double* dP);
int gpr_unpack_upper(gpr_ctx_t ctx, const double* dP, int n, double* dU, int ldu);

typedef struct gpr_mgpu* gpr_mgpu_t;
#define GPR_MGPU_BROADCAST 0 /* device 0 fits; RCCL broadcast of packed U + wt (xGMI)   */
#define GPR_MGPU_REPLICATE 1 /* every device fits for itself (no N^2 exchange)          */

/* A set of ngpu devices (distinct ids) with one context each and an RCCL communicator
 * (ncclCommInitAll; librccl.so.1 is dlopen'd: the process's own if loaded, else the
 * system's).  Create once, reuse across calls. */
int gpr_mgpu_create(int ngpu, const int* devices, gpr_mgpu_t* out);
int gpr_mgpu_destroy(gpr_mgpu_t h);
const char* gpr_mgpu_last_error(gpr_mgpu_t h);
/* The handle's knobs (GPR_MGPU_STREAM, GPR_MGPU_CHUNKS, GPR_MGPU_RESERVE_CU; see gpr_set_knob).
 * Unknown names: GPR_E_ARG. */
int gpr_mgpu_set_knob(gpr_mgpu_t h, const char* name, double value);
int gpr_mgpu_get_knob(gpr_mgpu_t h, const char* name, double* value);

/* predict(md, Cmap(+, xe, xq); diagonal_var=true) (src/predict.jl:14-25 ->
 * src/split_predict.jl:5-53) sharded over the handle's GPUs.  HOST arrays in and out (the
 * reference's CPU arrays): X d x ns, y ns, Xe d x ne, Xq d x nq; mu ne x nq column-major
 * (index e + q ne), var ne*nq (index e nq + q; rows outside [var_lo, var_hi) keep the prior).
 * fit_mode GPR_MGPU_BROADCAST / GPR_MGPU_REPLICATE.  Device i computes the rows
 * gpr_shard_pieces(ne, ngpu, i, var_lo, var_hi) and copies them into mu / var itself.
 * Returns > 0 (and *info) when K is not positive definite.  With ngpu = 1 the result equals
 * gpr_fit + gpr_split_predict on that device bit for bit.
 * Broadcast mode streams U out while device 0 factors it: chunks of 128-row tile rows
 * (GPR_MGPU_CHUNKS, default 16, about equal bytes) are packed and broadcast as soon as the
 * tile-DAG launch has finalised them, on a stream of their own and the GPR_MGPU_RESERVE_CU
 * (default 8) CUs the launch leaves free; the receivers unpack each chunk as it lands.
 * GPR_MGPU_STREAM=0 sends the same chunks after the fit instead. */
int gpr_split_predict_mgpu(gpr_mgpu_t h, const int* kinds, int nk, const double* hp, int d,
                           const double* X, int ns, const double* y, const double* Xe, int ne,
                           const double* Xq, int nq, int var_lo, int var_hi, double eps,
                           int fit_mode, double* mu, double* var, int* info);

#ifdef __cplusplus
}
#endif
#endif /* GPR_HIP_H */
