// Shared internals of libgpr_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <vector>

#include "../../include/gpr_hip.h"
#include "factor_cache.hpp"

#define KMAXP 4   // stationary parts one fused-kernel launch handles (more: groups of KMAXP)

// Radial profile of a stationary part: k = sigma^2 f(D) of the ARD-scaled squared distance D
// (kexp.hpp).  SE is the reference's; the two Matern profiles are this library's own.
enum { KPROF_SE = 0, KPROF_M32 = 1, KPROF_M52 = 2 };
inline bool kind_stationary(int kind) {
  return kind == GPR_SE || kind == GPR_M32 || kind == GPR_M52 || kind == GPR_PER;
}
// hyper-parameters of one part: [sigma, l_1..l_d] (SquaredExp, Matern), [sigma, l_1..l_d,
// p_1..p_d] (Periodic), [sigma_n] (WhiteNoise)
// (a product marker GPR_MUL owns none)
inline int kind_hp_width(int kind, int d) {
  return kind == GPR_MUL ? 0 : kind == GPR_WN ? 1 : kind == GPR_PER ? 2 * d + 1 : d + 1;
}
inline int kind_profile(int kind) {
  return kind == GPR_M32 ? KPROF_M32 : kind == GPR_M52 ? KPROF_M52 : KPROF_SE;
}
inline const char* kind_name(int kind) {
  return kind == GPR_SE ? "SquaredExp" : kind == GPR_M32 ? "Matern32" : kind == GPR_M52 ? "Matern52"
         : kind == GPR_PER ? "Periodic" : kind == GPR_WN ? "WhiteNoise"
         : kind == GPR_MUL ? "a product marker (GPR_MUL)" : "?";
}

// Kernel description passed BY VALUE to every assembly kernel (a few dozen bytes of kernargs;
// the per-part tables live in the context's parameter block, see KParBlock).
// Mirrors split(hp, dims) of src/compose_covar.jl:21-28: the stationary parts (SquaredExp,
// Matern32, Matern52: hp [sigma, l_1..l_d] each; Periodic: [sigma, l_1..l_d, p_1..p_d]) in `+` order
// and the first WhiteNoise part (add_noise! src/compose_covar.jl:63-71).  Any d >= 1 and any
// number of parts, as the reference.
struct KParams {
  int d;          // input dimension
  int nse;        // number of stationary parts (>= 1)
  int has_noise;  // a WhiteNoise part is present
  double eps;                    // jitter per stationary part on a same-object diagonal
  double noise2;                 // sigma_n^2
  double noise_sigma;            // sigma_n
  double sigma[KMAXP];           // sigma of the first KMAXP parts -- of the launch's group of
                                 // parts where a launcher narrows the description (kparams_group)
  // device tables of ALL parts in this call's slot of the context's parameter block, filled in
  // stream order by make_kparams: valid for launches on the context's streams until
  // KParBlock::NSLOT further descriptions have been made on the context
  const double* l;               // [nse][d] inverse length-scales (multipliers)
  const double* l2;              // [nse][d] their squares (the gradient pass's distance)
  const double* sig;             // [nse]    sigma of every stationary part
  const double* pf;              // [nse]    profile code (KPROF_*, as a double) of every part
  const double* exptab;          // device table 2^(j/256), j < 256 (ctx->dexptab)
  // the caller's description (host; valid during the C call): sigma of any part via kp_sigma
  const int* kinds;
  int nk;
  const double* hp;
  // profiles, by value (wave-uniform kernel arguments): prof[] follows sigma[] (the first KMAXP
  // parts, or the launch's group); mix = some part of this description (of the group, where
  // narrowed) is not SquaredExp -- selects the kernels' MIX instantiations, SE-only
  // descriptions launch the SE instantiations
  int prof[KMAXP];
  int mix;
  // Periodic parts (appended: descriptions without one pass the fields above unchanged).  A
  // Periodic part is the SquaredExp profile on the 2d embedded features
  // [l_k cos(2 pi x_k / p_k) | l_k sin(2 pi x_k / p_k)]; in a description that has one every
  // part's scaled points are de = 2d wide (SquaredExp / Matern parts: l_k x_k, then d zeros).
  int dx;             // the input dimension, also in a feature view (below), whose d is de
  int de;             // feature width of dxs / dxps / the Gram operands: 2d with a Periodic part, else d
  int nper;           // number of Periodic parts
  const double* per;  // [nse]    1.0 for a Periodic part, else 0.0 (null when nper == 0)
  const double* pk;   // [nse][d] periods p_k (1.0 for the other parts; null when nper == 0)
  // Product terms (appended: descriptions without a GPR_MUL marker pass the fields above
  // unchanged, with prod = 0 and every part closing a term of its own).  A kernel is a sum of
  // terms, a term the product of 1..KMAXP consecutive stationary parts (its factors).
  int prod;           // some term of this description (of the group, where narrowed) has > 1 factor
  int tendm;          // bit p: part p of sigma[] / prof[] (the launch's group) closes its term
  const double* tend; // [nse]    1.0 where the part closes its term, else 0.0
};

// The description as the K-assembly kernels take it: they read kp.d features per scaled point,
// so their launchers get d = de.  (They read neither l nor l2.)  Without a Periodic part this
// is kp itself.
inline KParams kparams_features(const KParams& kp) {
  KParams f = kp;
  f.d = kp.de;
  return f;
}

// sigma / profile of stationary part p (host side, any p < nse)
inline double kp_sigma(const KParams& kp, int p, int* prof = nullptr) {
  int off = 0, se = 0;
  for (int i = 0; i < kp.nk; ++i) {
    if (kind_stationary(kp.kinds[i])) {
      if (se++ == p) {
        if (prof) *prof = kind_profile(kp.kinds[i]);
        return kp.hp[off];
      }
    }
    off += kind_hp_width(kp.kinds[i], kp.dx);
  }
  if (prof) *prof = KPROF_SE;
  return 0.0;
}
// the first entry that is not SquaredExp / WhiteNoise (its kind: Matern, Periodic or a product
// marker), or 0: the
// calls that rely on SE's separability or its closed-form integrals refuse such a description
// (GPR_E_UNSUP)
inline int kinds_first_non_se(const int* kinds, int nk, int* index) {
  for (int i = 0; i < nk; ++i)
    if (kinds[i] == GPR_M32 || kinds[i] == GPR_M52 || kinds[i] == GPR_PER || kinds[i] == GPR_MUL) {
      if (index) *index = i;
      return kinds[i];
    }
  return 0;
}

// does stationary part p close its term (host side: no GPR_MUL marker follows it)?
inline bool kp_closes(const KParams& kp, int p) {
  int se = 0;
  for (int i = 0; i < kp.nk; ++i)
    if (kind_stationary(kp.kinds[i]) && se++ == p)
      return !(i + 1 < kp.nk && kp.kinds[i + 1] == GPR_MUL);
  return true;
}
// The parts of the launch group that starts at part p0 (the first part of a term): whole terms
// while they fit in KMAXP parts, so that a term never straddles two launches.  Without a marker
// every term is one part and this is min(KMAXP, nse - p0).
inline int kparams_group_count(const KParams& kp, int p0) {
  int cnt = 0;
  while (p0 + cnt < kp.nse) {
    int len = 1;
    while (!kp_closes(kp, p0 + cnt + len - 1)) ++len;
    if (cnt + len > KMAXP) break;
    cnt += len;
  }
  return cnt;
}

// The description narrowed to stationary parts [p0, p0 + cnt) (cnt <= KMAXP, whole terms:
// kparams_group_count) for one launch of the fused kernels: sigma[], prof[], the term mask and
// the device tables start at part p0 (a profile follows its part); mix and prod are the group's
// own; has_noise as given.
inline KParams kparams_group(const KParams& kp, int p0, int cnt, int has_noise) {
  KParams g = kp;
  g.nse = cnt;
  g.has_noise = has_noise;
  g.mix = 0;
  g.prod = 0;
  g.tendm = 0;
  for (int p = 0; p < KMAXP; ++p) {
    g.prof[p] = KPROF_SE;
    g.sigma[p] = p < cnt ? kp_sigma(kp, p0 + p, &g.prof[p]) : 0.0;
    if (g.prof[p] != KPROF_SE) g.mix = 1;
    if (p >= cnt || kp_closes(kp, p0 + p)) g.tendm |= 1 << p;
    else g.prod = 1;
  }
  g.tend = kp.tend + p0;
  g.l = kp.l + (size_t)p0 * kp.dx;
  g.l2 = kp.l2 + (size_t)p0 * kp.dx;
  g.sig = kp.sig + p0;
  g.pf = kp.pf + p0;
  if (kp.per) {
    g.per = kp.per + p0;
    g.pk = kp.pk + (size_t)p0 * kp.dx;
  }
  return g;
}

// Per-context parameter block: NSLOT device slots of `cap` doubles ([l | l2 | sigma | profile]
// of one kernel description each; the profile codes are part of the block, so that the
// comparison with the description made last tells SquaredExp from Matern at equal hp; with a
// Periodic part [is periodic | p] follow, see make_kparams; last the term table [closes its term],
// which tells SE + PER from SE * PER at equal hp) and as many pinned host staging slots.  make_kparams fills host
// slot `next`, uploads it in stream order and records ev[next] -- unless the tables equal those
// of the description made last, whose slot then serves again; a slot is re-filled only once
// its previous upload has completed (NSLOT descriptions later: the wait does not block in
// practice, and no host synchronisation is added to a call).  `cap` starts at the largest
// description of the old fixed-size envelope (4 parts x 64 dimensions) and grows on demand.
struct KParBlock {
  static constexpr int NSLOT = 8;
  double* dev = nullptr;
  double* host = nullptr;
  size_t cap = 0;  // doubles per slot
  int next = 0;
  hipEvent_t ev[NSLOT] = {};
  int last = -1;           // slot of the description made last (its host copy is compared), or -1
  size_t last_need = 0;    // its length in doubles
  int last_nper = 0;       // its number of Periodic parts (the two block layouts can be equally long)
  int last_nse = 0, last_d = 0;  // its stationary parts and input dimension (the same)
  std::vector<double> tmp; // the description being made
};

// A device workspace of the context: grown by ensure_buf, freed by release_buf and by nothing
// else.  Every one is listed in kWorkspaces (gpr_ctx.hip), which gpr_ctx_destroy walks.
struct DevBuf {
  double* p = nullptr;
  size_t cap = 0;  // doubles
  // (reads as the pointer it replaced -- but not through varargs: pass b.p to a "%p")
  operator double*() const { return p; }
};

// The context's device info words (gpr_ctx::dinfo, ints)
enum {
  INFO_WORD = 0,     // pivot / timeout info of a factorisation or solve (info_clear, info_read)
  INFO_POTRS = 4,    // potrs_core's sweep counters: fwd ticket/done, bwd ticket/done
  INFO_POTRS_N = 4,
  INFO_SKINNY = 8,   // the skinny sweeps of append.hip and remove.hip: ticket / blocks done
  INFO_SKINNY_N = 2,
  INFO_N = 16
};

// TC_GEMM_PIPE is kernel-level (every launch of the pipelined 2-WG/CU GEMM, whatever its call
// site), recorded in addition to the call-site class.
enum TimingClass {
  TC_KBUILD = 0, TC_SYRK = 1, TC_PANEL = 2, TC_TRSM_GEMM = 3, TC_OTHER = 4, TC_GEMM_PIPE = 5,
  TC_DAG = 6, TC_DAG_SOLVE = 7, TC_PGRAD_MEAN = 8, TC_PGRAD_VAR = 9, TC_PGRAD_SOLVE = 10,
  TC_APPEND_SOLVE = 11, TC_REMOVE_UPDATE = 12, TC_CV_GRAM = 13, TC_CV_SOLVE = 14,
  TC_LOO_SMALL = 15, TC_LOO_SYRK = 16, TC_N = 17
};

struct TimedLaunch {
  int cls;
  hipEvent_t a, b;
  double flops;
};

struct gpr_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  int nb = 128;   // inner panel width (diag blocks, in-place panel GEMMs)
  int nb2 = 1024;  // outer panel width = K of the big trailing updates (multiple of nb)
  hipStream_t ls = nullptr;       // stream the launch helpers enqueue on (default: stream)
  hipStream_t stream2 = nullptr;  // lookahead panel stream (GEMMs of the panel chain)
  hipStream_t srhs = nullptr;     // right-hand-side solves fused into the factorisation
  hipStream_t ssq = nullptr;      // square inverses of finished outer panels (fused solves)
  // gpr_fit_predict: 0 = factor, then solve (default); 1 / 2 = solve inside the factorisation
  // on its own stream / on the main stream (GPR_FUSED_RHS; measured slower at C3: 347 vs 334 ms)
  int fused_rhs = -1;             // gpr_fit_predict: -1 auto (fused, mode 2, when the tile-DAG
                                  // factors or n <= fused_rhs_nmax), 0 off, 1/2 forced
                                  // (GPR_FUSED_RHS)
  int fused_rhs_nmax = 16384;
  int fuse_y = 1;                 // gpr_fit: z = U^{-T} y inside the factorisation, then the
                                  // backward sweep alone (GPR_FUSE_Y=0: both sweeps after it;
                                  // C5's fit on one GPU: 727 -> 714 ms per job)
  int fuse_kinv = -1;             // gpr_fit_kinv (GPR_FUSE_KINV; -1 auto = 2): Z = U^{-T} solved
                                  // inside the factorisation (1), and K^{-1} = Z^T Z too (2) --
                                  // tile-DAG right-hand-side and gram tasks, or the blocked
                                  // factorisation's lookahead bubbles
  // persistent tile-DAG factorisation (dag.hip): 0 off (GPR_DAG=0: the blocked two-stream
  // factorisation), 1 on; the task list is cached per (tiles, rhs tiles).
  // Measured (POTRF alone, blocked -> DAG): N = 8192 9.3 -> 6.8 ms, 16384 34.5 -> 25.0,
  // 32768 193 -> 173.4 (67.7 TF/s); C3 fit + predict in one DAG launch 321.8 -> 305.5 ms.
  int dag_mode = 1;
  long long dag_spin_limit = 1ll << 25;  // DAG dependency wait bound in polls (~4 s); test
                                        // builds let GPR_DAG_SPIN_LIMIT override it per launch
  int dag_zlag = 4;       // lower-triangular right-hand-side rows scheduled after A's row i + lag (GPR_DAG_ZLAG)
  // plain launches' ticket order (dag.hip dag_task_order): rows taken dag_rgroup at a time
  // (GPR_DAG_RGROUP: 1 row order, 2, 4) from row dag_rgroup_min on (GPR_DAG_RGROUP_MIN), a
  // group's tasks merged by column with member r dag_rskew column slots behind member r - 1
  // (GPR_DAG_RSKEW), so the readers of a column panel run close together
  // Measured (C3 job, one box, alternating): group 1 292.0-294.2 ms per step, 2 289.8, 4 284.3-
  // 285.5, 8 289.9-290.1 (tried, not kept); every skew > 0 slower than skew 0; gmin 0 = 32.
  int dag_rgroup = 4, dag_rskew = 0, dag_rgroup_min = 32;
  int dag_order_built[4] = {-1, -1, -1, -1};  // (zlag, rgroup, rskew, rgroup_min) of dag_tasks
  // one-shot hook of the next whole-matrix factorisation launch (kglob 0, not a solve), called
  // right after the kernel is enqueued with an event that completes once the launch's progress
  // counters are reset (null if it could not be made): work ordered behind that event runs
  // BESIDE the launch (mgpu.hip streams finished tile rows of U out to the other GPUs); cleared
  // before the call
  // (colprog: the progress counters; ustored[i] = 1 once the diagonal tile U_ii is stored --
  // the launch raises colprog before that store)
  void (*dag_hook)(void* user, const double* dA, int n, int lda, const int* colprog,
                   const int* ustored, int nt, hipEvent_t counters_reset) = nullptr;
  void* dag_hook_user = nullptr;
  int dag_reserve_cu = 0;  // CUs the persistent grid leaves free for such concurrent work
  // set by a hook that left work polling dag_sync on another stream: the next DAG launch on
  // this context waits for it before resetting (or reallocating) the counters
  hipEvent_t dag_sync_readers = nullptr;
  bool dag_sync_readers_pending = false;
  int dag_gram = 1;       // K^{-1} += Z^T Z as gram tile tasks of the DAG launch (GPR_DAG_GRAM)
  int dag_solve = -1;     // solves from a finished factor as solve-only DAG launches (GPR_DAG_SOLVE; -1 auto)
  int dag_tail = 12288;  // blocked factorisations (GPR_DAG=0, ineligible sizes) hand their last
                         // <= dag_tail columns to the DAG (GPR_DAG_TAIL; 0 = off)
  unsigned* dag_tasks = nullptr;
  int dag_ntasks = 0, dag_nt = -1, dag_ntr = -1, dag_flags = -1;
  int* dag_sync = nullptr;
  size_t dag_sync_cap = 0;
  DevBuf dpadA, dpadB;  // padded copies for shapes the DAG launch does not take directly
  // rocSOLVER (dlopen'd, gpr_integrate_noise's eigendecomposition): a rocBLAS handle on this
  // context's stream, created on first use; rb_destroy releases it
  void* rb_handle = nullptr;
  int (*rb_destroy)(void*) = nullptr;
  int ncu = 0;
  std::vector<hipEvent_t> sync_events;
  size_t ev_next = 0;

  // cached inverses of the diagonal blocks of the last factor: winv[b] = U_bb^{-1}
  // (nb x nb, column-major, strictly-lower part zero), one slot per block.
  DevBuf winv;
  FactorCache fc;  // which factor winv / dsqinv belong to, and the upper-only assembly's claim

  int* dinfo = nullptr;         // device info words (INFO_*)
  double* dexptab = nullptr;    // 2^(j/256), j < 256, correctly rounded (assembly exp)
  DevBuf dscratch;              // generic scratch (partials, small vectors)
  // child contexts that run cross-validation folds concurrently (gpr_cv_batch)
  static constexpr int CV_MAX_SUB = 8;
  struct gpr_ctx* cv_sub[CV_MAX_SUB] = {};
  int cv_streams = 4;  // GPR_CV_STREAMS
  DevBuf dbig, dbig2;           // large scratch (Z for potri, Kpx for predict, ...)
  DevBuf dsqinv;                // U_sq^{-1} of every outer panel square (nb2^2 per slot)
  DevBuf dpanel;                // out-of-place result of the panel's rest GEMM
  DevBuf dtrsv;                 // single-launch triangular sweep hand-off vector (n x 2)
  DevBuf dahand;                // the append's skinny solve: hand-off blocks (128 x 16 per block)
  DevBuf drmw;                  // gpr_fit_remove: a group's W rows (8 x n'), then keep[] and idx[]
  DevBuf dxs;                   // per-part scaled training inputs  (nse x d x n)
  DevBuf dxps;                  // per-part scaled second inputs    (nse x d x m)
  DevBuf dscr_wt;                // gpr_fit_predict: K^{-1} y when the caller passes no alpha
  DevBuf dpanel_rhs;             // solved outer panel of the fused right-hand sides
  DevBuf dgA;                   // Gram-assembly row operands (MFMA lane order, assembly.hip)
  DevBuf dgB;                   // Gram-assembly column operands
  DevBuf dgc;                   // Gram-assembly centres (nse x d)
  // upper-only K assembly for a factorisation (assembly.hip kmat_symu_kernel): its work list
  // (strip << 16 | segment, built once per n); the matrix it last left without its strict
  // lower off-diagonal tiles is fc's kup claim -- the next potrf_core on exactly that matrix has
  // the tile-DAG write them (DAG_MIRROR), or mirrors them first on any other path
  struct KupList {
    long long key = -1;  // 2 n + full
    int nitems = 0;
    int* d = nullptr;
    unsigned long long used = 0;
  };
  KupList kup[4];
  unsigned long long kup_clock = 0;
  DevBuf dagb;                  // batched tile-DAG workspace (W slots, task lists, counters)
  DevBuf deig;                  // eigensolver workspace (eigen.hip, tridiag.hip)
  DevBuf ddc;                   // divide-and-conquer workspace (dstedc.hip)
  // its merge tables' pinned host staging buffer, re-filled only after dc_tab_ev (the previous
  // call's upload) has completed
  int* dc_tab_host = nullptr;
  size_t dc_tab_host_cap = 0;
  hipEvent_t dc_tab_ev = nullptr;
  DevBuf dtri;                  // the tridiagonal T between the two stages
  int kbuild_upper = 1;         // GPR_KBUILD_UPPER=0: fits build the full K (mirrored tiles)
  int kbuild_exact = 0;         // GPR_KBUILD_EXACT=1: the reference's difference form for K
  int kbuild_gram_maxd = 1 << 30;  // GPR_KBUILD_GRAM_MAXD: largest d that takes the Gram form
                                // (20: the compile-time-S kernels only, difference form above)
  KParBlock kpar;               // kernel-description tables (make_kparams)
  int kbuild_tiles = 0;         // GPR_KBUILD_TILES=1: one SE part's symmetric K by the mirrored
                                // tiles too (A/B runs against the Matern profiles)
  int kbuild_colstore = 1;      // GPR_KBUILD_COLSTORE=0: single-part upper builds store in the
                                // MFMA D layout instead of 1-KB column segments
  int cv_batch = 1;             // GPR_CV_BATCH=0: cv_batch folds one by one on child contexts
  double cv_batch_gb = 16.0;    // GPR_CV_BATCH_GB: device-memory budget of a batched launch
  int cv_kfold_gram = -1;       // GPR_CV_KFOLD_GRAM: gpr_cv_kfold's P_FF as fold Grams of Z = U^{-T}
                                // (1), or gathered from the full K^{-1} (0); -1 auto: the Grams for
                                // folds of up to 128 points, the gather above (cvfold.hip)
  double quad_batch_gb = 16.0;  // GPR_QUAD_BATCH_GB: the same for the quadrature's columns
  int quad_eigen = -1;          // GPR_QUAD_EIGEN: sample_noise quadrature path (-1 auto)
  int quad_seq = 0;             // GPR_QUAD_SEQ=1: its per-column factorisations one at a time
  int pgrad_slab = 1024;        // GPR_PGRAD_SLAB: training points per workgroup of the posterior-
                                // gradient passes (predict_grad.hip; rounded up to a multiple of 64)
  int pgrad_solve = -1;         // GPR_PGRAD_SOLVE: Q = K^{-1} K(x, xp) of the variance gradient by
                                // potrs_core's sweeps (0), by Z = U^{-T} and two MFMA products (1),
                                // -1 auto (predict_grad.hip)
  int append_sweep = -1;        // GPR_APPEND_SWEEP: V = U^{-T} K(x, x_new) of gpr_fit_append by the
                                // single-launch skinny sweep (1, m <= 128), by trsm_ut_core (0),
                                // -1 auto (append.hip)
  int remove_sweep = -1;        // GPR_REMOVE_SWEEP: the rank-r update of gpr_fit_remove as one persistent
                                // launch per group of 8 removed points (1), as one diagonal and one
                                // panel launch per 128-row block (0), -1 auto = 0 (remove.hip)

  bool timing = false;
  std::vector<TimedLaunch> pending;
  std::vector<hipEvent_t> event_pool;
  double t_ms[TC_N] = {};
  long long t_launches[TC_N] = {};
  double t_flops[TC_N] = {};
};

// ---- error helpers -------------------------------------------------------------------
// split prediction of sorted, disjoint row pieces [pieces[2k], pieces[2k+1]) (predict.hip)
int split_predict_pieces(gpr_ctx* ctx, const int* kinds, int nk, const double* hp, int d,
                         const double* dX, int ns, const double* dU, int ldu, const double* dwt,
                         const double* dXe, int ne, const double* dXq, int nq, const int* pieces,
                         int npieces, int var_lo, int var_hi, double eps, double* dmu, int ldmu,
                         double* dvar, bool compact);
int set_err(gpr_ctx* ctx, int code, const char* fmt, ...);
// the knob values of `from` onto `to` (child contexts follow their parent)
void copy_knobs(const gpr_ctx* from, gpr_ctx* to);

#define HIP_TRY(ctx, expr)                                                          \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess)                                                           \
      return set_err(ctx, GPR_E_HIP, "%s failed: %s (%s:%d)", #expr,                \
                     hipGetErrorString(_e), __FILE__, __LINE__);                    \
  } while (0)

#define GPR_TRY(expr)            \
  do {                           \
    int _r = (expr);             \
    if (_r != 0) return _r;      \
  } while (0)

#define LAUNCH_CHECK(ctx) HIP_TRY(ctx, hipGetLastError())

// the calls built on SquaredExp's separability or its closed-form integrals: GPR_E_UNSUP,
// naming the part, before anything is computed or written
inline int refuse_non_se(gpr_ctx* ctx, const int* kinds, int nk, const char* what) {
  int idx = 0;
  const int kind = kinds ? kinds_first_non_se(kinds, nk, &idx) : 0;
  if (!kind) return 0;
  return set_err(ctx, GPR_E_UNSUP, "%s needs SquaredExp parts: part %d is %s", what, idx + 1,
                 kind_name(kind));
}

// ---- workspace ------------------------------------------------------------------------
int ensure_buf(gpr_ctx* ctx, DevBuf& b, size_t need_doubles);
// the one place a workspace is freed: synchronise, free, zero, and drop every cache of ctx->fc
// whose key points into the freed range
// (synced: the caller has synchronised the stream already -- several buffers in a row, one wait)
int release_buf(gpr_ctx* ctx, DevBuf& b, bool synced = false);
int ensure_winv(gpr_ctx* ctx, int n, int nb);
// ---- info word ------------------------------------------------------------------------
// clear INFO_WORD in stream order; copy it back and synchronise the stream
int info_clear(gpr_ctx* ctx, hipStream_t st);
int info_read(gpr_ctx* ctx, hipStream_t st, int* hinfo);

// ---- timing ---------------------------------------------------------------------------
struct TimerScope {
  gpr_ctx* ctx;
  TimedLaunch tl;
  bool on;
  hipStream_t st;
  TimerScope(gpr_ctx* c, int cls, double flops);
  ~TimerScope();
};

// ---- parse a kernel description -------------------------------------------------------
int make_kparams(gpr_ctx* ctx, const int* kinds, int nk, const double* hp, int d,
                 double eps, KParams* kp, int* D_total);

// ---- cross-TU launchers ---------------------------------------------------------------
// C[m,n] = alpha * sum_{k<K} P[k + m*ldp] * Q[k + n*ldq] (* qscale[k]) + beta * C[m,n]
struct GemmArgs {
  const double* P; int ldp;
  const double* Q; int ldq;
  double* C; int ldc;
  int M, N, K;
  double alpha, beta;
  int upper;              // grid over upper tiles only (M == N) + element mask m <= n
  int mask_upper;         // element mask m <= n + mask_off on a general grid
  int mask_off;           // column offset of C relative to its row origin (mask_upper)
  int kfrom_n;            // tile's K loop starts at its n0 (triangular factor, Z^T Z)
  int kend_from_m;        // tile's K loop ends at min(K, m0+TM) (upper-triangular P:
                          // P[t][m] = 0 for t > m, e.g. P = U^{-1}); 2: at min(K, m0), the
                          // rows above the diagonal tile only (its stages go to a tri_p launch)
  const double* qscale;   // optional per-k scale of Q (diag(wt) C)
  const double* E; int lde;  // optional Hadamard factor: C = beta*C + alpha*acc*E
  double* norm_out;       // optional: norm_out[n] -= sum_m (result)^2 (needs M <= tile)
  const int* info;        // optional: skip when *info != 0
  int occ1;               // launch at one workgroup per CU (lookahead co-residence)
  // P is a factor BUFFER (upper triangle U, anything -- K, NaN -- below it): elements k > m
  // are replaced by zero as the diagonal tile's K-stages are staged (a select, never a
  // product).  Needs kend_from_m; default off.  (sample.hip: S = mu 1^T + U^T Z)
  int tri_p;
  int kfrom_m;            // with tri_p: the K loop starts at the tile's m0 (diagonal tile only)
  const double* mu;       // with tri_p: optional, C[m, n] += mu[m] after alpha / beta
};
int launch_gemm_tn(gpr_ctx* ctx, const GemmArgs& g, int timing_class);

int launch_kernel_matrix(gpr_ctx* ctx, const KParams& kp, const double* dX, int n,
                         const double* dXp, int m, int same, double* dK, int ldk);
// K for a factorisation that follows at once (potrf_core on exactly dK): where the tile-DAG
// takes the matrix directly, only what the factorisation reads is assembled -- the upper
// triangle and the whole 128 x 128 diagonal blocks, column-contiguously -- and the DAG writes
// the strict lower off-diagonal tiles from the tiles it loads (DAG_MIRROR); anything else
// gets the full symmetric K.  The buffer ends as the reference's: upper U, strict lower K.
int launch_kernel_matrix_for_factor(gpr_ctx* ctx, const KParams& kp, const double* dX, int n,
                                    double* dK, int ldk);
int launch_mirror_upper(gpr_ctx* ctx, double* A, int n, int lda);
int launch_scale_inputs(gpr_ctx* ctx, const KParams& kp, const double* dX, int n, double* out);
// ctx->dxs <- per part and point [cos(2 pi x_k / p_k) | sin(2 pi x_k / p_k)] (2d wide, without
// l_k) for the Periodic parts of kp (the other parts' rows are not for use); the MLL gradient's
// per-point table
int launch_embed_unit(gpr_ctx* ctx, const KParams& kp, const double* dX, int n);
// the same into *buf (grown to nse x 2d x n doubles): the posterior gradient's training and test points
int launch_embed_unit_to(gpr_ctx* ctx, const KParams& kp, const double* dX, int n, DevBuf& buf);
int launch_pair(gpr_ctx* ctx, int mode, int d, const double* xa, int na, const double* xb, int nb,
                double s2, double* out, size_t sa, size_t sb);
int launch_set_identity(gpr_ctx* ctx, double* A, int n, int lda);
// Right-hand sides solved during the factorisation: B <- U^{-T} B (outer panel s of B is
// solved as soon as panel s of U is final, on ctx->srhs beside the trailing updates).
// lower_rhs: B is lower triangular (identity), outer block s touches columns < (s+1) nb2.
struct RhsSpec {
  double* B;
  int nrhs;
  int ldb;
  int lower_rhs;
  int mode;  // 1: own stream (srhs) beside the trailing updates; 2: main stream after each SYRK
  // optional: gram (ldg) = B^T B -- K^{-1} = Z^T Z when B is the identity: gram tile tasks
  // of the tile-DAG launch (all of it), or accumulated panel by panel by the blocked path
  // (X_s^T X_s of each solved panel, upper; potrf_core zeroes it first; the caller mirrors)
  double* gram;
  int ldg;
  // results, written by potrf_core
  bool solved = false;     // B was solved (else dropped by the block sizes: the caller solves it)
  bool gram_full = false;  // gram was written in full (the tile-DAG; else the caller mirrors)
};
// one-launch tile-DAG factorisation (+ B <- U^{-T} B); 1 = shape not eligible, 0 = launched
// DAG_GRAM (with DAG_LOWER, B = the identity's Z = U^{-T}): also G = Z^T Z (every tile)
// DAG_MIRROR: A holds only its upper triangle and 128 x 128 diagonal blocks (the upper-only
// K assembly): every off-diagonal task also stores its loaded tile A_ij, transposed, into the
// strict lower tile (j, i)
enum { DAG_SOLVE = 1, DAG_LOWER = 2, DAG_GRAM = 4, DAG_MIRROR = 8 };
int launch_potrf_dag(gpr_ctx* ctx, double* dA, int n, int lda, double* dB, int nrhs, int ldb,
                     int kglob, hipStream_t st, int flags = 0, double* dG = nullptr, int ldg = 0);
// true when potrf_core would factor (n, lda, dA) as ONE tile-DAG launch (directly, or for
// other shapes on a padded copy); dag_shape_ok: the launch takes the shape directly
bool dag_takes_whole(const gpr_ctx* ctx, int n, int lda, const double* dA);
bool dag_shape_ok(int n, int lda, const double* dA);
int launch_potrf_dag_batch(gpr_ctx* ctx, double* dA, size_t strA, int n, int lda, double* dB,
                           size_t strB, int nrhs, int ldb, int nbatch, int* info_out);
int launch_potrf_dag_padded(gpr_ctx* ctx, double* dA, int n, int lda, double* dB, int nrhs,
                            int ldb);
int potrf_core(gpr_ctx* ctx, double* dA, int n, int lda, int* info, RhsSpec* spec = nullptr);
// the upper-triangle product C = beta C + alpha P^T P (P: K x n, ld ldp) as launch_gemm_tn takes it
inline GemmArgs syrk_upper_args(const double* P, int ldp, double* C, int ldc, int n, int K,
                                double alpha, double beta) {
  GemmArgs g{};
  g.P = P; g.ldp = ldp;
  g.Q = P; g.ldq = ldp;
  g.C = C; g.ldc = ldc;
  g.M = n; g.N = n; g.K = K;
  g.alpha = alpha; g.beta = beta;
  g.upper = 1;
  return g;
}
// dst (ld n) <- the n x nrhs columns of src (ld lds), device to device on ctx->stream
int copy_columns(gpr_ctx* ctx, double* dst, int n, const double* src, int lds, int nrhs);
int ensure_factor_inverses(gpr_ctx* ctx, const double* dU, int n, int ldu);
// the diagonal-block kernels on their own (potrf.hip): factor the block at kglob of A in place
// (inverse into winv; a failing pivot: kglob + its order in ctx->dinfo), and ctx->winv's slots
// from block b0 on recomputed from the factor
int diag_factor_block(gpr_ctx* ctx, double* A, int lda, int n, int kglob, double* winv);
int diag_inverse_blocks(gpr_ctx* ctx, const double* dU, int ldu, int n, int b0);
int trsm_ut_core(gpr_ctx* ctx, const double* dU, int n, int ldu, double* dB, int nrhs,
                 int ldb, double* norm_out, int lower_rhs);
int kinv_from_z(gpr_ctx* ctx, const double* Z, int n, double* dKinv, int ldk);
// cvfold.hip: K = U^T U into dK (ldk), Z = U^{-T} (ld n), alpha = K^{-1} y and, where P is not
// null, P = K^{-1} in full (ld n), in gpr_fit_kinv's order of calls; *hinfo > 0: not positive definite
int fit_z_alpha(gpr_ctx* ctx, const KParams& kp, const double* dX, int n, const double* dy,
                double* K, int ldk, double* Z, double* dalpha, double* P, int* hinfo);
// mll.hip: the host part of gpr_mll_grad -- grad[D] (host) = -0.5 sum_ab (a_a a_b - M_ab) dK_i,ab
// from one fused pass over the upper 64 x 64 tiles of M (n x n, ldm; a diagonal tile is read in
// full), in hp order, G .*= hp with log_scale.  gpr_mll_grad: M = K^{-1}, a = alpha; gpr_loo_grad:
// a = 0 and its weight matrix.  Synchronises.
int weighted_dk_sums(gpr_ctx* ctx, const KParams& kp, int D, const int* kinds, int nk,
                     const double* hp, int d, const double* dX, int n, const double* dM, int ldm,
                     const double* da, int log_scale, double* grad);
// symmetric eigendecomposition A = P diag(lam) P^T applied to B: lam (n, device) and
// B <- P^T B (n x m, ld ldb), A read only; *sweeps may be null.  method 0: tridiagonal
// reduction + divide and conquer (tridiag.hip, dstedc.hip) where n fits them, else block
// Jacobi (eigen.hip); 2: block Jacobi, whose floor >= 0 asks for the eigenvalues of A + floor I
// to high relative accuracy (what (lam + s)^-1 needs for every s >= floor; 0 = those of A)
int sym_eig_apply(gpr_ctx* ctx, const double* dA, int n, int lda, double* dB, int m, int ldb,
                  double* dlam, int* sweeps, double floor, int method);
// dstedc.hip: T = tridiag(e, d, e) = Z diag(lam) Z^T, C <- Z^T C; n <= 6144 (tridiag_eig_ok)
int tridiag_eig_apply(gpr_ctx* ctx, const double* dd, const double* de, int n, double* dC, int m,
                      int ldc, double* dlam);
bool tridiag_eig_ok(int n);
// tridiag.hip: A = Q T Q^T (d, e on the device; B <- Q^T B when m > 0), one persistent launch
// (+ blocked WY back-transform for m > 1024); n <= 6144 (sym_tridiag_ok).  Workspace ctx->deig.
int sym_tridiag(gpr_ctx* ctx, const double* dA, int n, int lda, double* dB, int m, int ldb,
                double* dd, double* de);
bool sym_tridiag_ok(int n);
// the quadrature's columns from T: out[2j] = C[:, j]' (T + s_j I)^{-1} c, out[2j+1] = k2 - c' (T +
// s_j I)^{-1} c with c = C[:, ny]; scr: 4 n quad_tridiag_chunk(n, ny) doubles
int quad_tridiag_chunk(int n, int ny);
int quad_tridiag_solves(gpr_ctx* ctx, const double* dd, const double* de, int n, const double* C,
                        int ldc, int ny, const double* dnoise, double k2, double* scr, double* out);
// norm[j] -= ||B[:, j]||^2 (one wave per column, deterministic), on ctx->stream
int launch_colnorm_sub(gpr_ctx* ctx, const double* dB, int ldb, int n, int ncols, double* norm);
// forward = false: only the backward sweep U x = B (B already holds U^{-T} b);
// backward = false: only the forward sweep U^T z = B
int potrs_core(gpr_ctx* ctx, const double* dU, int n, int ldu, double* dB, int nrhs, int ldb,
               bool forward = true, bool backward = true);
