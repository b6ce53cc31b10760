// Context, memory, error and timing plumbing of libgpr_hip.so.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>

#include "common.hpp"

int set_err(gpr_ctx* ctx, int code, const char* fmt, ...) {
  if (ctx) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    ctx->err = buf;
  }
  return code;
}

int release_buf(gpr_ctx* ctx, DevBuf& b, bool synced) {
  if (!b.p) return 0;
  // (a stream that cannot be synchronised may still be using the buffer: it is kept, and the
  // error returned, as ensure_buf's regrow always did)
  if (!synced) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipFree(b.p));
  ctx->fc.release_range(b.p, b.cap);
  b = DevBuf{};
  return 0;
}

int ensure_buf(gpr_ctx* ctx, DevBuf& b, size_t need) {
  if (b.cap >= need && b.p) return 0;
  GPR_TRY(release_buf(ctx, b));
  if (need == 0) need = 1;
  if (hipMalloc((void**)&b.p, need * sizeof(double)) != hipSuccess) {
    b.p = nullptr;
    return set_err(ctx, GPR_E_NOMEM, "hipMalloc of %zu bytes failed", need * sizeof(double));
  }
  b.cap = need;
  return 0;
}

int ensure_winv(gpr_ctx* ctx, int n, int nb) {
  size_t nblk = (size_t)((n + nb - 1) / nb);
  return ensure_buf(ctx, ctx->winv, nblk * nb * nb);
}

int info_clear(gpr_ctx* ctx, hipStream_t st) {
  HIP_TRY(ctx, hipMemsetAsync(ctx->dinfo + INFO_WORD, 0, sizeof(int), st));
  return 0;
}

int info_read(gpr_ctx* ctx, hipStream_t st, int* hinfo) {
  HIP_TRY(ctx, hipMemcpyAsync(hinfo, ctx->dinfo + INFO_WORD, sizeof(int), hipMemcpyDeviceToHost,
                              st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return 0;
}

int copy_columns(gpr_ctx* ctx, double* dst, int n, const double* src, int lds, int nrhs) {
  HIP_TRY(ctx, hipMemcpy2DAsync(dst, (size_t)n * sizeof(double), src, (size_t)lds * sizeof(double),
                                (size_t)n * sizeof(double), nrhs, hipMemcpyDeviceToDevice,
                                ctx->stream));
  return 0;
}

// ---- timing ----------------------------------------------------------------------------
static hipEvent_t get_event(gpr_ctx* ctx) {
  if (!ctx->event_pool.empty()) {
    hipEvent_t e = ctx->event_pool.back();
    ctx->event_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}

TimerScope::TimerScope(gpr_ctx* c, int cls, double flops) : ctx(c), on(c->timing) {
  if (!on) return;
  st = ctx->ls ? ctx->ls : ctx->stream;
  tl.cls = cls;
  tl.flops = flops;
  tl.a = get_event(ctx);
  tl.b = get_event(ctx);
  hipEventRecord(tl.a, st);
}

TimerScope::~TimerScope() {
  if (!on) return;
  hipEventRecord(tl.b, st);
  ctx->pending.push_back(tl);
}

static void drain_timing(gpr_ctx* ctx) {
  if (ctx->pending.empty()) return;
  hipStreamSynchronize(ctx->stream);
  for (auto& t : ctx->pending) {
    float ms = 0;
    hipEventElapsedTime(&ms, t.a, t.b);
    ctx->t_ms[t.cls] += ms;
    ctx->t_launches[t.cls] += 1;
    ctx->t_flops[t.cls] += t.flops;
    ctx->event_pool.push_back(t.a);
    ctx->event_pool.push_back(t.b);
  }
  ctx->pending.clear();
}

// ---- kernel description ------------------------------------------------------------------
int make_kparams(gpr_ctx* ctx, const int* kinds, int nk, const double* hp, int d, double eps,
                 KParams* kp, int* D_total) {
  if (!kinds || nk <= 0) return set_err(ctx, GPR_E_ARG, "bad kinds/nk (%d)", nk);
  if (!hp) return set_err(ctx, GPR_E_ARG, "hp is NULL");
  if (d <= 0) return set_err(ctx, GPR_E_ARG, "d=%d (needs d >= 1)", d);
  memset(kp, 0, sizeof *kp);
  int nse = 0, nper = 0, nfac = 0;  // nfac: factors of the term being read
  for (int i = 0, off = 0; i < nk; ++i) {
    if (kinds[i] == GPR_MUL) {  // an infix marker: a stationary part on either side
      if (i == 0 || i == nk - 1)
        return set_err(ctx, GPR_E_ARG, "kinds[%d]: a product marker (GPR_MUL) is %s of the "
                                       "description", i, i == 0 ? "the first entry" : "the last entry");
      if (kinds[i - 1] == GPR_MUL)
        return set_err(ctx, GPR_E_ARG, "kinds[%d]: two product markers (GPR_MUL) in a row", i);
      if (kinds[i - 1] == GPR_WN || kinds[i + 1] == GPR_WN)
        return set_err(ctx, GPR_E_ARG, "kinds[%d]: a product marker (GPR_MUL) next to WhiteNoise "
                                       "(kinds[%d]); products take stationary factors only", i,
                       kinds[i - 1] == GPR_WN ? i - 1 : i + 1);
      continue;
    }
    if (kind_stationary(kinds[i])) {
      ++nse;
      nfac = (i > 0 && kinds[i - 1] == GPR_MUL) ? nfac + 1 : 1;
      if (nfac > KMAXP)
        return set_err(ctx, GPR_E_UNSUP, "kinds[%d]: factor %d of a product term (at most %d "
                                         "factors per term)", i, nfac, KMAXP);
    }
    else if (kinds[i] != GPR_WN) return set_err(ctx, GPR_E_ARG, "unknown kernel kind %d", kinds[i]);
    if (kinds[i] == GPR_PER) {  // (before anything is computed or written)
      ++nper;
      for (int k = 0; k < d; ++k) {
        const double p = hp[off + 1 + d + k];
        if (!(std::fabs(p) > 0.0) || std::isinf(p))
          return set_err(ctx, GPR_E_ARG, "part %d (Periodic): period p_%d = %g of dimension %d is "
                                         "zero or not finite", i + 1, k + 1, p, k + 1);
      }
    }
    off += kind_hp_width(kinds[i], d);
  }
  if (nse == 0)
    return set_err(ctx, GPR_E_ARG, "kernel needs at least one stationary part (SquaredExp, "
                                   "Matern32, Matern52 or Periodic)");
  // this description's slot of the parameter block:
  // [l (nse d) | l2 (nse d) | sigma (nse) | profile (nse)], then with a Periodic part
  // [is periodic (nse) | p (nse d)] -- a longer block, so that it never compares equal to one
  // without, and two Periodic parts that differ only in p differ in the block; last the term
  // table [closes its term (nse)]: 1.0 unless a product marker follows the part
  KParBlock& kb = ctx->kpar;
  const size_t nl = (size_t)nse * d;
  const size_t ntab = 2 * nl + 2 * (size_t)nse + (nper ? nl + (size_t)nse : 0);  // before tend
  const size_t need = ntab + (size_t)nse;
  if (need > kb.cap || !kb.dev) {
    // (first use, or a description past every earlier one: never inside the 4 x 64 envelope
    // once the block exists)
    const size_t cap = std::max(need, (size_t)(2 * 4 * 64 + 3 * 4));
    if (kb.dev) {
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      HIP_TRY(ctx, hipFree(kb.dev));
      HIP_TRY(ctx, hipHostFree(kb.host));
      kb.dev = kb.host = nullptr;
      kb.cap = 0;
    }
    const size_t bytes = KParBlock::NSLOT * cap * sizeof(double);
    if (hipMalloc((void**)&kb.dev, bytes) != hipSuccess) {
      kb.dev = nullptr;
      return set_err(ctx, GPR_E_NOMEM, "hipMalloc of %zu bytes failed", bytes);
    }
    if (hipHostMalloc((void**)&kb.host, bytes, hipHostMallocDefault) != hipSuccess) {
      hipFree(kb.dev);
      kb.dev = kb.host = nullptr;
      return set_err(ctx, GPR_E_NOMEM, "hipHostMalloc of %zu bytes failed", bytes);
    }
    kb.cap = cap;
    kb.last = -1;
  }
  kb.tmp.resize(need);
  double* hl = kb.tmp.data();
  kp->exptab = ctx->dexptab;
  kp->d = kp->dx = d;
  kp->de = nper ? 2 * d : d;
  kp->nper = nper;
  kp->eps = eps;
  kp->kinds = kinds;
  kp->nk = nk;
  kp->hp = hp;
  int off = 0;
  kp->tendm = (1 << KMAXP) - 1;
  for (int i = 0; i < nk; ++i) {
    if (kinds[i] == GPR_MUL) continue;
    if (kinds[i] != GPR_WN) {
      const int prof = kind_profile(kinds[i]);
      const bool closes = !(i + 1 < nk && kinds[i + 1] == GPR_MUL);
      if (!closes) kp->prod = 1;
      hl[ntab + kp->nse] = closes ? 1.0 : 0.0;
      if (kp->nse < KMAXP) {
        kp->sigma[kp->nse] = hp[off];
        kp->prof[kp->nse] = prof;
        if (!closes) kp->tendm &= ~(1 << kp->nse);
      }
      if (prof != KPROF_SE) kp->mix = 1;
      hl[2 * nl + kp->nse] = hp[off];
      hl[2 * nl + nse + kp->nse] = (double)prof;
      for (int k = 0; k < d; ++k) {
        hl[(size_t)kp->nse * d + k] = hp[off + 1 + k];
        hl[nl + (size_t)kp->nse * d + k] = hp[off + 1 + k] * hp[off + 1 + k];
      }
      if (nper) {
        const bool per = kinds[i] == GPR_PER;
        hl[2 * nl + 2 * nse + kp->nse] = per ? 1.0 : 0.0;
        for (int k = 0; k < d; ++k)
          hl[2 * nl + 3 * (size_t)nse + (size_t)kp->nse * d + k] = per ? hp[off + 1 + d + k] : 1.0;
      }
      kp->nse++;
      off += kind_hp_width(kinds[i], d);
    } else {
      if (!kp->has_noise) {  // findfirst(WhiteNoise) -- src/compose_covar.jl:64-68
        kp->has_noise = 1;
        kp->noise_sigma = hp[off];
        kp->noise2 = hp[off] * hp[off];
      }
      off += 1;
    }
  }
  // the tables of the description made last on this context (a fit and the gradient or the
  // posterior that follows it share hp): its slot serves again, nothing is uploaded
  int slot = kb.last;
  if (slot < 0 || kb.last_need != need || kb.last_nper != nper || kb.last_nse != nse ||
      kb.last_d != d ||
      memcmp(kb.host + (size_t)slot * kb.cap, hl, need * sizeof(double)) != 0) {
    slot = kb.next;
    kb.next = (slot + 1) % KParBlock::NSLOT;
    if (!kb.ev[slot]) HIP_TRY(ctx, hipEventCreateWithFlags(&kb.ev[slot], hipEventDisableTiming));
    else HIP_TRY(ctx, hipEventSynchronize(kb.ev[slot]));  // this slot's previous upload (NSLOT ago)
    kb.last = -1;
    memcpy(kb.host + (size_t)slot * kb.cap, hl, need * sizeof(double));
    HIP_TRY(ctx, hipMemcpyAsync(kb.dev + (size_t)slot * kb.cap, kb.host + (size_t)slot * kb.cap,
                                need * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(kb.ev[slot], ctx->stream));
    kb.last = slot;
    kb.last_need = need;
    kb.last_nper = nper;
    kb.last_nse = nse;
    kb.last_d = d;
  }
  const double* dl = kb.dev + (size_t)slot * kb.cap;
  kp->l = dl;
  kp->l2 = dl + nl;
  kp->sig = dl + 2 * nl;
  kp->pf = dl + 2 * nl + nse;
  if (nper) {
    kp->per = dl + 2 * nl + 2 * nse;
    kp->pk = dl + 2 * nl + 3 * (size_t)nse;
  }
  kp->tend = dl + ntab;
  if (D_total) *D_total = off;
  return 0;
}

// ---- knobs ---------------------------------------------------------------------------------
// Every run-time switch of the library: a GPR_* environment variable read once by
// gpr_ctx_create, or gpr_set_knob on a live context.  Documented in include/gpr_hip.h; none of
// them changes a result beyond rounding (they pick between equivalent code paths or tune
// memory budgets).  Test-only fault injection exists only in libgpr_hip_testing.so
// (-DGPR_TESTING).
namespace {
struct Knob {
  const char* name;
  int gpr_ctx::*ip;     // an int field, or
  double gpr_ctx::*dp;  // a double field
};
const Knob kKnobs[] = {
    {"GPR_DAG", &gpr_ctx::dag_mode, nullptr},
    {"GPR_DAG_TAIL", &gpr_ctx::dag_tail, nullptr},
    {"GPR_DAG_SOLVE", &gpr_ctx::dag_solve, nullptr},
    {"GPR_DAG_GRAM", &gpr_ctx::dag_gram, nullptr},
    {"GPR_DAG_ZLAG", &gpr_ctx::dag_zlag, nullptr},
    {"GPR_DAG_RGROUP", &gpr_ctx::dag_rgroup, nullptr},
    {"GPR_DAG_RSKEW", &gpr_ctx::dag_rskew, nullptr},
    {"GPR_DAG_RGROUP_MIN", &gpr_ctx::dag_rgroup_min, nullptr},
    {"GPR_FUSED_RHS", &gpr_ctx::fused_rhs, nullptr},
    {"GPR_FUSE_Y", &gpr_ctx::fuse_y, nullptr},
    {"GPR_FUSE_KINV", &gpr_ctx::fuse_kinv, nullptr},
    {"GPR_KBUILD_UPPER", &gpr_ctx::kbuild_upper, nullptr},
    {"GPR_KBUILD_EXACT", &gpr_ctx::kbuild_exact, nullptr},
    {"GPR_KBUILD_COLSTORE", &gpr_ctx::kbuild_colstore, nullptr},
    {"GPR_KBUILD_TILES", &gpr_ctx::kbuild_tiles, nullptr},
    {"GPR_KBUILD_GRAM_MAXD", &gpr_ctx::kbuild_gram_maxd, nullptr},
    {"GPR_CV_STREAMS", &gpr_ctx::cv_streams, nullptr},
    {"GPR_CV_BATCH", &gpr_ctx::cv_batch, nullptr},
    {"GPR_CV_BATCH_GB", nullptr, &gpr_ctx::cv_batch_gb},
    {"GPR_CV_KFOLD_GRAM", &gpr_ctx::cv_kfold_gram, nullptr},
    {"GPR_QUAD_BATCH_GB", nullptr, &gpr_ctx::quad_batch_gb},
    {"GPR_QUAD_EIGEN", &gpr_ctx::quad_eigen, nullptr},
    {"GPR_QUAD_SEQ", &gpr_ctx::quad_seq, nullptr},
    {"GPR_PGRAD_SLAB", &gpr_ctx::pgrad_slab, nullptr},
    {"GPR_PGRAD_SOLVE", &gpr_ctx::pgrad_solve, nullptr},
    {"GPR_APPEND_SWEEP", &gpr_ctx::append_sweep, nullptr},
    {"GPR_REMOVE_SWEEP", &gpr_ctx::remove_sweep, nullptr},
};

void knob_set(gpr_ctx* ctx, const Knob& k, double v) {
  if (k.ip) {
    int iv = (int)v;
    if (k.ip == &gpr_ctx::dag_zlag) iv = std::max(0, iv);
    if (k.ip == &gpr_ctx::dag_rgroup) iv = iv < 2 ? 1 : (iv < 4 ? 2 : 4);
    if (k.ip == &gpr_ctx::dag_rskew || k.ip == &gpr_ctx::dag_rgroup_min) iv = std::max(0, iv);
    if (k.ip == &gpr_ctx::cv_streams) iv = std::max(1, std::min(iv, (int)gpr_ctx::CV_MAX_SUB));
    if (k.ip == &gpr_ctx::pgrad_slab) iv = (std::max(iv, 64) + 63) / 64 * 64;
    ctx->*k.ip = iv;
  } else {
    ctx->*k.dp = v;
  }
}

// Every device workspace of a context; gpr_ctx_destroy releases exactly these.
DevBuf gpr_ctx::*const kWorkspaces[] = {
    &gpr_ctx::winv,   &gpr_ctx::dscratch, &gpr_ctx::dbig,       &gpr_ctx::dbig2, &gpr_ctx::dsqinv,
    &gpr_ctx::dpanel, &gpr_ctx::dtrsv,    &gpr_ctx::dahand,     &gpr_ctx::drmw,  &gpr_ctx::dxs,
    &gpr_ctx::dxps,   &gpr_ctx::dscr_wt,  &gpr_ctx::dpanel_rhs, &gpr_ctx::dgA,   &gpr_ctx::dgB,
    &gpr_ctx::dgc,    &gpr_ctx::dpadA,    &gpr_ctx::dpadB,      &gpr_ctx::dagb,  &gpr_ctx::deig,
    &gpr_ctx::ddc,    &gpr_ctx::dtri,
};

const Knob* knob_find(const char* name) {
  if (!name) return nullptr;
  for (const Knob& k : kKnobs)
    if (!strcmp(k.name, name)) return &k;
  return nullptr;
}
}  // namespace

void copy_knobs(const gpr_ctx* from, gpr_ctx* to) {
  for (const Knob& k : kKnobs) {
    if (k.ip) to->*k.ip = from->*k.ip;
    else to->*k.dp = from->*k.dp;
  }
  to->dag_spin_limit = from->dag_spin_limit;
}

extern "C" {

const char* gpr_version(void) { return "gpr_hip 0.1.0 (gfx950)"; }

int gpr_ctx_create(int device, void* stream, gpr_ctx_t* out) {
  if (!out) return GPR_E_ARG;
  *out = nullptr;
  gpr_ctx* ctx = new gpr_ctx();
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess) {
    gpr_ctx_destroy(ctx);
    return GPR_E_HIP;
  }
  if (stream) {
    ctx->stream = (hipStream_t)stream;
  } else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
      ctx->stream = nullptr;
      gpr_ctx_destroy(ctx);
      return GPR_E_HIP;
    }
    ctx->own_stream = true;
  }
  ctx->ls = ctx->stream;
  // the lookahead panel stream gets the highest priority: its latency-bound chain
  // (diag factor + panel TRSM) must win CUs over the big trailing SYRK it overlaps
  int prio_lo = 0, prio_hi = 0;
  hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if (hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, prio_hi) != hipSuccess)
    ctx->stream2 = nullptr;
  if (ctx->stream2 && hipStreamCreateWithFlags(&ctx->srhs, hipStreamNonBlocking) != hipSuccess)
    ctx->srhs = nullptr;
  if (ctx->srhs && hipStreamCreateWithFlags(&ctx->ssq, hipStreamNonBlocking) != hipSuccess)
    ctx->ssq = nullptr;
  if (!ctx->ssq) {
    gpr_ctx_destroy(ctx);
    return GPR_E_HIP;
  }
  // Concurrent child contexts of cv_batch / integrate_noise: each drives its own stream, so
  // by default no more of them than the process has hardware queues (GPU_MAX_HW_QUEUES,
  // HIP's default 4); more only multiplex onto the same queues.
  if (const char* e = getenv("GPU_MAX_HW_QUEUES")) {
    const int q = atoi(e);
    if (q > 0) ctx->cv_streams = std::min(ctx->cv_streams, q);
  }
  // the documented knobs (include/gpr_hip.h), read once here; gpr_set_knob changes them
  for (const Knob& k : kKnobs)
    if (const char* e = getenv(k.name)) knob_set(ctx, k, atof(e));
  if (hipMalloc((void**)&ctx->dinfo, INFO_N * sizeof(int)) != hipSuccess) {
    ctx->dinfo = nullptr;
    gpr_ctx_destroy(ctx);
    return GPR_E_NOMEM;
  }
  {
    // 2^(j/256) in extended precision, rounded once to double (assembly kexp_neg table)
    double tab[256];
    for (int j = 0; j < 256; ++j) tab[j] = (double)exp2l((long double)j / 256.0L);
    if (hipMalloc((void**)&ctx->dexptab, sizeof tab) != hipSuccess) ctx->dexptab = nullptr;
    if (!ctx->dexptab ||
        hipMemcpy(ctx->dexptab, tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess) {
      gpr_ctx_destroy(ctx);
      return GPR_E_NOMEM;
    }
  }
  *out = ctx;
  return 0;
}

// (also of a half-built context: gpr_ctx_create's failure paths end here)
int gpr_ctx_destroy(gpr_ctx_t ctx) {
  if (!ctx) return 0;
  for (auto* sub : ctx->cv_sub) gpr_ctx_destroy(sub);
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  if (ctx->dag_sync_readers) {  // a hook's readers of dag_sync (freed below)
    hipEventSynchronize(ctx->dag_sync_readers);
    hipEventDestroy(ctx->dag_sync_readers);
  }
  drain_timing(ctx);
  for (auto e : ctx->event_pool) hipEventDestroy(e);
  for (auto e : ctx->sync_events) hipEventDestroy(e);
  if (ctx->stream2) hipStreamDestroy(ctx->stream2);
  if (ctx->srhs) hipStreamDestroy(ctx->srhs);
  if (ctx->ssq) hipStreamDestroy(ctx->ssq);
  for (auto w : kWorkspaces) (void)release_buf(ctx, ctx->*w, /*synced=*/true);
  if (ctx->dag_tasks) hipFree(ctx->dag_tasks);
  if (ctx->dag_sync) hipFree(ctx->dag_sync);
  if (ctx->rb_handle && ctx->rb_destroy) ctx->rb_destroy(ctx->rb_handle);
  if (ctx->dinfo) hipFree(ctx->dinfo);
  if (ctx->dexptab) hipFree(ctx->dexptab);
  if (ctx->kpar.dev) hipFree(ctx->kpar.dev);
  if (ctx->kpar.host) hipHostFree(ctx->kpar.host);
  for (auto e : ctx->kpar.ev)
    if (e) hipEventDestroy(e);
  for (auto& e : ctx->kup)
    if (e.d) hipFree(e.d);
  if (ctx->dc_tab_ev) hipEventDestroy(ctx->dc_tab_ev);
  if (ctx->dc_tab_host) hipHostFree(ctx->dc_tab_host);
  if (ctx->own_stream) hipStreamDestroy(ctx->stream);
  delete ctx;
  return 0;
}

const char* gpr_last_error(gpr_ctx_t ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int gpr_sync(gpr_ctx_t ctx) {
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

void* gpr_ctx_stream(gpr_ctx_t ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int gpr_malloc(gpr_ctx_t ctx, size_t bytes, void** dptr) {
  if (!dptr) return set_err(ctx, GPR_E_ARG, "dptr is NULL");
  if (hipMalloc(dptr, bytes ? bytes : 1) != hipSuccess)
    return set_err(ctx, GPR_E_NOMEM, "hipMalloc(%zu) failed", bytes);
  return 0;
}

int gpr_free(gpr_ctx_t ctx, void* dptr) {
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (dptr) HIP_TRY(ctx, hipFree(dptr));
  return 0;
}

int gpr_upload(gpr_ctx_t ctx, void* dst, const void* src, size_t bytes) {
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

int gpr_download(gpr_ctx_t ctx, void* dst, const void* src, size_t bytes) {
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

int gpr_set_block(gpr_ctx_t ctx, int nb) {
  if (nb != 64 && nb != 128) return set_err(ctx, GPR_E_ARG, "nb must be 64 or 128 (got %d)", nb);
  ctx->nb = nb;
  if (ctx->nb2 % nb) ctx->nb2 = 4 * nb;
  ctx->fc.factor_forget_blocks();
  return 0;
}

int gpr_set_outer_block(gpr_ctx_t ctx, int nb2) {
  if (nb2 < ctx->nb || nb2 % ctx->nb)
    return set_err(ctx, GPR_E_ARG, "outer block %d must be a multiple of nb=%d", nb2, ctx->nb);
  ctx->nb2 = nb2;
  return 0;
}

int gpr_set_knob(gpr_ctx_t ctx, const char* name, double value) {
  if (!ctx) return GPR_E_ARG;
  const Knob* k = knob_find(name);
  if (!k) return set_err(ctx, GPR_E_ARG, "unknown knob %s", name ? name : "(null)");
  knob_set(ctx, *k, value);
  // (the cached task list depends on GPR_DAG_ZLAG / RGROUP / RSKEW / RGROUP_MIN: the next
  // launch compares all four with the values the list was built from and rebuilds it)
  return 0;
}

int gpr_get_knob(gpr_ctx_t ctx, const char* name, double* value) {
  if (!ctx || !value) return GPR_E_ARG;
  const Knob* k = knob_find(name);
  if (!k) return set_err(ctx, GPR_E_ARG, "unknown knob %s", name ? name : "(null)");
  *value = k->ip ? (double)(ctx->*k->ip) : ctx->*k->dp;
  return 0;
}

int gpr_forget_factor(gpr_ctx_t ctx) {
  ctx->fc.factor_forget();
  return 0;
}

int gpr_timing_enable(gpr_ctx_t ctx, int on) {
  ctx->timing = on != 0;
  return 0;
}

int gpr_timing_get(gpr_ctx_t ctx, int cls, double* ms, long long* launches, double* flops) {
  if (cls < 0 || cls >= TC_N) return set_err(ctx, GPR_E_ARG, "bad timing class %d", cls);
  drain_timing(ctx);
  if (ms) *ms = ctx->t_ms[cls];
  if (launches) *launches = ctx->t_launches[cls];
  if (flops) *flops = ctx->t_flops[cls];
  return 0;
}

int gpr_timing_reset(gpr_ctx_t ctx) {
  drain_timing(ctx);
  for (int i = 0; i < TC_N; ++i) {
    ctx->t_ms[i] = 0;
    ctx->t_launches[i] = 0;
    ctx->t_flops[i] = 0;
  }
  return 0;
}

}  // extern "C"
