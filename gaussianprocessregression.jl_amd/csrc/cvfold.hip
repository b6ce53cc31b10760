// gpr_cv_kfold: k-fold and leave-one-out cross-validation from ONE factorisation.
//
// For a fold that tests the points F and trains on ALL the others, with K the GPR_SELF matrix of
// all n points (eps per stationary part + the first WhiteNoise's sigma_n^2), P = K^{-1} and
// alpha = K^{-1} y:
//   Sigma_p = (P_FF)^{-1}            the full posterior covariance predict! forms
//   y_F - yp = (P_FF)^{-1} alpha_F   the residual
// (Sigma_p is the Schur complement of K_TT in K, and the reference's predict! builds exactly
// those blocks: eps + noise on the test points, the plain cross kernel between test and
// training points).  With K = U^T U and Z = U^{-T} (lower triangular), P_FF = Z[:, F]^T Z[:, F],
// so one factorisation with Z as a lower-triangular right-hand side serves every fold.
//
// Route 1 (GPR_CV_KFOLD_GRAM = 1; the auto rule's choice for folds of up to 128 points):
// G_f = Z[:, F]^T Z[:, F] by a gathered-column Gram kernel on FP64 MFMA (cf_gram_kernel: one
// workgroup per (fold, row slab), partial Grams summed in slab order by the solve -- no atomics,
// two calls agree bit for bit), then one workgroup per fold factors G_f in LDS (diag_block.hpp),
// r = G_f^{-1} alpha_F, diag(G_f^{-1}) and the loss.
// Route 0: P = K^{-1} in full (gpr_fit_kinv's internals) and G_f = P[F, F] gathered from it; the
// same per-fold solve.  Folds of more than 128 points: G_f by the upper SYRK of a gathered panel
// (route 1) or the gather (route 0), then potrf_core / potrs_core and the inverse by
// trsm_ut_core, fold after fold.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "diag_block.hpp"

namespace {

constexpr int CF_T = 128;           // largest fold the LDS kernels take
constexpr int CF_KR = 32;           // rows of Z per stage (the kernel's row granularity)
constexpr int CF_LDK = CF_KR + 4;   // LDS stride of a staged column (16-B aligned, 8 banks apart)
constexpr int CF_THREADS = 256;
constexpr int CF_QMAX = 9;          // upper 16 x 16 tiles per wave: 36 tiles of 128 x 128 over 4 waves

// ---- fold Grams ------------------------------------------------------------------------------
// Workgroup (f, s): Gp[f, s] = Z[R_s, F]^T Z[R_s, F] (T x T, ld T, upper 16 x 16 tiles; T = the
// fold size rounded up to 16, padded columns are zero) over its slab R_s of the rows
// [first[f], n), first[f] = the fold's smallest index rounded down to CF_KR: column c of Z is
// zero above row c.  What the buffer holds above the diagonal is not relied on (the launch that
// made Z wrote the identity's zeros there and the lower tiles only, but a diagonal tile's upper
// half is a product with W's zeros): an element with row < column is replaced by zero as it is
// staged -- a select, never a product.
// A stage is CF_KR rows of the fold's columns: 16 threads per column, 16 bytes (two rows) each
// when n is even (every column of Z is then 16-B aligned at even rows; vec = 0: 8-B loads), the
// next stage's loads in flight while the MFMAs of this one run from LDS.
__global__ __launch_bounds__(CF_THREADS) void cf_gram_kernel(
    const double* __restrict__ Z, int n, size_t ldz, const int* __restrict__ idx,
    const int* __restrict__ first, int ntst, int T, int nslab, int vec, double* __restrict__ Gp) {
  extern __shared__ __attribute__((aligned(16))) double cf_lds[];
  double* Zs = cf_lds;                                      // T x CF_LDK
  int* cols = reinterpret_cast<int*>(cf_lds + (size_t)T * CF_LDK);  // T
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int f = blockIdx.x / nslab, s = blockIdx.x - f * nslab;
  if (tid < T) cols[tid] = tid < ntst ? idx[(size_t)f * ntst + tid] : -1;
  __syncthreads();
  const int r0 = first[f];
  const int nst = (n - r0 + CF_KR - 1) / CF_KR;
  const int per = (nst + nslab - 1) / nslab;
  const int st0 = s * per, st1 = min(nst, st0 + per);
  const int nt = T / 16, ntile = nt * (nt + 1) / 2;
  const int nit = T / 16;  // 16-byte items per thread and stage
  // this wave's tiles: t = wv + 4 q, upper tiles in column order
  int ti[CF_QMAX], tj[CF_QMAX];
  d4v acc[CF_QMAX];
#pragma unroll
  for (int q = 0; q < CF_QMAX; ++q) {
    const int t = min(wv + 4 * q, ntile - 1);
    int j = 0;
    while ((j + 1) * (j + 2) / 2 <= t) ++j;
    tj[q] = j;
    ti[q] = t - j * (j + 1) / 2;
    acc[q] = d4v{0.0, 0.0, 0.0, 0.0};
  }
  // this thread's items: column (tid >> 4) + 16 e, rows 2 (tid & 15) + {0, 1} of the stage
  const int pr = 2 * (tid & 15);
  d2v pre[CF_T / 16];
  auto fetch = [&](int st) {
    const int row = r0 + st * CF_KR + pr;
#pragma unroll
    for (int e = 0; e < CF_T / 16; ++e) {
      d2v v = {0.0, 0.0};
      if (e < nit) {
        const int c = cols[(tid >> 4) + 16 * e];
        // (rows above the column's diagonal, beyond n, and padded columns: nothing is loaded)
        const bool in0 = c >= 0 && row >= c && row < n;
        const bool in1 = c >= 0 && row + 1 >= c && row + 1 < n;
        const double* src = Z + (size_t)max(c, 0) * ldz;
        if (vec) {
          if (in1) {  // (n even and row even: row + 1 < n whenever row < n)
            v = *reinterpret_cast<const d2v*>(src + row);
            if (!in0) v[0] = 0.0;
          }
        } else {
          if (in0) v[0] = src[row];
          if (in1) v[1] = src[row + 1];
        }
      }
      pre[e] = v;
    }
  };
  if (st0 < st1) fetch(st0);
  for (int st = st0; st < st1; ++st) {
    __syncthreads();  // the previous stage's MFMA operands are read
#pragma unroll
    for (int e = 0; e < CF_T / 16; ++e)
      if (e < nit)
        *reinterpret_cast<d2v*>(Zs + (size_t)((tid >> 4) + 16 * e) * CF_LDK + pr) = pre[e];
    __syncthreads();
    if (st + 1 < st1) fetch(st + 1);
#pragma unroll
    for (int q = 0; q < CF_QMAX; ++q) {
      if (wv + 4 * q < ntile) {  // (wave-uniform)
        const double* pa = Zs + (size_t)(16 * ti[q] + (lane & 15)) * CF_LDK + (lane >> 4);
        const double* pb = Zs + (size_t)(16 * tj[q] + (lane & 15)) * CF_LDK + (lane >> 4);
#pragma unroll
        for (int kk = 0; kk < CF_KR / 4; ++kk)
          acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[4 * kk], pb[4 * kk], acc[q], 0, 0, 0);
      }
    }
  }
  double* G = Gp + (size_t)blockIdx.x * T * T;
#pragma unroll
  for (int q = 0; q < CF_QMAX; ++q) {
    if (wv + 4 * q < ntile) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        G[(size_t)(16 * ti[q] + (lane >> 4) + 4 * r) + (size_t)(16 * tj[q] + (lane & 15)) * T] =
            acc[q][r];
    }
  }
}

// route 0: Gp[f] (one slab) = P[F, F] from the full P = K^{-1} (n x n, ld ldp), zero-padded to T
__global__ void cf_gather_p_kernel(const double* __restrict__ P, size_t ldp,
                                   const int* __restrict__ idx, int ntst, int T,
                                   double* __restrict__ Gp) {
  const int f = blockIdx.x;
  const int* F = idx + (size_t)f * ntst;
  double* G = Gp + (size_t)f * T * T;
  for (int e = threadIdx.x; e < T * T; e += blockDim.x) {
    const int r = e % T, c = e / T;
    G[e] = (r < ntst && c < ntst) ? P[(size_t)F[r] + (size_t)F[c] * ldp] : 0.0;
  }
}

// ---- per-fold solve, folds of up to 128 points ---------------------------------------------
// One workgroup per fold (a grid-stride loop over the folds; W slot per workgroup): G_f = the
// sum of its nslab partial Grams in slab order, padded with the identity, factored in LDS
// (diag2_core: G_f = U_f^T U_f, W = U_f^{-1} to the workgroup's slot), then with a = alpha_F
//   t = W^T a,  r = W t = G_f^{-1} a,  v_i = sum_j W_ij^2 = (G_f^{-1})_ii = (Sigma_p)_ii
//   MSE = sum r_i^2 / |F|,  ChiSq = sum r_i^2 / v_i,  Mahalanobis = a^T G_f^{-1} a = sum t_j^2
// every sum sequential in index order.  A fold whose factorisation fails leaves finfo[f] > 0.
constexpr int CF_VEC = D2_LDS_DOUBLES;  // a | t | r | v, 128 doubles each, behind the factor's LDS
constexpr size_t CF_SOLVE_LDS = sizeof(double) * (CF_VEC + 4 * CF_T);

__global__ __launch_bounds__(DIAG_THREADS) void cf_solve_kernel(
    const double* __restrict__ Gp, int T, int nslab, const int* __restrict__ idx, int ntst,
    int nfold, const double* __restrict__ alpha, const double* __restrict__ y, int cost,
    double* __restrict__ Wws, double* __restrict__ lss, double* __restrict__ mu,
    double* __restrict__ var, int* __restrict__ finfo) {
  extern __shared__ double dsm[];
  lds_d* S = (lds_d*)dsm;
  lds_d(*Xd)[D2_PB] = reinterpret_cast<lds_d(*)[D2_PB]>(S + D2_PK);
  lds_i* fail = reinterpret_cast<lds_i*>(S + D2_PK + 4 * D2_PB);
  lds_d* va = S + CF_VEC;
  lds_d* vt = va + CF_T;
  lds_d* vr = vt + CF_T;
  lds_d* vv = vr + CF_T;
  const int tid = threadIdx.x;
  double* W = Wws + (size_t)blockIdx.x * CF_T * CF_T;
  for (int f = blockIdx.x; f < nfold; f += gridDim.x) {
    __syncthreads();  // the previous fold's vectors are read
    const int* F = idx + (size_t)f * ntst;
    const double* G = Gp + (size_t)f * nslab * T * T;
    for (int e = tid; e < CF_T * CF_T; e += DIAG_THREADS) {
      const int r = e & (CF_T - 1), c = e >> 7;
      if (r > c) continue;
      double g = r == c ? 1.0 : 0.0;
      if (c < ntst) {
        g = 0.0;
        for (int s = 0; s < nslab; ++s) g += G[(size_t)s * T * T + r + (size_t)c * T];
      }
      S[pk(r, c)] = g;
    }
    if (tid < CF_T) va[tid] = tid < ntst ? alpha[F[tid]] : 0.0;
    __syncthreads();
    const int bad = diag2_core<false>(S, Xd, fail, nullptr, 0, ntst, 0, W);
    if (bad) {  // (uniform)
      if (tid == 0) finfo[f] = bad;
      continue;
    }
    // W back from the workgroup's slot (its own stores: release, barrier, acquire), packed upper
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    for (int e = tid; e < CF_T * CF_T; e += DIAG_THREADS) {
      const int r = e & (CF_T - 1), c = e >> 7;
      if (r <= c) S[pk(r, c)] = W[e];
    }
    __syncthreads();
    if (tid < CF_T) {
      double t = 0.0;
      for (int i = 0; i <= tid; ++i) t = fma(S[pk(i, tid)], va[i], t);
      vt[tid] = t;
    }
    __syncthreads();
    if (tid < CF_T) {
      double r = 0.0;
      for (int j = tid; j < ntst; ++j) r = fma(S[pk(tid, j)], vt[j], r);
      vr[tid] = r;
    } else {
      const int i = tid - CF_T;
      double v = 0.0;
      for (int j = i; j < ntst; ++j) {
        const double w = S[pk(i, j)];
        v = fma(w, w, v);
      }
      vv[i] = v;
    }
    __syncthreads();
    if (tid == 0) {
      double l = 0.0;
      for (int i = 0; i < ntst; ++i) {
        if (cost == GPR_COST_MSE) l += vr[i] * vr[i];
        else if (cost == GPR_COST_CHISQ) l += vr[i] * vr[i] / vv[i];
        else l += vt[i] * vt[i];
      }
      lss[f] = cost == GPR_COST_MSE ? l / ntst : l;
    }
    if (tid < ntst) {
      mu[(size_t)f * ntst + tid] = y[F[tid]] - vr[tid];
      var[(size_t)f * ntst + tid] = vv[tid];
    }
  }
}

// ---- folds of more than 128 points ----------------------------------------------------------
// panel (n x ntst, ld n) <- the fold's columns of Z, zero above each column's diagonal
__global__ void cf_panel_kernel(const double* __restrict__ Z, int n, size_t ldz,
                                const int* __restrict__ F, int ntst, double* __restrict__ panel) {
  const size_t tot = (size_t)n * ntst;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot;
       e += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(e % n), j = (int)(e / n);
    const int c = F[j];
    panel[e] = r >= c ? Z[(size_t)c * ldz + r] : 0.0;
  }
}

// G (ntst x ntst, ld ntst) <- P[F, F]
__global__ void cf_gather_big_kernel(const double* __restrict__ P, size_t ldp,
                                     const int* __restrict__ F, int ntst, double* __restrict__ G) {
  const size_t tot = (size_t)ntst * ntst;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot;
       e += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(e % ntst), c = (int)(e / ntst);
    G[e] = P[(size_t)F[r] + (size_t)F[c] * ldp];
  }
}

// a[j] = src[F[j]]
__global__ void cf_gather_vec_kernel(const double* __restrict__ src, const int* __restrict__ F,
                                     int ntst, double* __restrict__ a) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < ntst; j += gridDim.x * blockDim.x)
    a[j] = src[F[j]];
}

__global__ void cf_zero_kernel(double* __restrict__ a, int m) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x)
    a[j] = 0.0;
}

// the fold's loss and predictions from a = alpha_F, r = G_f^{-1} a and nv = -diag(G_f^{-1})
// (nv is read only where it was formed: ChiSq, or with_var); one thread sums in index order
__global__ void cf_finish_kernel(const double* __restrict__ a, const double* __restrict__ r,
                                 const double* __restrict__ nv, const double* __restrict__ y,
                                 const int* __restrict__ F, int ntst, int cost, int with_var,
                                 double* __restrict__ lss, double* __restrict__ mu,
                                 double* __restrict__ var) {
  for (int j = threadIdx.x; j < ntst; j += blockDim.x) {
    mu[j] = y[F[j]] - r[j];
    var[j] = with_var ? -nv[j] : 0.0;
  }
  if (threadIdx.x == 0) {
    double l = 0.0;
    for (int i = 0; i < ntst; ++i) {
      if (cost == GPR_COST_MSE) l += r[i] * r[i];
      else if (cost == GPR_COST_CHISQ) l += r[i] * r[i] / -nv[i];
      else l += a[i] * r[i];
    }
    *lss = cost == GPR_COST_MSE ? l / ntst : l;
  }
}

int blocks_for(size_t items) { return (int)std::min<size_t>((items + 255) / 256, 4096); }

// row slabs per fold: enough workgroups to fill the chip with few folds (a fixed target, so the
// cut -- and with it every bit of the result -- depends on the shape alone), at least two stages
// per slab
int cf_slabs(int n, int nfold) {
  const int nst = (n + CF_KR - 1) / CF_KR;
  const int want = (1024 + nfold - 1) / nfold;
  return std::max(1, std::min(want, nst / 2));
}

}  // namespace

// K = U^T U into dK (n x n, ldk: upper U, strict lower K, as gpr_fit), Z = U^{-T} (n x n, ld n,
// lower triangular: what lies above its diagonal is not to be relied on), alpha = K^{-1} y, and,
// where P is given, P = K^{-1} in full (n x n, ld n) -- gpr_fit_kinv's order of calls.  The front
// half of gpr_cv_kfold and the whole of gpr_fit_loo.  *hinfo > 0: K is not positive definite.
int fit_z_alpha(gpr_ctx* ctx, const KParams& kp, const double* dX, int n, const double* dy,
                double* K, int ldk, double* Z, double* dalpha, double* P, int* hinfo) {
  GPR_TRY(launch_kernel_matrix_for_factor(ctx, kp, dX, n, K, ldk));
  GPR_TRY(launch_set_identity(ctx, Z, n, n));
  GPR_TRY(copy_columns(ctx, dalpha, n, dy, n, 1));
  RhsSpec rhs{Z, n, n, 1, ctx->fused_rhs == 2 ? 2 : 1, nullptr, 0};
  const int fuse = ctx->fuse_kinv >= 0 ? ctx->fuse_kinv : 2;
  if (P && fuse == 2) {
    rhs.gram = P;
    rhs.ldg = n;
  }
  *hinfo = 0;
  GPR_TRY(potrf_core(ctx, K, n, ldk, hinfo, &rhs));
  if (*hinfo != 0) return 0;
  const bool solved = rhs.solved;
  GPR_TRY(potrs_core(ctx, K, n, ldk, dalpha, 1, n));
  if (!solved) GPR_TRY(trsm_ut_core(ctx, K, n, ldk, Z, n, n, nullptr, 1));
  if (P) {
    if (solved && rhs.gram) {
      if (!rhs.gram_full) GPR_TRY(launch_mirror_upper(ctx, P, n, n));
    } else {
      GPR_TRY(kinv_from_z(ctx, Z, n, P, n));
    }
  }
  return 0;
}

extern "C" int gpr_cv_kfold(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                            const double* dX, int n, const double* dy, const int* tst, int ntst,
                            int nfold, int cost, double eps, double* lss, double* mu,
                            double* var) {
  if (!ctx) return GPR_E_ARG;
  if (!kinds) return set_err(ctx, GPR_E_ARG, "gpr_cv_kfold: kinds is NULL");
  if (!hp) return set_err(ctx, GPR_E_ARG, "gpr_cv_kfold: hp is NULL");
  if (!dX) return set_err(ctx, GPR_E_ARG, "gpr_cv_kfold: dX is NULL");
  if (!dy) return set_err(ctx, GPR_E_ARG, "gpr_cv_kfold: dy is NULL");
  if (!tst) return set_err(ctx, GPR_E_ARG, "gpr_cv_kfold: tst is NULL");
  if (!lss) return set_err(ctx, GPR_E_ARG, "gpr_cv_kfold: lss is NULL");
  if (n < 2) return set_err(ctx, GPR_E_ARG, "gpr_cv_kfold: n = %d (at least 2)", n);
  if (ntst < 1 || ntst >= n)
    return set_err(ctx, GPR_E_ARG, "gpr_cv_kfold: ntst = %d (1 <= ntst < n = %d)", ntst, n);
  if (nfold < 1) return set_err(ctx, GPR_E_ARG, "gpr_cv_kfold: nfold = %d (at least 1)", nfold);
  if (cost != GPR_COST_MSE && cost != GPR_COST_CHISQ && cost != GPR_COST_MAHALANOBIS)
    return set_err(ctx, GPR_E_ARG, "gpr_cv_kfold: unknown cost %d", cost);
  std::vector<int> hfirst(nfold);
  {
    std::vector<int> seen(n, -1);
    for (int f = 0; f < nfold; ++f) {
      int lo = n;
      for (int j = 0; j < ntst; ++j) {
        const int i = tst[(size_t)f * ntst + j];
        if (i < 0 || i >= n)
          return set_err(ctx, GPR_E_ARG, "gpr_cv_kfold: tst[%d][%d] = %d out of range (n = %d)", f,
                         j, i, n);
        if (seen[i] == f)
          return set_err(ctx, GPR_E_ARG, "gpr_cv_kfold: tst[%d] holds index %d twice", f, i);
        seen[i] = f;
        lo = std::min(lo, i);
      }
      hfirst[f] = lo / CF_KR * CF_KR;
    }
  }
  KParams kp;
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, eps, &kp, nullptr));
  hipStream_t st = ctx->stream;
  const bool small = ntst <= CF_T;
  // auto: the fold Grams where the LDS kernels take the fold; above, one SYRK per fold over a
  // gathered panel fills few tiles and measured slower than K^{-1} once and a gather per fold
  // (n = 8192, 10 folds of 819: 27.0 vs 20.1 ms)
  const bool gram_route = ctx->cv_kfold_gram < 0 ? small : ctx->cv_kfold_gram != 0;
  const bool want_var = var != nullptr || cost == GPR_COST_CHISQ;
  const size_t nn = (size_t)n * n, nout = (size_t)nfold * ntst;

  // ---- workspace: Z in dbig; everything else in dbig2 (no call below touches either) ----------
  const int T = (ntst + 15) / 16 * 16;
  int nslab = 1, nfc = nfold, nwg = 0;
  size_t szfold = 0;  // doubles of per-fold scratch
  if (small) {
    const size_t budget = (size_t)1 << 25;  // 256 MB of partial Grams per chunk of folds
    const int nfc0 = (int)std::min<size_t>((size_t)nfold, std::max<size_t>(1, budget / ((size_t)T * T)));
    nslab = gram_route ? cf_slabs(n, nfc0) : 1;
    nfc = (int)std::min<size_t>((size_t)nfold, std::max<size_t>(1, budget / ((size_t)nslab * T * T)));
    nwg = std::min(nfc, 512);
    szfold = (size_t)nfc * nslab * T * T + (size_t)nwg * CF_T * CF_T;
  } else {
    // panel (route 1) | G | W2 | a | r | nv
    szfold = (gram_route ? (size_t)n * ntst : 0) + 2 * (size_t)ntst * ntst + 3 * (size_t)ntst;
  }
  const size_t szd = nn + (gram_route ? 0 : nn) + n + nfold + 2 * nout + szfold;
  const size_t nints = nout + 2 * (size_t)nfold;
  GPR_TRY(ensure_buf(ctx, ctx->dbig, nn));
  GPR_TRY(ensure_buf(ctx, ctx->dbig2, szd + (nints + 1) / 2 + 2));
  double* Z = ctx->dbig;
  double* K = ctx->dbig2;
  double* P = gram_route ? nullptr : K + nn;
  double* dalpha = K + nn + (gram_route ? 0 : nn);
  double* dlss = dalpha + n;
  double* dmu = dlss + nfold;
  double* dvar = dmu + nout;
  double* fold_ws = dvar + nout;
  int* didx = reinterpret_cast<int*>(fold_ws + szfold);
  int* dfirst = didx + nout;
  int* dfinfo = dfirst + nfold;

  // ---- one factorisation: K = U^T U, Z = U^{-T}, alpha = K^{-1} y (gpr_fit_kinv's order) -----
  int hinfo = 0;
  GPR_TRY(fit_z_alpha(ctx, kp, dX, n, dy, K, n, Z, dalpha, P, &hinfo));
  if (hinfo != 0) return hinfo;

  HIP_TRY(ctx, hipMemcpyAsync(didx, tst, nout * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dfirst, hfirst.data(), (size_t)nfold * sizeof(int),
                              hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(dfinfo, 0, (size_t)nfold * sizeof(int), st));

  int rc = 0;
  if (small) {
    double* Gp = fold_ws;
    double* Wws = Gp + (size_t)nfc * nslab * T * T;
    for (int f0 = 0; f0 < nfold; f0 += nfc) {
      const int nb = std::min(nfc, nfold - f0);
      const int* cidx = didx + (size_t)f0 * ntst;
      if (gram_route) {
        TimerScope ts(ctx, TC_CV_GRAM, 2.0 * T * T * (double)n * nb);
        const size_t lds = sizeof(double) * (size_t)T * CF_LDK + sizeof(int) * (size_t)T;
        cf_gram_kernel<<<nb * nslab, CF_THREADS, lds, st>>>(Z, n, (size_t)n, cidx, dfirst + f0,
                                                            ntst, T, nslab, n % 2 == 0, Gp);
        LAUNCH_CHECK(ctx);
      } else {
        TimerScope ts(ctx, TC_CV_GRAM, 0.0);
        cf_gather_p_kernel<<<nb, 256, 0, st>>>(P, (size_t)n, cidx, ntst, T, Gp);
        LAUNCH_CHECK(ctx);
      }
      {
        TimerScope ts(ctx, TC_CV_SOLVE, 0.0);
        cf_solve_kernel<<<std::min(nb, nwg), DIAG_THREADS, CF_SOLVE_LDS, st>>>(
            Gp, T, nslab, cidx, ntst, nb, dalpha, dy, cost, Wws, dlss + f0,
            dmu + (size_t)f0 * ntst, dvar + (size_t)f0 * ntst, dfinfo + f0);
        LAUNCH_CHECK(ctx);
      }
    }
  } else {
    double* panel = fold_ws;
    double* G = panel + (gram_route ? (size_t)n * ntst : 0);
    double* W2 = G + (size_t)ntst * ntst;
    double* va = W2 + (size_t)ntst * ntst;
    double* vr = va + ntst;
    double* nv = vr + ntst;
    for (int f = 0; f < nfold && !rc; ++f) {
      const int* F = didx + (size_t)f * ntst;
      if (gram_route) {
        {
          TimerScope ts(ctx, TC_CV_GRAM, 0.0);
          cf_panel_kernel<<<blocks_for((size_t)n * ntst), 256, 0, st>>>(Z, n, (size_t)n, F, ntst,
                                                                       panel);
          LAUNCH_CHECK(ctx);
        }
        GPR_TRY(launch_gemm_tn(ctx, syrk_upper_args(panel, n, G, ntst, ntst, n, 1.0, 0.0),
                               TC_CV_GRAM));
      } else {
        TimerScope ts(ctx, TC_CV_GRAM, 0.0);
        cf_gather_big_kernel<<<blocks_for((size_t)ntst * ntst), 256, 0, st>>>(P, (size_t)n, F, ntst,
                                                                             G);
        LAUNCH_CHECK(ctx);
      }
      cf_gather_vec_kernel<<<blocks_for(ntst), 256, 0, st>>>(dalpha, F, ntst, va);
      LAUNCH_CHECK(ctx);
      HIP_TRY(ctx, hipMemcpyAsync(vr, va, sizeof(double) * ntst, hipMemcpyDeviceToDevice, st));
      int finfo = 0;
      if ((rc = potrf_core(ctx, G, ntst, ntst, &finfo))) break;
      if (finfo != 0) {
        rc = finfo;
        break;
      }
      if ((rc = potrs_core(ctx, G, ntst, ntst, vr, 1, ntst))) break;
      if (want_var) {
        // diag(G^{-1})_i = ||column i of U_f^{-T}||^2 (the inverse route of gpr_potri_upper)
        if ((rc = launch_set_identity(ctx, W2, ntst, ntst))) break;
        if ((rc = trsm_ut_core(ctx, G, ntst, ntst, W2, ntst, ntst, nullptr, 1))) break;
        cf_zero_kernel<<<blocks_for(ntst), 256, 0, st>>>(nv, ntst);
        if ((rc = launch_colnorm_sub(ctx, W2, ntst, ntst, ntst, nv))) break;
      }
      cf_finish_kernel<<<1, 256, 0, st>>>(va, vr, nv, dy, F, ntst, cost, want_var ? 1 : 0,
                                          dlss + f, dmu + (size_t)f * ntst,
                                          dvar + (size_t)f * ntst);
      if (hipGetLastError() != hipSuccess) rc = set_err(ctx, GPR_E_HIP, "gpr_cv_kfold: launch failed");
    }
    // the caches describe the last fold's G, which lives in scratch the next call overwrites
    ctx->fc.factor_forget();
    if (rc) return rc;
  }
  // the fitted K sits in workspace too: no later call may take its inverses for a hit
  ctx->fc.factor_forget();

  std::vector<int> hfinfo(nfold);
  std::vector<double> hl(nfold), hmu(mu ? nout : 0), hvar(var ? nout : 0);
  HIP_TRY(ctx, hipMemcpyAsync(hfinfo.data(), dfinfo, (size_t)nfold * sizeof(int),
                              hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(hl.data(), dlss, (size_t)nfold * sizeof(double),
                              hipMemcpyDeviceToHost, st));
  if (mu)
    HIP_TRY(ctx, hipMemcpyAsync(hmu.data(), dmu, nout * sizeof(double), hipMemcpyDeviceToHost, st));
  if (var)
    HIP_TRY(ctx, hipMemcpyAsync(hvar.data(), dvar, nout * sizeof(double), hipMemcpyDeviceToHost,
                                st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (int f = 0; f < nfold; ++f)
    if (hfinfo[f] > 0) return hfinfo[f];
  std::copy(hl.begin(), hl.end(), lss);
  if (mu) std::copy(hmu.begin(), hmu.end(), mu);
  if (var) std::copy(hvar.begin(), hvar.end(), var);
  return 0;
}
