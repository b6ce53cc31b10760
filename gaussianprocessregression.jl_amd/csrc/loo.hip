// Leave-one-out training criteria and their hyper-parameter gradient on gfx950.
//
// With K the GPR_SELF matrix of all n points, P = K^{-1} and alpha = K^{-1} y, the leave-one-out
// prediction of point i is mu_i = y_i - alpha_i / P_ii with variance 1 / P_ii (gpr_cv_kfold with
// one-point folds), so a leave-one-out criterion is L = sum_i f(alpha_i, P_ii):
//   GPR_COST_LOGPRED      f = -0.5 log P_ii + alpha_i^2 / (2 P_ii) + 0.5 log 2 pi
//   GPR_COST_MSE          f = (alpha_i / P_ii)^2
//   GPR_COST_CHISQ        f = alpha_i^2 / P_ii        (GPR_COST_MAHALANOBIS on one point: the same)
// the last three the SUM over the n one-point folds of what gpr_cv_kfold returns.
// Gradient (Rasmussen & Williams 5.4.2), with d alpha = -P dK alpha and dP_ii = -(P dK P)_ii:
//   dL/dtheta_j = -sum_ab dK_j,ab [ 0.5 (b_a alpha_b + alpha_a b_b) + (P D P)_ab ]
//   b = P f_alpha,  D = diag(f_P),  f_alpha, f_P the partial derivatives of f per point.
// f_P <= 0 for every criterion, so with s_i = sqrt(-f_P,i) and S = diag(s) P: P D P = -S^T S, one
// SYRK.  The fused pass behind gpr_mll_grad computes -0.5 sum_ab (a_a a_b - M_ab) dK_ab; called
// with a = 0 and M = 2 S^T S - (b alpha^T + alpha b^T) it yields the gradient above for all D
// hyper-parameters of every kind of part (its WhiteNoise slot reads -M_aa, its eps handling is
// dK's own): the work is ONE n^3 product, however many hyper-parameters there are.
// Every sum runs in a fixed order (no atomics): two calls on the same inputs agree bit for bit.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace {

constexpr int LT = 64;  // the gradient pass's tile: it reads a diagonal LT x LT tile of M in full

// f, f_alpha and f_P of one point
__device__ __forceinline__ void loo_point(int crit, double a, double p, double* f, double* fa,
                                          double* fp) {
  if (crit == GPR_COST_LOGPRED) {
    *f = -0.5 * log(p) + a * a / (2.0 * p) + 0.9189385332046727418;  // 0.5 log 2 pi
    *fa = a / p;
    *fp = -0.5 / p - a * a / (2.0 * p * p);
  } else if (crit == GPR_COST_MSE) {
    const double r = a / p;
    *f = r * r;
    *fa = 2.0 * r / p;
    *fp = -2.0 * r * r / p;
  } else {  // ChiSq; Mahalanobis on a single point
    *f = a * a / p;
    *fa = 2.0 * a / p;
    *fp = -(a * a) / (p * p);
  }
}

// pd[i] = P_ii = sum_{k >= i} Z[k, i]^2, the column norms of Z = U^{-T} (lower triangular; what
// the buffer holds above the diagonal is never read): one wave per column, lanes over the rows
// from i on, fixed order
__global__ __launch_bounds__(256) void loo_zdiag_kernel(const double* __restrict__ Z, size_t ldz,
                                                        int n, double* __restrict__ pd) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const double* col = Z + (size_t)i * ldz;
  double s0 = 0.0, s1 = 0.0;
  int k = i + lane;
  for (; k + 64 < n; k += 128) {
    s0 = fma(col[k], col[k], s0);
    s1 = fma(col[k + 64], col[k + 64], s1);
  }
  if (k < n) s0 = fma(col[k], col[k], s0);
  double s = s0 + s1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) pd[i] = s;
}

// Per point: f_alpha -> fa[i], s_i = sqrt(-f_P) -> sv[i] (both where fa is not null), and the
// value sum_i f -> out[0].  p_i = dp[i incp].  One workgroup; the 16 waves' sums added in order.
__global__ __launch_bounds__(1024) void loo_terms_kernel(int crit, const double* __restrict__ dp,
                                                         size_t incp,
                                                         const double* __restrict__ alpha, int n,
                                                         double* __restrict__ fa,
                                                         double* __restrict__ sv,
                                                         double* __restrict__ out) {
  __shared__ double red[16];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    double f, dfa, dfp;
    loo_point(crit, alpha[i], dp[(size_t)i * incp], &f, &dfa, &dfp);
    s += f;
    if (fa) {
      fa[i] = dfa;
      sv[i] = sqrt(-dfp);
    }
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += red[w];
    out[0] = t;
  }
}

// b = P v for the symmetric P stored in full (n x n, ldp): b_j = column j . v, one wave per
// column, so P is read once and contiguously
__global__ __launch_bounds__(256) void loo_symv_kernel(const double* __restrict__ P, size_t ldp,
                                                       int n, const double* __restrict__ v,
                                                       double* __restrict__ b) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;
  const double* col = P + (size_t)j * ldp;
  double s0 = 0.0, s1 = 0.0;
  int k = lane;
  for (; k + 64 < n; k += 128) {
    s0 = fma(col[k], v[k], s0);
    s1 = fma(col[k + 64], v[k + 64], s1);
  }
  if (k < n) s0 = fma(col[k], v[k], s0);
  double s = s0 + s1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) b[j] = s;
}

// S = diag(s) P (n x n, ld n) and, on the upper triangle, M = -(b_r alpha_c + alpha_r b_c)
// (n x n, ld n): a workgroup per 1024 rows of a column (blockIdx.y strides over the columns)
__global__ __launch_bounds__(256) void loo_scale_kernel(const double* __restrict__ P, size_t ldp,
                                                        int n, const double* __restrict__ sv,
                                                        double* __restrict__ S) {
  for (int c = blockIdx.y; c < n; c += gridDim.y) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = blockIdx.x * 1024 + u * 256 + threadIdx.x;
      if (r < n) S[(size_t)c * n + r] = sv[r] * P[(size_t)c * ldp + r];
    }
  }
}
__global__ __launch_bounds__(256) void loo_prefill_kernel(int n, const double* __restrict__ alpha,
                                                          const double* __restrict__ b,
                                                          double* __restrict__ M) {
  for (int c = blockIdx.y; c < n; c += gridDim.y) {
    if (blockIdx.x * 1024 > c) continue;  // (uniform: the block lies below the diagonal)
    const double ac = alpha[c], bc = b[c];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = blockIdx.x * 1024 + u * 256 + threadIdx.x;
      if (r <= c) M[(size_t)c * n + r] = -(b[r] * ac + alpha[r] * bc);
    }
  }
}

// the strict lower half of every diagonal LT x LT tile of M <- its upper half (the SYRK writes
// the upper triangle; the gradient pass reads a diagonal tile in full)
__global__ __launch_bounds__(256) void loo_mirror_diag_kernel(int n, double* __restrict__ M) {
  const int t0 = blockIdx.x * LT;
  for (int e = threadIdx.x; e < LT * LT; e += 256) {
    const int r = t0 + (e & (LT - 1)), c = t0 + e / LT;
    if (r > c && r < n) M[(size_t)c * n + r] = M[(size_t)r * n + c];
  }
}

bool crit_ok(int crit) {
  return crit == GPR_COST_MSE || crit == GPR_COST_CHISQ || crit == GPR_COST_MAHALANOBIS ||
         crit == GPR_COST_LOGPRED;
}

dim3 col_grid(int n) { return dim3((unsigned)((n + 1023) / 1024), (unsigned)std::min(n, 65535)); }

}  // namespace

extern "C" {

int gpr_fit_loo(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d, const double* dX,
                int n, const double* dy, double eps, double* dK, int ldk, double* dalpha,
                double* dpdiag, int* info) {
  if (!ctx) return GPR_E_ARG;
  if (!kinds) return set_err(ctx, GPR_E_ARG, "gpr_fit_loo: kinds is NULL");
  if (!hp) return set_err(ctx, GPR_E_ARG, "gpr_fit_loo: hp is NULL");
  if (!dX) return set_err(ctx, GPR_E_ARG, "gpr_fit_loo: dX is NULL");
  if (!dy) return set_err(ctx, GPR_E_ARG, "gpr_fit_loo: dy is NULL");
  if (!dK) return set_err(ctx, GPR_E_ARG, "gpr_fit_loo: dK is NULL");
  if (!dalpha) return set_err(ctx, GPR_E_ARG, "gpr_fit_loo: dalpha is NULL");
  if (!dpdiag) return set_err(ctx, GPR_E_ARG, "gpr_fit_loo: dpdiag is NULL");
  if (n < 1) return set_err(ctx, GPR_E_ARG, "gpr_fit_loo: n = %d (at least 1)", n);
  if (ldk < n) return set_err(ctx, GPR_E_ARG, "gpr_fit_loo: ldk = %d < n = %d", ldk, n);
  KParams kp;
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, eps, &kp, nullptr));
  GPR_TRY(ensure_buf(ctx, ctx->dbig, (size_t)n * n));
  double* Z = ctx->dbig;
  int hinfo = 0;
  GPR_TRY(fit_z_alpha(ctx, kp, dX, n, dy, dK, ldk, Z, dalpha, nullptr, &hinfo));
  if (info) *info = hinfo;
  if (hinfo != 0) return hinfo;
  {
    TimerScope ts(ctx, TC_LOO_SMALL, 0.0);
    loo_zdiag_kernel<<<(n + 3) / 4, 256, 0, ctx->stream>>>(Z, (size_t)n, n, dpdiag);
    LAUNCH_CHECK(ctx);
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

int gpr_loo(gpr_ctx_t ctx, int crit, const double* dp, int incp, const double* dalpha, int n,
            double* out) {
  if (!ctx) return GPR_E_ARG;
  if (!crit_ok(crit)) return set_err(ctx, GPR_E_ARG, "gpr_loo: unknown crit %d", crit);
  if (!dp) return set_err(ctx, GPR_E_ARG, "gpr_loo: dp is NULL");
  if (!dalpha) return set_err(ctx, GPR_E_ARG, "gpr_loo: dalpha is NULL");
  if (!out) return set_err(ctx, GPR_E_ARG, "gpr_loo: out is NULL");
  if (n < 1) return set_err(ctx, GPR_E_ARG, "gpr_loo: n = %d (at least 1)", n);
  if (incp < 1) return set_err(ctx, GPR_E_ARG, "gpr_loo: incp = %d (at least 1)", incp);
  GPR_TRY(ensure_buf(ctx, ctx->dscratch, 64));
  {
    TimerScope ts(ctx, TC_LOO_SMALL, 0.0);
    loo_terms_kernel<<<1, 1024, 0, ctx->stream>>>(crit, dp, (size_t)incp, dalpha, n, nullptr,
                                                  nullptr, ctx->dscratch);
    LAUNCH_CHECK(ctx);
  }
  double h = 0.0;
  HIP_TRY(ctx, hipMemcpyAsync(&h, ctx->dscratch, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *out = h;
  return 0;
}

int gpr_loo_grad(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                 const double* dX, int n, const double* dKinv, int ldk, const double* dalpha,
                 double eps, int crit, int log_scale, double* value, double* grad) {
  if (!ctx) return GPR_E_ARG;
  if (!kinds) return set_err(ctx, GPR_E_ARG, "gpr_loo_grad: kinds is NULL");
  if (!hp) return set_err(ctx, GPR_E_ARG, "gpr_loo_grad: hp is NULL");
  if (!dX) return set_err(ctx, GPR_E_ARG, "gpr_loo_grad: dX is NULL");
  if (!dKinv) return set_err(ctx, GPR_E_ARG, "gpr_loo_grad: dKinv is NULL");
  if (!dalpha) return set_err(ctx, GPR_E_ARG, "gpr_loo_grad: dalpha is NULL");
  if (!grad) return set_err(ctx, GPR_E_ARG, "gpr_loo_grad: grad is NULL");
  if (n < 1) return set_err(ctx, GPR_E_ARG, "gpr_loo_grad: n = %d (at least 1)", n);
  if (ldk < n) return set_err(ctx, GPR_E_ARG, "gpr_loo_grad: ldk = %d < n = %d", ldk, n);
  if (!crit_ok(crit)) return set_err(ctx, GPR_E_ARG, "gpr_loo_grad: unknown crit %d", crit);
  KParams kp;
  int D = 0;
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, eps, &kp, &D));
  hipStream_t st = ctx->stream;
  // ---- workspace: S in dbig (Z's place, free after gpr_fit_kinv); M and the vectors in dbig2 --
  const size_t nn = (size_t)n * n, nv = ((size_t)n + 1) / 2 * 2;  // (vectors 16-B aligned)
  GPR_TRY(ensure_buf(ctx, ctx->dbig, nn));
  GPR_TRY(ensure_buf(ctx, ctx->dbig2, nn + 4 * nv + 8));
  double* S = ctx->dbig;
  double* M = ctx->dbig2;
  double* fa = M + (nn + 1) / 2 * 2;
  double* sv = fa + nv;
  double* b = sv + nv;
  double* zero = b + nv;
  double* val = zero + nv;
  {
    TimerScope ts(ctx, TC_LOO_SMALL, 0.0);
    loo_terms_kernel<<<1, 1024, 0, st>>>(crit, dKinv, (size_t)ldk + 1, dalpha, n, fa, sv, val);
    loo_symv_kernel<<<(n + 3) / 4, 256, 0, st>>>(dKinv, (size_t)ldk, n, fa, b);
    loo_scale_kernel<<<col_grid(n), 256, 0, st>>>(dKinv, (size_t)ldk, n, sv, S);
    loo_prefill_kernel<<<col_grid(n), 256, 0, st>>>(n, dalpha, b, M);
    LAUNCH_CHECK(ctx);
  }
  // the one n^3 step: M <- 2 S^T S + M on the upper triangle
  GPR_TRY(launch_gemm_tn(ctx, syrk_upper_args(S, n, M, n, n, n, 2.0, 1.0), TC_LOO_SYRK));
  {
    TimerScope ts(ctx, TC_LOO_SMALL, 0.0);
    loo_mirror_diag_kernel<<<(n + LT - 1) / LT, 256, 0, st>>>(n, M);
    LAUNCH_CHECK(ctx);
  }
  HIP_TRY(ctx, hipMemsetAsync(zero, 0, (size_t)n * sizeof(double), st));
  double hval = 0.0;
  if (value) HIP_TRY(ctx, hipMemcpyAsync(&hval, val, sizeof hval, hipMemcpyDeviceToHost, st));
  std::vector<double> g(D);
  const int rc = weighted_dk_sums(ctx, kp, D, kinds, nk, hp, d, dX, n, M, n, zero, log_scale, g.data());
  if (rc != 0) {  // (the value's copy may still be in flight)
    (void)hipStreamSynchronize(st);
    return rc;
  }
  std::copy(g.begin(), g.end(), grad);
  if (value) *value = hval;
  return 0;
}

}  // extern "C"
