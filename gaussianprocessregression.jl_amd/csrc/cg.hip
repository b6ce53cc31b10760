// K^{-1} B without K: conjugate gradients on the matrix gpr_fit factors (the GPR_SELF form: eps
// per term and sigma_n^2 on the diagonal), every product K P by the matrix-free kernel
// (kmatmul.hip), so a model with more points than an n x n buffer allows still gets its weights.
//
// The nrhs columns are independent recurrences that share one product per iteration; a column
// whose residual has met the stop test is frozen (x, r, p keep their values) while the others go
// on.  K's diagonal is constant (the terms' sigma^2 products + eps each + sigma_n^2), so Jacobi
// scaling is a scalar: z = r / diag.  It is the only preconditioning.
// Per iteration, after Q = K P:
//   cg_dot_kernel     partial sums of p.q per column, one per 256-thread block (each thread a
//                     fixed stride of rows, then a fixed tree) -- stage one
//   cg_step_xr_kernel every block sums the column's partials in the same fixed tree (stage two),
//                     alpha = (r.r / diag) / p.q, x += alpha p, r -= alpha q, partials of r.r
//   cg_step_p_kernel  the same second stage for r.r, beta = r.r / (previous r.r), p = r / diag +
//                     beta p; block 0 writes the column's r.r and its frozen flag for the next
//                     iteration into the other of two scalar slots (nobody reads that slot in
//                     this launch)
// No atomics: two calls agree bit for bit.  alpha and beta never leave the device; the host reads
// the nrhs values of r.r once per iteration for the stop test ||r_c|| <= tol ||b_c||.
// At the end relres is the TRUE residual ||b - K x|| / ||b|| from one more product, not the
// recurrence's.
//
// Limits.  Memory is O(n nrhs): r, p, q (3 n nrhs doubles) beside the product's linear
// workspace.  The iteration count is governed by sqrt(cond_2(K)) -- about 0.5 sqrt(cond) ln(2 /
// tol) -- and cond_2 <= 1 + n sigma^2 / sigma_n^2: small noise means many iterations, each a full
// evaluation of K.  Reaching maxit is not an error.
//
// The remedy is a low-rank preconditioner: with rank > 0 (gpr_solve_pcg, or the knob GPR_CG_PRECOND
// for gpr_solve_cg) z = P^{-1} r with P = L L^T + delta I from a pivoted Cholesky factor of the
// noise-free kernel (pchol.hip), and the recurrence becomes
//   rho = r.z,  alpha = rho / p.q,  x += alpha p,  r -= alpha q,  z = P^{-1} r,
//   beta = rho_new / rho,  p = z + beta p.
// cg_dot_kernel and cg_step_xr_kernel serve unchanged (the slot's first scalar holds rho, the Jacobi
// factor is 1); pchol_apply leaves z and the block partials of r.z; pcg_step_p_kernel sums both
// r.z and r.r, forms beta and p and writes the next slot.  The stop test stays on r.r, the freezing
// and the two slots are the same.  With rank 0 none of this runs: the kernels above, in the order
// above.
//
// GPR_KMM_PREC = 1 (a description the FP32 product kernel takes, kmatmul_f32.hip): iterative
// refinement around the same recurrence -- x = 0, r = b; per outer step the recurrence on K~ d = r
// (products with FP32 kernel evaluation) from d = 0 to the column's threshold, x += d, r = b - K x
// by one FP64 product; an outer step that gains less than 4 x sends the rest of the call to FP64
// products.  iters counts every product of either precision; relres stays the FP64 residual.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"

namespace {

constexpr int CG_MAXB = 256;  // most partial sums (blocks) per column

// sum of the 256 threads' values by a fixed tree; every thread gets it
__device__ __forceinline__ double cg_block_sum(double v, double* red) {
  __syncthreads();  // red's previous use is over
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

// the scalars of one column, slot s of two: sc[(s * nrhs + c) * 2 + {0: r.r, 1: frozen}]; bb[c]
__host__ __device__ inline double* cg_slot(double* sc, int s, int nrhs, int c) {
  return sc + ((size_t)s * nrhs + c) * 2;
}

// grid (nblk, nrhs).  x = 0, r = b, p = b / diag; part[c][blk] = partial b.b
__global__ __launch_bounds__(256) void cg_init_kernel(const double* __restrict__ B, size_t ldb,
                                                      int n, double dinv, double* __restrict__ X,
                                                      size_t ldx, double* __restrict__ R,
                                                      double* __restrict__ P,
                                                      double* __restrict__ part) {
  __shared__ double red[256];
  const int c = blockIdx.y;
  double s = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double b = B[(size_t)c * ldb + i];
    X[(size_t)c * ldx + i] = 0.0;
    R[(size_t)c * n + i] = b;
    P[(size_t)c * n + i] = b * dinv;
    s = fma(b, b, s);
  }
  s = cg_block_sum(s, red);
  if (threadIdx.x == 0) part[(size_t)c * CG_MAXB + blockIdx.x] = s;
}

// grid nrhs.  bb[c] = b.b; slot 0: r.r = b.b, frozen when b = 0 (x = 0 is the solution)
__global__ __launch_bounds__(256) void cg_init_scalars_kernel(const double* __restrict__ part,
                                                              int nblk, int nrhs, double tol2,
                                                              double* __restrict__ sc,
                                                              double* __restrict__ bb) {
  __shared__ double red[256];
  const int c = blockIdx.x;
  const double s =
      cg_block_sum((int)threadIdx.x < nblk ? part[(size_t)c * CG_MAXB + threadIdx.x] : 0.0, red);
  if (threadIdx.x == 0) {
    bb[c] = s;
    double* o = cg_slot(sc, 0, nrhs, c);
    o[0] = s;
    o[1] = s <= tol2 * s ? 1.0 : 0.0;  // (only b = 0, or tol >= 1)
  }
}

// grid (nblk, nrhs).  part[c][blk] = partial sum_i u_i v_i (u, v: n x nrhs, ld n)
__global__ __launch_bounds__(256) void cg_dot_kernel(const double* __restrict__ U,
                                                     const double* __restrict__ V, int n,
                                                     double* __restrict__ part) {
  __shared__ double red[256];
  const int c = blockIdx.y;
  double s = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    s = fma(U[(size_t)c * n + i], V[(size_t)c * n + i], s);
  s = cg_block_sum(s, red);
  if (threadIdx.x == 0) part[(size_t)c * CG_MAXB + blockIdx.x] = s;
}

// grid (nblk, nrhs).  alpha = (r.r dinv) / p.q from pq's partials; x += alpha p, r -= alpha q;
// rr[c][blk] = partial r.r of the new r.  A frozen column is left alone.
__global__ __launch_bounds__(256) void cg_step_xr_kernel(
    const double* __restrict__ pq, int nblk, int nrhs, int slot, double* __restrict__ sc,
    double dinv, int n, const double* __restrict__ P, const double* __restrict__ Q,
    double* __restrict__ X, size_t ldx, double* __restrict__ R, double* __restrict__ rr) {
  __shared__ double red[256];
  const int c = blockIdx.y;
  const double* cur = cg_slot(sc, slot, nrhs, c);
  if (cur[1] != 0.0) return;  // (block-uniform)
  const double den =
      cg_block_sum((int)threadIdx.x < nblk ? pq[(size_t)c * CG_MAXB + threadIdx.x] : 0.0, red);
  const double alpha = (cur[0] * dinv) / den;
  double s = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const size_t k = (size_t)c * n + i;
    X[(size_t)c * ldx + i] = fma(alpha, P[k], X[(size_t)c * ldx + i]);
    const double r = fma(-alpha, Q[k], R[k]);
    R[k] = r;
    s = fma(r, r, s);
  }
  s = cg_block_sum(s, red);
  if (threadIdx.x == 0) rr[(size_t)c * CG_MAXB + blockIdx.x] = s;
}

// grid (nblk, nrhs).  beta = r.r / previous r.r; p = r dinv + beta p; block 0 fills the other
// slot: the new r.r and frozen = r.r <= tol^2 b.b.  A frozen column carries its slot over.
__global__ __launch_bounds__(256) void cg_step_p_kernel(
    const double* __restrict__ rr, int nblk, int nrhs, int slot, double* __restrict__ sc,
    const double* __restrict__ bb, double tol2, double dinv, int n, const double* __restrict__ R,
    double* __restrict__ P) {
  __shared__ double red[256];
  const int c = blockIdx.y;
  const double* cur = cg_slot(sc, slot, nrhs, c);
  double* nxt = cg_slot(sc, slot ^ 1, nrhs, c);
  if (cur[1] != 0.0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      nxt[0] = cur[0];
      nxt[1] = 1.0;
    }
    return;
  }
  const double num =
      cg_block_sum((int)threadIdx.x < nblk ? rr[(size_t)c * CG_MAXB + threadIdx.x] : 0.0, red);
  const double beta = num / cur[0];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const size_t k = (size_t)c * n + i;
    P[k] = fma(beta, P[k], R[k] * dinv);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    nxt[0] = num;
    nxt[1] = num <= tol2 * bb[c] ? 1.0 : 0.0;
  }
}

// sum of up to PCH_MAXB = 4 x 256 partials: each thread four in order, then the fixed tree
__device__ __forceinline__ double pcg_sum_rz(const double* __restrict__ rz, int nz, double* red) {
  double v = 0.0;
  for (int k = 0; k < 4; ++k) {
    const int b = 4 * (int)threadIdx.x + k;
    if (b < nz) v += rz[b];
  }
  return cg_block_sum(v, red);
}

// grid (nblk, nrhs).  p = z; block 0: the slot's r.r becomes rho = r.z (the frozen flag stays)
__global__ __launch_bounds__(256) void pcg_start_kernel(const double* __restrict__ rz, int nz,
                                                        int nrhs, double* __restrict__ sc, int n,
                                                        const double* __restrict__ Z,
                                                        double* __restrict__ P) {
  __shared__ double red[256];
  const int c = blockIdx.y;
  const double rho = pcg_sum_rz(rz + (size_t)c * PCH_MAXB, nz, red);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    P[(size_t)c * n + i] = Z[(size_t)c * n + i];
  if (blockIdx.x == 0 && threadIdx.x == 0) cg_slot(sc, 0, nrhs, c)[0] = rho;
}

// grid (nblk, nrhs).  beta = r.z / previous r.z; p = z + beta p; block 0 fills the other slot: the
// new r.z and frozen = r.r <= tol^2 b.b.  A frozen column carries its slot over.
__global__ __launch_bounds__(256) void pcg_step_p_kernel(
    const double* __restrict__ rr, int nblk, const double* __restrict__ rz, int nz, int nrhs,
    int slot, double* __restrict__ sc, const double* __restrict__ bb, double tol2, int n,
    const double* __restrict__ Z, double* __restrict__ P) {
  __shared__ double red[256];
  const int c = blockIdx.y;
  const double* cur = cg_slot(sc, slot, nrhs, c);
  double* nxt = cg_slot(sc, slot ^ 1, nrhs, c);
  if (cur[1] != 0.0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      nxt[0] = cur[0];
      nxt[1] = 1.0;
    }
    return;
  }
  const double num =
      cg_block_sum((int)threadIdx.x < nblk ? rr[(size_t)c * CG_MAXB + threadIdx.x] : 0.0, red);
  const double rho = pcg_sum_rz(rz + (size_t)c * PCH_MAXB, nz, red);
  const double beta = rho / cur[0];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const size_t k = (size_t)c * n + i;
    P[k] = fma(beta, P[k], Z[k]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    nxt[0] = rho;
    nxt[1] = num <= tol2 * bb[c] ? 1.0 : 0.0;
  }
}

// grid (nblk, nrhs).  part[c][blk] = partial ||b - q||^2
__global__ __launch_bounds__(256) void cg_resid_kernel(const double* __restrict__ B, size_t ldb,
                                                       const double* __restrict__ Q, int n,
                                                       double* __restrict__ part) {
  __shared__ double red[256];
  const int c = blockIdx.y;
  double s = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double r = B[(size_t)c * ldb + i] - Q[(size_t)c * n + i];
    s = fma(r, r, s);
  }
  s = cg_block_sum(s, red);
  if (threadIdx.x == 0) part[(size_t)c * CG_MAXB + blockIdx.x] = s;
}

// grid nrhs.  out[c] = the sum of the column's partials
__global__ __launch_bounds__(256) void cg_sum_kernel(const double* __restrict__ part, int nblk,
                                                     double* __restrict__ out) {
  __shared__ double red[256];
  const int c = blockIdx.x;
  const double s =
      cg_block_sum((int)threadIdx.x < nblk ? part[(size_t)c * CG_MAXB + threadIdx.x] : 0.0, red);
  if (threadIdx.x == 0) out[c] = s;
}

// ---- iterative refinement around the recurrence (GPR_KMM_PREC) --------------------------------
// grid nrhs.  The start of an inner solve K d = r from d = 0: s = r.r (the partials of
// cg_init_kernel); the column's stop threshold thr[c] = max(tol^2 b.b, floor2 s) -- floor2 = 2^-32:
// ||r_in|| <= max(tol ||b|| / ||r||, 2^-16) ||r||; 0: the FP64 recurrence to tol -- and slot 0:
// r.r = s, frozen when s <= thr (a column whose FP64 residual has met tol stays as it is)
__global__ __launch_bounds__(256) void cg_refine_scalars_kernel(const double* __restrict__ part,
                                                                int nblk, int nrhs, double tol2,
                                                                double floor2,
                                                                const double* __restrict__ bb,
                                                                double* __restrict__ sc,
                                                                double* __restrict__ thr) {
  __shared__ double red[256];
  const int c = blockIdx.x;
  const double s =
      cg_block_sum((int)threadIdx.x < nblk ? part[(size_t)c * CG_MAXB + threadIdx.x] : 0.0, red);
  if (threadIdx.x == 0) {
    const double t = fmax(tol2 * bb[c], floor2 * s);
    thr[c] = t;
    double* o = cg_slot(sc, 0, nrhs, c);
    o[0] = s;
    o[1] = s <= t ? 1.0 : 0.0;
  }
}

// grid (nblk, nrhs).  x += d
__global__ __launch_bounds__(256) void cg_add_kernel(const double* __restrict__ D, int n,
                                                     double* __restrict__ X, size_t ldx) {
  const int c = blockIdx.y;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    X[(size_t)c * ldx + i] += D[(size_t)c * n + i];
}

// grid (nblk, nrhs).  r = b - q, stored; part[c][blk] = partial ||r||^2
__global__ __launch_bounds__(256) void cg_resid_store_kernel(const double* __restrict__ B,
                                                             size_t ldb,
                                                             const double* __restrict__ Q, int n,
                                                             double* __restrict__ R,
                                                             double* __restrict__ part) {
  __shared__ double red[256];
  const int c = blockIdx.y;
  double s = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double r = B[(size_t)c * ldb + i] - Q[(size_t)c * n + i];
    R[(size_t)c * n + i] = r;
    s = fma(r, r, s);
  }
  s = cg_block_sum(s, red);
  if (threadIdx.x == 0) part[(size_t)c * CG_MAXB + blockIdx.x] = s;
}

// K's constant diagonal in the GPR_SELF form
double cg_diagonal(const KParams& kp) {
  double dg = kp.has_noise ? kp.noise2 : 0.0, term = 1.0;
  for (int p = 0; p < kp.nse; ++p) {
    const double s = kp_sigma(kp, p);
    term *= s * s;
    if (kp_closes(kp, p)) {
      dg += term + kp.eps;
      term = 1.0;
    }
  }
  return dg;
}

struct PinnedDoubles {  // the stop test's host copy
  double* p = nullptr;
  ~PinnedDoubles() {
    if (p) (void)hipHostFree(p);
  }
};

// the solve: rank 0 is the plain recurrence, rank > 0 the preconditioned one (rank_out: the rank
// the factor reached)
int cg_solve(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d, const double* dX,
             int n, const double* dB, int nrhs, int ldb, double eps, double tol, int maxit,
             int rank, double rtol, double* dXout, int ldx, int* iters, double* relres,
             int* rank_out) {
  KParams kp;
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, eps, &kp, nullptr));
  if (!dX) return set_err(ctx, GPR_E_ARG, "dX is NULL");
  if (!dB) return set_err(ctx, GPR_E_ARG, "dB is NULL");
  if (!dXout) return set_err(ctx, GPR_E_ARG, "dXout is NULL");
  if (n < 1) return set_err(ctx, GPR_E_ARG, "n=%d < 1", n);
  if (nrhs < 1) return set_err(ctx, GPR_E_ARG, "nrhs=%d < 1", nrhs);
  if (ldb < n) return set_err(ctx, GPR_E_ARG, "ldb=%d < n=%d", ldb, n);
  if (ldx < n) return set_err(ctx, GPR_E_ARG, "ldx=%d < n=%d", ldx, n);
  if (!(tol > 0.0)) return set_err(ctx, GPR_E_ARG, "tol=%g is not positive", tol);
  if (maxit < 0) return set_err(ctx, GPR_E_ARG, "maxit=%d < 0", maxit);
  if (rank < 0 || rank > 256)
    return set_err(ctx, GPR_E_ARG, "rank=%d outside [0, 256]", rank);
  if (!(rtol >= 0.0)) return set_err(ctx, GPR_E_ARG, "rtol=%g is negative", rtol);
  rank = std::min(rank, n);
  const bool pre = rank > 0;
  const double dinv = pre ? 1.0 : 1.0 / cg_diagonal(kp), tol2 = tol * tol;
  const size_t nn = (size_t)n * nrhs, np = (size_t)nrhs * CG_MAXB;
  PcholOps pc{};
  if (pre) GPR_TRY(pchol_prepare(ctx, kp, dX, n, rank, rtol, nrhs, &pc));
  if (rank_out) *rank_out = pre ? pc.k : 0;
  int nz = 0;
  KmmOps ops;
  GPR_TRY(kmm_prepare(ctx, kp, dX, n, nullptr, n, GPR_SELF, &ops, true));
  const bool mixed = ops.fa != nullptr;  // GPR_KMM_PREC, a description its kernel takes
  // r | p | q | p.q partials | r.r partials | two scalar slots | b.b | the final residuals
  // (| z | r.z partials, preconditioned) (| d | the FP64 residual | thresholds, refined)
  const size_t npre = pre ? nn + (size_t)nrhs * PCH_MAXB : 0;
  GPR_TRY(ensure_buf(ctx, ctx->dcg, 3 * nn + 2 * np + 6 * (size_t)nrhs + npre +
                                        (mixed ? 2 * nn + nrhs : 0)));
  double* R = ctx->dcg;
  double *P = R + nn, *Q = P + nn, *pq = Q + nn, *rr = pq + np, *sc = rr + np;
  double *bb = sc + 4 * (size_t)nrhs, *res = bb + nrhs;
  double *Z = res + nrhs, *rz = Z + nn;
  double *Dx = res + nrhs + npre, *Ro = Dx + nn, *thr = Ro + nn;
  PinnedDoubles host;
  HIP_TRY(ctx, hipHostMalloc((void**)&host.p, sizeof(double) * 2 * nrhs, hipHostMallocDefault));
  const int nblk = std::max(1, std::min(CG_MAXB, (n + 1023) / 1024));
  const dim3 grid((unsigned)nblk, (unsigned)nrhs);
  hipStream_t st = ctx->stream;
  // the stop test reads the slot's (r.r, frozen) pairs: every column frozen
  auto all_frozen = [&](int slot, bool* done) {
    HIP_TRY(ctx, hipMemcpyAsync(host.p, cg_slot(sc, slot, nrhs, 0), sizeof(double) * 2 * nrhs,
                                hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *done = true;
    for (int c = 0; c < nrhs; ++c)
      if (host.p[2 * c + 1] == 0.0) *done = false;
    return 0;
  };
  int it = 0;
  // the recurrence from R, P and slot 0 as initialised, into Xd: products of precision prec
  // (kmm_apply's), a column frozen at r.r <= t2 stop[c]; every product counts in it, capped at maxit
  auto recur = [&](double* Xd, size_t ldxd, const double* stop, double t2, int prec) {
    if (pre) {
      GPR_TRY(pchol_apply(ctx, pc, R, nrhs, Z, rz, &nz));
      pcg_start_kernel<<<grid, 256, 0, st>>>(rz, nz, nrhs, sc, n, Z, P);
    }
    LAUNCH_CHECK(ctx);
    int k = 0;
    bool done = false;
    GPR_TRY(all_frozen(0, &done));
    while (!done && it < maxit) {
      const int slot = k & 1;
      GPR_TRY(kmm_apply(ctx, ops, P, nrhs, n, Q, n, prec));
      cg_dot_kernel<<<grid, 256, 0, st>>>(P, Q, n, pq);
      cg_step_xr_kernel<<<grid, 256, 0, st>>>(pq, nblk, nrhs, slot, sc, dinv, n, P, Q, Xd, ldxd, R,
                                              rr);
      if (pre) {
        GPR_TRY(pchol_apply(ctx, pc, R, nrhs, Z, rz, &nz));
        pcg_step_p_kernel<<<grid, 256, 0, st>>>(rr, nblk, rz, nz, nrhs, slot, sc, stop, t2, n, Z, P);
      } else {
        cg_step_p_kernel<<<grid, 256, 0, st>>>(rr, nblk, nrhs, slot, sc, stop, t2, dinv, n, R, P);
      }
      LAUNCH_CHECK(ctx);
      ++k;
      ++it;
      GPR_TRY(all_frozen(k & 1, &done));
    }
    return 0;
  };
  bool have_res = false;  // res holds ||b - K x||^2 of the x returned
  if (!mixed) {
    cg_init_kernel<<<grid, 256, 0, st>>>(dB, (size_t)ldb, n, dinv, dXout, (size_t)ldx, R, P, rr);
    cg_init_scalars_kernel<<<nrhs, 256, 0, st>>>(rr, nblk, nrhs, tol2, sc, bb);
    GPR_TRY(recur(dXout, (size_t)ldx, bb, tol2, 0));
  } else {
    // Iterative refinement: x = 0, r = b; per outer step the recurrence on K~ d = r (the FP32
    // kernel's matrix) to the column's threshold, x += d, r = b - K x by one FP64 product.  A
    // column is done when that residual meets tol.  An outer step that takes a column's residual
    // down by less than 4 x (cond_2(K) ||K~ - K|| / ||K|| is not small) sends the rest of the call
    // to FP64 products: the recurrence on K d = r to tol.
    ctx->cg_outer = ctx->cg_f64 = 0;
    cg_init_kernel<<<grid, 256, 0, st>>>(dB, (size_t)ldb, n, dinv, dXout, (size_t)ldx, Ro, P, rr);
    cg_sum_kernel<<<nrhs, 256, 0, st>>>(rr, nblk, bb);
    cg_sum_kernel<<<nrhs, 256, 0, st>>>(rr, nblk, res);
    LAUNCH_CHECK(ctx);
    std::vector<double> prev(nrhs), b2(nrhs);
    auto read_res = [&]() {  // (bb and res are adjacent: one copy)
      HIP_TRY(ctx, hipMemcpyAsync(host.p, bb, sizeof(double) * 2 * nrhs, hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));
      return 0;
    };
    GPR_TRY(read_res());
    for (int c = 0; c < nrhs; ++c) b2[c] = host.p[c], prev[c] = host.p[nrhs + c];
    have_res = true;
    bool f64 = false;
    for (;;) {
      bool active = false;
      for (int c = 0; c < nrhs; ++c) active = active || prev[c] > tol2 * b2[c];
      if (!active || it >= maxit) break;
      cg_init_kernel<<<grid, 256, 0, st>>>(Ro, (size_t)n, n, dinv, Dx, (size_t)n, R, P, rr);
      cg_refine_scalars_kernel<<<nrhs, 256, 0, st>>>(rr, nblk, nrhs, tol2, f64 ? 0.0 : 0x1p-32, bb,
                                                     sc, thr);
      const int it0 = it;
      GPR_TRY(recur(Dx, (size_t)n, thr, 1.0, f64 ? 0 : 1));
      if (f64) ctx->cg_f64 += it - it0;
      cg_add_kernel<<<grid, 256, 0, st>>>(Dx, n, dXout, (size_t)ldx);
      LAUNCH_CHECK(ctx);
      ++ctx->cg_outer;
      have_res = false;
      if (it >= maxit) break;
      GPR_TRY(kmm_apply(ctx, ops, dXout, nrhs, ldx, Q, n, 0));
      ++it;
      ++ctx->cg_f64;
      cg_resid_store_kernel<<<grid, 256, 0, st>>>(dB, (size_t)ldb, Q, n, Ro, rr);
      cg_sum_kernel<<<nrhs, 256, 0, st>>>(rr, nblk, res);
      LAUNCH_CHECK(ctx);
      GPR_TRY(read_res());
      have_res = true;
      for (int c = 0; c < nrhs; ++c) {
        const double now = host.p[nrhs + c];
        // (a column the step has brought to tol is done, whatever the step gained)
        if (now > tol2 * b2[c] && now > prev[c] / 16.0) f64 = true;
        prev[c] = now;
      }
    }
  }
  if (iters) *iters = it;
  if (relres) {  // the true residual
    if (!have_res) {
      GPR_TRY(kmm_apply(ctx, ops, dXout, nrhs, ldx, Q, n, 0));
      cg_resid_kernel<<<grid, 256, 0, st>>>(dB, (size_t)ldb, Q, n, rr);
      cg_sum_kernel<<<nrhs, 256, 0, st>>>(rr, nblk, res);
      LAUNCH_CHECK(ctx);
    }
    // (bb and res are adjacent: one copy)
    HIP_TRY(ctx, hipMemcpyAsync(host.p, bb, sizeof(double) * 2 * nrhs, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int c = 0; c < nrhs; ++c)
      relres[c] = host.p[c] > 0.0 ? std::sqrt(host.p[nrhs + c] / host.p[c]) : 0.0;
  }
  return 0;
}

}  // namespace

extern "C" {

int gpr_solve_cg(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                 const double* dX, int n, const double* dB, int nrhs, int ldb, double eps,
                 double tol, int maxit, double* dXout, int ldx, int* iters, double* relres) {
  return cg_solve(ctx, kinds, nk, hp, d, dX, n, dB, nrhs, ldb, eps, tol, maxit,
                  ctx ? ctx->cg_precond : 0, 0.0, dXout, ldx, iters, relres, nullptr);
}

int gpr_solve_pcg(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                  const double* dX, int n, const double* dB, int nrhs, int ldb, double eps,
                  double tol, int maxit, int rank, double rtol, double* dXout, int ldx, int* iters,
                  double* relres, int* rank_out) {
  return cg_solve(ctx, kinds, nk, hp, d, dX, n, dB, nrhs, ldb, eps, tol, maxit, rank, rtol, dXout,
                  ldx, iters, relres, rank_out);
}

}  // extern "C"
