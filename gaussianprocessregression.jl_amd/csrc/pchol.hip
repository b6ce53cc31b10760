// A pivoted-Cholesky preconditioner for the matrix-free CG solve (cg.hip).
//
// K = K_c + delta I for the GPR_SELF matrix: K_c the cross-form kernel of (cov, hp, x, x) -- no
// eps, no noise, constant diagonal c = sum over terms of the factors' sigma^2 product -- and
// delta = sigma_n^2 + eps (number of terms).  With L (n x k) the rank-k partial pivoted Cholesky
// of K_c the preconditioner is P = L L^T + delta I, applied through the Woodbury identity
//     P^{-1} r = (r - L C^{-1} L^T r) / delta,   C = delta I_k + L^T L  (k x k, SPD).
//
// Building L: pchol_step_kernel, one launch per step m, enqueued back to back -- no host round
// trip, no cooperative launch, no atomics.  A 1-D grid of 256-thread blocks, each owning a fixed
// set of points (block b: points b 256 + t + s 256 nblk).  The state is on the device: L
// (column-major: a step writes one contiguous column), the residual diagonal dres, the pivots,
// two sets of per-block (max, index) partials (a step reads one and writes the other, so a fast
// block cannot overwrite what a slow one still reads) and a (stopped, rank) flag.
//   1. every block reduces the previous step's <= 256 partials in the same fixed tree, ties to
//      the lower index: all agree on the pivot i and d_i without a second launch;
//   2. d_i <= rtol n c: block 0 raises the flag with rank = m; this and every later step return
//      at once and write nothing.  (rtol = 0 stops only at d_i <= 0, where the step's square root
//      has no meaning.)
//   3. K_c(x_a, x_i) straight from differences (kpair_dist on raw x, on the unit features for a
//      Periodic part) with kexp.hpp's profiles, the description walked at run time: a term the
//      product of its factors, the kernel the sum of its terms -- every kind, any d, any number
//      of parts.  P only has to be SPD and close to K, so these need not be the Gram route's bits;
//   4. L[a, m] = (K_c(x_a, x_i) - sum_{j<m} L[a, j] L[i, j]) / sqrt(d_i): the pivot's row in LDS
//      once per block, one fixed-order chain per point, the earlier columns read coalesced across
//      points -- n m doubles per step, n k^2 / 2 in all, the build's byte floor;
//   5. dres[a] -= L[a, m]^2, clamped at 0; a chosen pivot carries the marker -1; the block's new
//      (max, index) partial.
//
// Applying P^{-1}, every CG iteration, on v_mfma_f64_16x16x4:
//   pchol_lt_kernel   T = L^T R partials.  Grid (slabs of points, 16-column blocks of L, 16-column
//                     blocks of R).  A workgroup walks its slab 128 points at a time: L's and R's
//                     128 x 16 blocks are staged in LDS column by column with stride 130 doubles
//                     (a half wave's operand read -- 16 columns x 2 points -- touches 32 distinct
//                     bank pairs), the next block fetched into registers before the products;
//                     wave w multiplies points [32 w, 32 w + 32) (A[m][k] = L[point k, column m],
//                     B[k][n] = R[point k, column n]); the four waves' 16 x 16 blocks are added in
//                     wave order through LDS.  Ragged n, k, nrhs enter as exact zeros.
//   pchol_reduce_kernel  adds the slabs' partials in slab order (+ delta on the diagonal for C):
//                     no atomics, two calls agree bit for bit.
//   (t = C^{-1} T by gpr_potrs_upper's sweeps on C's factor from gpr_potrf_upper.)
//   pchol_z_kernel    Z = (R - L t) / delta as Z^T = t^T L^T: t (k x 16) in LDS for the launch
//                     (A[m][k'] = t[j + k', column m], lane-consecutive: conflict-free), L's
//                     elements straight from memory as the B operand (B[k'][n] = L[point n, j +
//                     k']: 16 consecutive points per column, 128-byte runs), a wave owning 16
//                     points; the result's lanes hold 16 consecutive points of 4 columns, so R is
//                     read and Z written in 128-byte runs.  Fused with the recurrence's next need:
//                     the block's partial of r.z per column, summed in a fixed order.
// Both passes read L once: 2 x 8 n k bytes per iteration.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.hpp"
#include "kexp.hpp"

namespace {

constexpr int PCH_BLKS = 256;    // most blocks (pivot partials) of a build step
constexpr int PCH_PTS = 512;     // points a build block owns before the grid stops growing
constexpr int PCH_MAXK = 256;    // largest rank
constexpr int LT_PTS = 128;      // points per staged block of the L^T R product
constexpr int LT_STR = LT_PTS + 2;
constexpr int LT_MAXS = 64;      // most slabs
typedef double pd4 __attribute__((ext_vector_type(4)));

// (max, index) over the 256 threads by a fixed tree, ties to the lower index; every thread gets it
__device__ __forceinline__ void pch_argmax(double& v, int& i, double* rv, int* ri) {
  const int t = threadIdx.x;
  __syncthreads();
  rv[t] = v;
  ri[t] = i;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      const double ov = rv[t + w];
      const int oi = ri[t + w];
      if (ov > rv[t] || (ov == rv[t] && oi < ri[t])) {
        rv[t] = ov;
        ri[t] = oi;
      }
    }
    __syncthreads();
  }
  v = rv[0];
  i = ri[0];
}

// the build's device state
struct PchState {
  double* dres;  // [n]
  double* pmax;  // [2][PCH_BLKS]
  int* pidx;     // [2][PCH_BLKS]
  int* piv;      // [PCH_MAXK]
  int* flag;     // stopped, rank
};

// dres = c, the partials of step 0 (the first point wins the tie), the flag
__global__ __launch_bounds__(256) void pchol_start_kernel(PchState s, int n, double c, int rank) {
  __shared__ double rv[256];
  __shared__ int ri[256];
  double v = -2.0;
  int idx = INT_MAX;
  for (size_t a = (size_t)blockIdx.x * 256 + threadIdx.x; a < (size_t)n;
       a += (size_t)gridDim.x * 256) {
    s.dres[a] = c;
    if (idx == INT_MAX) {
      v = c;
      idx = (int)a;
    }
  }
  pch_argmax(v, idx, rv, ri);
  if (threadIdx.x == 0) {
    s.pmax[blockIdx.x] = v;
    s.pidx[blockIdx.x] = idx;
    if (blockIdx.x == 0) {
      s.flag[0] = 0;
      s.flag[1] = rank;
    }
  }
}

// f(D) of a part's profile with the unscaled table tab[j] = 2^(j/256)
__device__ __forceinline__ double pch_profile(int prof, double D, const double* tab) {
  if (prof == 1) return kprof_s2<1>(D, tab);
  if (prof == 2) return kprof_s2<2>(D, tab);
  return kprof_s2<0>(D, tab);
}

// K_c(x_a, x_i): the sum over terms of the product over factors of sigma^2 f(D)
__device__ __forceinline__ double pch_element(const KParams& kp, const double* __restrict__ X,
                                              const double* __restrict__ cs, int n, size_t a,
                                              size_t i, const double* tab) {
  const int d = kp.dx, de = kp.de;
  double sum = 0.0, term = 1.0;
  for (int p = 0; p < kp.nse; ++p) {
    const bool per = kp.nper && kp.per[p] != 0.0;
    const double* cp = per ? cs + (size_t)p * n * de : nullptr;
    const double D = kpair_dist(per, d, kp.l2 + (size_t)p * d, X + a * d, X + i * d,
                                per ? cp + a * de : nullptr, per ? cp + i * de : nullptr);
    const double sg = kp.sig[p];
    term *= (sg * sg) * pch_profile((int)kp.pf[p], D, tab);
    if (kp.tend[p] != 0.0) {
      sum += term;
      term = 1.0;
    }
  }
  return sum;
}

// step m of the factorisation (the file comment's 1 - 5).  grid nblk <= PCH_BLKS
__global__ __launch_bounds__(256) void pchol_step_kernel(KParams kp, const double* __restrict__ X,
                                                         const double* __restrict__ cs, int n,
                                                         double* __restrict__ L, size_t ldl,
                                                         PchState s, int m, double thresh) {
  __shared__ double rv[256];
  __shared__ int ri[256];
  __shared__ double tab[256];
  __shared__ double lrow[PCH_MAXK];
  if (s.flag[0] != 0) return;  // (written by an earlier launch: grid-uniform)
  const int t = threadIdx.x, nblk = gridDim.x;
  const int in = (m & 1) * PCH_BLKS, out = ((m + 1) & 1) * PCH_BLKS;
  double di = t < nblk ? s.pmax[in + t] : -2.0;
  int piv = t < nblk ? s.pidx[in + t] : INT_MAX;
  pch_argmax(di, piv, rv, ri);
  if (!(di > thresh)) {  // (every block decides the same from the same partials)
    if (blockIdx.x == 0 && t == 0) {
      s.flag[0] = 1;
      s.flag[1] = m;
    }
    return;
  }
  if (blockIdx.x == 0 && t == 0) s.piv[m] = piv;
  tab[t] = kp.exptab[t];
  for (int j = t; j < m; j += 256) lrow[j] = L[(size_t)piv + (size_t)j * ldl];
  __syncthreads();
  const double sq = sqrt(di);
  double bv = -2.0;
  int bi = INT_MAX;
  for (size_t a = (size_t)blockIdx.x * 256 + t; a < (size_t)n; a += (size_t)nblk * 256) {
    double v = pch_element(kp, X, cs, n, a, (size_t)piv, tab);
    const double* la = L + a;
    for (int j = 0; j < m; ++j) v = fma(-la[(size_t)j * ldl], lrow[j], v);
    v /= sq;
    L[a + (size_t)m * ldl] = v;
    const double da = s.dres[a];
    double nd = -1.0;  // a chosen pivot
    if (da >= 0.0 && a != (size_t)piv) nd = fmax(fma(-v, v, da), 0.0);
    s.dres[a] = nd;
    if (nd > bv) {  // (a ascends: the lower index keeps a tie)
      bv = nd;
      bi = (int)a;
    }
  }
  pch_argmax(bv, bi, rv, ri);
  if (t == 0) {
    s.pmax[out + blockIdx.x] = bv;
    s.pidx[out + blockIdx.x] = bi;
  }
}

// this thread's share of points [a0, a0 + 128) x 16 columns from c0 of M (ld ldm, nc columns):
// point (t & 127), columns (t >> 7) + 2 q.  Zero past n or nc, and nothing past them is read.
__device__ __forceinline__ void lt_fetch(const double* __restrict__ M, size_t ldm, int n, int nc,
                                         size_t a0, int c0, double (&r)[8]) {
  const size_t a = a0 + (threadIdx.x & 127);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int c = c0 + (int)(threadIdx.x >> 7) + 2 * q;
    r[q] = (a < (size_t)n && c < nc) ? M[(size_t)c * ldm + a] : 0.0;
  }
}
__device__ __forceinline__ void lt_stage(const double (&r)[8], double* S) {
#pragma unroll
  for (int q = 0; q < 8; ++q) S[((threadIdx.x >> 7) + 2 * q) * LT_STR + (threadIdx.x & 127)] = r[q];
}

// W[slab][k x nrhs] = the slab's part of L^T R.  grid (slabs, ceil(k / 16), ceil(nrhs / 16)).
__global__ __launch_bounds__(256) void pchol_lt_kernel(const double* __restrict__ L, size_t ldl,
                                                       int n, int k, const double* __restrict__ R,
                                                       size_t ldr, int nrhs, int slab_blocks,
                                                       double* __restrict__ W) {
  __shared__ double Ls[16 * LT_STR];
  __shared__ double Rs[16 * LT_STR];
  __shared__ double red[4 * 256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int j0 = blockIdx.y * 16, c0 = blockIdx.z * 16;
  const int nb = (n + LT_PTS - 1) / LT_PTS;
  const int b_lo = blockIdx.x * slab_blocks, b_hi = min(b_lo + slab_blocks, nb);
  pd4 acc = {0.0, 0.0, 0.0, 0.0};
  double lr[8], rr[8];
  lt_fetch(L, ldl, n, k, (size_t)b_lo * LT_PTS, j0, lr);
  lt_fetch(R, ldr, n, nrhs, (size_t)b_lo * LT_PTS, c0, rr);
  lt_stage(lr, Ls);
  lt_stage(rr, Rs);
  __syncthreads();
  const int off = (lane & 15) * LT_STR + 32 * w + (lane >> 4);
  for (int b = b_lo; b < b_hi; ++b) {
    const bool more = b + 1 < b_hi;
    if (more) {  // lands under the products
      lt_fetch(L, ldl, n, k, (size_t)(b + 1) * LT_PTS, j0, lr);
      lt_fetch(R, ldr, n, nrhs, (size_t)(b + 1) * LT_PTS, c0, rr);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ls[off + 4 * q], Rs[off + 4 * q], acc, 0, 0, 0);
    __syncthreads();  // the block is read
    if (more) {
      lt_stage(lr, Ls);
      lt_stage(rr, Rs);
    }
    __syncthreads();
  }
  // D: lane l, register q = (L column j0 + (l >> 4) + 4 q, R column c0 + (l & 15))
#pragma unroll
  for (int q = 0; q < 4; ++q) red[w * 256 + q * 64 + lane] = acc[q];
  __syncthreads();
  {
    const int e = threadIdx.x, q = e >> 6, l = e & 63;
    const int j = j0 + (l >> 4) + 4 * q, c = c0 + (l & 15);
    const double v = ((red[e] + red[256 + e]) + red[512 + e]) + red[768 + e];
    if (j < k && c < nrhs) W[((size_t)blockIdx.x * nrhs + c) * k + j] = v;
  }
}

// T[j, c] (ldt) = W_0 + W_1 + ... in slab order (+ delta where j == c and diag)
__global__ __launch_bounds__(256) void pchol_reduce_kernel(const double* __restrict__ W, int nslab,
                                                           int k, int nrhs, double delta, int diag,
                                                           double* __restrict__ T, size_t ldt) {
  const size_t total = (size_t)k * nrhs;
  for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t c = e / k, j = e - c * k;
    double v = W[e];
    for (int sl = 1; sl < nslab; ++sl) v += W[(size_t)sl * total + e];
    if (diag && j == c) v += delta;
    T[c * ldt + j] = v;
  }
}

// Z = (R - L t) / delta and rz[c][block] = the block's part of r_c . z_c.  grid (nblk <= PCH_MAXB,
// ceil(nrhs / 16)); a wave owns 16 points of a 64-point tile, the grid strides over the tiles.
// Dynamic LDS: t's block, ceil(k / 4) 4 x 16 doubles.
__global__ __launch_bounds__(256) void pchol_z_kernel(const double* __restrict__ L, size_t ldl,
                                                      int n, int k, const double* __restrict__ T,
                                                      size_t ldt, const double* __restrict__ R,
                                                      int nrhs, double dinv, double* __restrict__ Z,
                                                      double* __restrict__ rz) {
  extern __shared__ double ts[];  // ts[j * 16 + column]
  __shared__ double sred[4 * 256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c0 = blockIdx.y * 16, kp4 = (k + 3) / 4 * 4;
  for (int e = threadIdx.x; e < kp4 * 16; e += 256) {
    const int j = e >> 4, c = c0 + (e & 15);
    ts[e] = (j < k && c < nrhs) ? T[(size_t)c * ldt + j] : 0.0;
  }
  __syncthreads();
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  const size_t ntile = ((size_t)n + 63) / 64;
  for (size_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const size_t a = tile * 64 + 16 * w + (lane & 15);
    const size_t ac = a < (size_t)n ? a : (size_t)n - 1;  // (a clamped point is not stored)
    pd4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < kp4; j += 4) {
      const int jl = min(j + (lane >> 4), k - 1);  // (t's padded rows are zero)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ts[j * 16 + lane], L[ac + (size_t)jl * ldl], acc,
                                                 0, 0, 0);
    }
    // D: lane l, register q = (column c0 + (l >> 4) + 4 q, point l & 15)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + (lane >> 4) + 4 * q;
      if (a < (size_t)n && c < nrhs) {
        const double r = R[(size_t)c * n + a];
        const double z = (r - acc[q]) * dinv;
        Z[(size_t)c * n + a] = z;
        s[q] = fma(r, z, s[q]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) sred[q * 256 + threadIdx.x] = s[q];
  __syncthreads();
  if (threadIdx.x < 16) {  // column c0 + cc: its 64 lane sums, wave by wave
    const int cc = threadIdx.x, q = cc >> 2, g = cc & 3;
    double v = 0.0;
    for (int ww = 0; ww < 4; ++ww)
      for (int i = 0; i < 16; ++i) v += sred[q * 256 + ww * 64 + g * 16 + i];
    if (c0 + cc < nrhs) rz[(size_t)(c0 + cc) * PCH_MAXB + blockIdx.x] = v;
  }
}

// c = sum over terms of the factors' sigma^2 product; delta = sigma_n^2 + eps per term
void pch_diagonal(const KParams& kp, double* c, double* delta) {
  double cc = 0.0, dl = kp.has_noise ? kp.noise2 : 0.0, term = 1.0;
  for (int p = 0; p < kp.nse; ++p) {
    const double s = kp_sigma(kp, p);
    term *= s * s;
    if (kp_closes(kp, p)) {
      cc += term;
      dl += kp.eps;
      term = 1.0;
    }
  }
  *c = cc;
  *delta = dl;
}

// W (ctx->dpchw) and Out (k x nrhs, ldo) = L^T R (+ delta I)
int pch_lt(gpr_ctx* ctx, const double* L, size_t ldl, int n, int k, const double* R, size_t ldr,
           int nrhs, double delta, int diag, double* Out, size_t ldo) {
  const int nb = (n + LT_PTS - 1) / LT_PTS;
  const int kb = (k + 15) / 16, rb = (nrhs + 15) / 16;
  const int ncu = ctx->ncu > 0 ? ctx->ncu : 256;
  int slabs = std::max(1, std::min((2 * ncu + kb * rb - 1) / (kb * rb), std::min(nb, LT_MAXS)));
  const int slab_blocks = (nb + slabs - 1) / slabs;
  slabs = (nb + slab_blocks - 1) / slab_blocks;  // (no empty slab)
  GPR_TRY(ensure_buf(ctx, ctx->dpchw, (size_t)slabs * k * nrhs));
  pchol_lt_kernel<<<dim3((unsigned)slabs, (unsigned)kb, (unsigned)rb), 256, 0, ctx->stream>>>(
      L, ldl, n, k, R, ldr, nrhs, slab_blocks, ctx->dpchw);
  const int blocks = (int)std::min<size_t>(((size_t)k * nrhs + 255) / 256, 1024);
  pchol_reduce_kernel<<<blocks, 256, 0, ctx->stream>>>(ctx->dpchw, slabs, k, nrhs, delta, diag, Out,
                                                       ldo);
  LAUNCH_CHECK(ctx);
  return 0;
}

}  // namespace

int pchol_factor(gpr_ctx* ctx, const KParams& kp, const double* dX, int n, int rank, double rtol,
                 double* dL, int ldl, int* piv, int* rank_out) {
  double c, delta;
  pch_diagonal(kp, &c, &delta);
  // dres | two sets of partial maxima | their indices, the pivots and the flag (ints)
  const size_t nint = 2 * PCH_BLKS + PCH_MAXK + 2;
  GPR_TRY(ensure_buf(ctx, ctx->dpch, (size_t)n + 2 * PCH_BLKS + (nint + 1) / 2));
  PchState s;
  s.dres = ctx->dpch;
  s.pmax = s.dres + n;
  s.pidx = reinterpret_cast<int*>(s.pmax + 2 * PCH_BLKS);
  s.piv = s.pidx + 2 * PCH_BLKS;
  s.flag = s.piv + PCH_MAXK;
  if (kp.nper) GPR_TRY(launch_embed_unit_to(ctx, kp, dX, n, ctx->dpchcs));
  const double* cs = kp.nper ? ctx->dpchcs.p : nullptr;
  const int nblk = std::max(1, std::min(PCH_BLKS, (n + PCH_PTS - 1) / PCH_PTS));
  hipStream_t st = ctx->stream;
  pchol_start_kernel<<<nblk, 256, 0, st>>>(s, n, c, rank);
  const double thresh = rtol * (double)n * c;
  for (int m = 0; m < rank; ++m)
    pchol_step_kernel<<<nblk, 256, 0, st>>>(kp, dX, cs, n, dL, (size_t)ldl, s, m, thresh);
  LAUNCH_CHECK(ctx);
  int host[PCH_MAXK + 2];  // (piv and flag are adjacent: one copy)
  HIP_TRY(ctx, hipMemcpyAsync(host, s.piv, sizeof(int) * (PCH_MAXK + 2), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  const int r = host[PCH_MAXK + 1];
  if (piv)
    for (int m = 0; m < r; ++m) piv[m] = host[m];
  *rank_out = r;
  return 0;
}

int pchol_prepare(gpr_ctx* ctx, const KParams& kp, const double* dX, int n, int rank, double rtol,
                  int nrhs, PcholOps* o) {
  double c, delta;
  pch_diagonal(kp, &c, &delta);
  if (!(delta > 0.0))
    return set_err(ctx, GPR_E_ARG, "the preconditioner needs sigma_n^2 + eps > 0 (delta=%g)", delta);
  const size_t nl = (size_t)n * rank, nc = (size_t)rank * rank;
  GPR_TRY(ensure_buf(ctx, ctx->dpchl, nl + nc + (size_t)rank * nrhs));
  double* L = ctx->dpchl;
  int r = 0;
  GPR_TRY(pchol_factor(ctx, kp, dX, n, rank, rtol, L, n, nullptr, &r));
  o->L = L;
  o->n = n;
  o->k = r;
  o->nrhs = nrhs;
  o->delta = delta;
  double* C = L + nl;
  o->U = C;
  o->T = C + nc;
  if (r == 0) return 0;  // (P = delta I)
  GPR_TRY(pch_lt(ctx, L, (size_t)n, n, r, L, (size_t)n, r, delta, 1, C, (size_t)r));
  int info = 0;
  GPR_TRY(potrf_core(ctx, C, r, r, &info));
  if (info != 0)
    return set_err(ctx, GPR_E_HIP, "the preconditioner's C = delta I + L^T L is not positive "
                   "definite (minor %d of %d)", info, r);
  return 0;
}

int pchol_apply(gpr_ctx* ctx, const PcholOps& o, const double* R, int nrhs, double* Z, double* rz,
                int* nblk) {
  const int n = o.n, k = o.k;
  const int blocks = (int)std::max<size_t>(1, std::min<size_t>(((size_t)n + 63) / 64, PCH_MAXB));
  *nblk = blocks;
  if (k > 0) {
    GPR_TRY(pch_lt(ctx, o.L, (size_t)n, n, k, R, (size_t)n, nrhs, 0.0, 0, o.T, (size_t)k));
    GPR_TRY(potrs_core(ctx, o.U, k, k, o.T, nrhs, k));
  }
  // (rank 0 reached: one zero row of t, so that the pass still forms z = r / delta and r.z)
  const int ke = std::max(k, 1);
  const size_t lds = sizeof(double) * (size_t)((ke + 3) / 4 * 4) * 16;
  pchol_z_kernel<<<dim3((unsigned)blocks, (unsigned)((nrhs + 15) / 16)), 256, lds, ctx->stream>>>(
      o.L, (size_t)n, n, k > 0 ? k : 0, o.T, (size_t)ke, R, nrhs, 1.0 / o.delta, Z, rz);
  LAUNCH_CHECK(ctx);
  return 0;
}

extern "C" {

int gpr_pchol(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d, const double* dX,
              int n, double eps, int rank, double rtol, double* dL, int ldl, int* piv,
              int* rank_out) {
  KParams kp;
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, eps, &kp, nullptr));
  if (!dX) return set_err(ctx, GPR_E_ARG, "dX is NULL");
  if (!dL) return set_err(ctx, GPR_E_ARG, "dL is NULL");
  if (!piv) return set_err(ctx, GPR_E_ARG, "piv is NULL");
  if (!rank_out) return set_err(ctx, GPR_E_ARG, "rank_out is NULL");
  if (n < 1) return set_err(ctx, GPR_E_ARG, "n=%d < 1", n);
  if (rank < 1 || rank > std::min(n, PCH_MAXK))
    return set_err(ctx, GPR_E_ARG, "rank=%d outside [1, min(n=%d, %d)]", rank, n, PCH_MAXK);
  if (ldl < n) return set_err(ctx, GPR_E_ARG, "ldl=%d < n=%d", ldl, n);
  if (!(rtol >= 0.0)) return set_err(ctx, GPR_E_ARG, "rtol=%g is negative", rtol);
  return pchol_factor(ctx, kp, dX, n, rank, rtol, dL, ldl, piv, rank_out);
}

}  // extern "C"
