// gpr_fit_append: condition a fitted model on m more observations without refactoring it.
//
// With K = U^T U the fitted n0 x n0 block, B = K(x, x_new) (n0 x m) and K_new = K(x_new, x_new)
// in the GPR_SELF form, the factor of the extended matrix is the old factor plus m columns:
//   V = U^{-T} B,   S = K_new - V^T V = R^T R,   U' = [U V; 0 R]
// and alpha' = K'^{-1} y' by the block formula, with c = y_new - B^T alpha:
//   alpha'_tail = S^{-1} c,   alpha'_head = alpha - U^{-1} (V alpha'_tail).
// Nothing of the old n0 x n0 block is rewritten; the work is O(n0^2 m) and, for a skinny B, one
// pass over the upper triangle of U per 16 columns (append_fwd_sweep_kernel below), one more per
// two columns of y for alpha'_head (the backward sweep of potrs_core).
#include <algorithm>

#include "common.hpp"
#include "sweep_handoff.hpp"

namespace {

typedef double a2v __attribute__((ext_vector_type(2)));
typedef double a4v __attribute__((ext_vector_type(4)));

// ---- the skinny forward solve ------------------------------------------------------------------
// V = U^{-T} B in place for nc <= 16 columns in ONE launch that reads the upper triangle of U once:
// potrf.hip's ticketed left-looking pipeline (trsv_fwd_sweep_kernel) with the tile arithmetic on
// FP64 MFMA.  One workgroup per 128-column block b of U, handed out by an atomic ticket, so every
// block a workgroup waits on belongs to a workgroup that is already running; blocks finish in
// order, so one monotonic "blocks done" counter publishes them (sweep_handoff.hpp: sc1 stores ->
// vmcnt(0) drain -> barrier -> sc1 counter store; every wave polls for itself and loads its share of
// the block with sc1 loads only after its own poll matched).
//   V_b = W_b^T (B_b - sum_{k < b} U_kb^T V_k),   W_b = U_bb^{-1} (the context's block inverses)
// U_kb^T V_k is (128 x 128)^T x (128 x 16) on v_mfma_f64_16x16x4_f64: wave w owns columns
// [16 w, 16 w + 16) of the block (the A operand's rows), lane (q = lane >> 4, i = lane & 15) holds
// rows 8 s + 2 q + e (s < 16, e < 2) of column 16 w + i in registers -- a sum over the tile's 128
// rows may take them in any order -- and the same rows of V_k's column lane & 15 come from LDS, where
// the workgroup stages the 128 x 16 block once.  Tile k + 1 (after the last one: W_b, "tile b" of
// the same product) is requested before the wait on block k.  The hand-off buffer holds 128 x 16
// doubles per block, block-major, then column-major with 128 rows.
// sync[0] = ticket, sync[1] = blocks done; both zeroed before the launch.
constexpr int AS_NB = 128, AS_NC = 16, AS_THREADS = 512, AS_PITCH = 136;
constexpr int AS_BLK = AS_NB * AS_NC;  // doubles per hand-off block

// rows 8 s + 2 q + e of one column of a tile into u[2 s + e] (zeros when !ok; `col` is a valid
// address either way)
template <bool VEC>
__device__ __forceinline__ void as_load_tile(double (&u)[32], const double* __restrict__ col,
                                             bool ok, int q) {
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const double* p = col + 8 * s + 2 * q;
    double v0, v1;
    if (VEC) {
      const a2v v = *reinterpret_cast<const a2v*>(p);
      v0 = v.x;
      v1 = v.y;
    } else {
      v0 = p[0];
      v1 = p[1];
    }
    u[2 * s] = ok ? v0 : 0.0;
    u[2 * s + 1] = ok ? v1 : 0.0;
  }
}

// the same of column j of W_b = U_bb^{-1} (128 x 128, ld 128, 16-B aligned): rows <= j of the
// block's kb valid columns, zeros elsewhere (selected, never multiplied)
__device__ __forceinline__ void as_load_w(double (&u)[32], const double* __restrict__ col, int j,
                                          int kb, int q) {
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int i = 8 * s + 2 * q;
    const a2v v = *reinterpret_cast<const a2v*>(col + i);
    u[2 * s] = (j < kb && i <= j) ? v.x : 0.0;
    u[2 * s + 1] = (j < kb && i + 1 <= j) ? v.y : 0.0;
  }
}

// acc[e] (row q + 4 e, column lane & 15) += sum over the tile's 128 rows of u x the staged block
__device__ __forceinline__ a4v as_mma(const double (&u)[32], const double* __restrict__ vs, int q,
                                      int r) {
  a4v a0 = {0.0, 0.0, 0.0, 0.0}, a1 = {0.0, 0.0, 0.0, 0.0};
  const double* vr = vs + r * AS_PITCH + 2 * q;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const a2v b = *reinterpret_cast<const a2v*>(vr + 8 * s);
    a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(u[2 * s], b.x, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(u[2 * s + 1], b.y, a1, 0, 0, 0);
  }
  return a0 + a1;
}

template <bool VEC>
__global__ __launch_bounds__(AS_THREADS) void append_fwd_sweep_kernel(
    const double* __restrict__ U, size_t ldu, int n, const double* __restrict__ W, double* B,
    size_t ldb, int nc, double* hand, int* sync) {
  __shared__ int sblk;
  __shared__ __attribute__((aligned(16))) double vs[2][AS_NC * AS_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int q = lane >> 4, r = lane & 15;
  if (tid == 0) sblk = atomicAdd(&sync[0], 1);
  __syncthreads();
  const int b = sblk;
  const int c0 = b * AS_NB, kb = min(AS_NB, n - c0);
  const int j = w * 16 + r;  // this lane's column of the block (A operand)
  const bool jok = j < kb;
  const double* ucol = U + (size_t)(c0 + (jok ? j : 0)) * ldu;
  const double* wcol = W + (size_t)b * AS_NB * AS_NB + (size_t)j * AS_NB;
  double cur[32], nxt[32];
  if (b > 0)
    as_load_tile<VEC>(cur, ucol, jok, q);
  else
    as_load_w(cur, wcol, j, kb, q);
  a4v acc = {0.0, 0.0, 0.0, 0.0};
  int known = 0;
  for (int k = 0; k < b; ++k) {
    if (k + 1 < b)
      as_load_tile<VEC>(nxt, ucol + (size_t)(k + 1) * AS_NB, jok, q);
    else
      as_load_w(nxt, wcol, j, kb, q);
    sweep_wait(sync, k + 1, known, lane);
    double* buf = vs[k & 1];
    const double* hk = hand + (size_t)k * AS_BLK;
#pragma unroll
    for (int t = 0; t < AS_BLK / AS_THREADS; ++t) {
      const int idx = tid + t * AS_THREADS;
      const int cc = idx >> 7, row = idx & (AS_NB - 1);
      buf[cc * AS_PITCH + row] = cc < nc ? hand_ld(hk + idx) : 0.0;
    }
    __syncthreads();
    acc += as_mma(cur, buf, q, r);
#pragma unroll
    for (int t = 0; t < 32; ++t) cur[t] = nxt[t];
  }
  // R_b = B_b - the partial sums (rows beyond kb, columns beyond nc: zero), staged like a V block
  double* buf = vs[b & 1];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int jj = w * 16 + q + 4 * e;
    buf[r * AS_PITCH + jj] =
        (jj < kb && r < nc) ? B[(size_t)(c0 + jj) + (size_t)r * ldb] - acc[e] : 0.0;
  }
  __syncthreads();
  // V_b = W_b^T R_b: the same product with W_b as the tile
  const a4v out = as_mma(cur, buf, q, r);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int jj = w * 16 + q + 4 * e;
    if (jj < kb && r < nc) {
      hand_st(&hand[(size_t)b * AS_BLK + r * AS_NB + jj], out[e]);
      B[(size_t)(c0 + jj) + (size_t)r * ldb] = out[e];
    }
  }
  sweep_publish(sync, b + 1);
}

// ---- the small kernels around it ---------------------------------------------------------------
// K[n0 + j, i] = K[i, n0 + j] for i < n0, j < m: the strict-lower rows of the extended matrix
__global__ __launch_bounds__(256) void append_lower_rows_kernel(double* __restrict__ K, size_t ldk,
                                                                int n0, int m) {
  __shared__ double t[32][33];
  const int i0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int jj = ty; jj < 32; jj += 8) {
    const int i = i0 + tx, j = j0 + jj;
    t[jj][tx] = (i < n0 && j < m) ? K[(size_t)i + (size_t)(n0 + j) * ldk] : 0.0;
  }
  __syncthreads();
  for (int ii = ty; ii < 32; ii += 8) {
    const int i = i0 + ii, j = j0 + tx;
    if (i < n0 && j < m) K[(size_t)(n0 + j) + (size_t)i * ldk] = t[tx][ii];
  }
}

// c[j, r] = y[n0 + j, r] - sum_i K[i, n0 + j] alpha0[i, r] into out[n0 + j + r ldo]: one workgroup
// per (j, r), the sum in a fixed order (per thread by stride, then the wave, then the four waves)
__global__ __launch_bounds__(256) void append_mean_rhs_kernel(
    const double* __restrict__ K, size_t ldk, int n0, const double* __restrict__ alpha0,
    const double* __restrict__ y, size_t ldy, double* __restrict__ out, size_t ldo) {
  __shared__ double part[4];
  const int j = blockIdx.x, r = blockIdx.y;
  const double* col = K + (size_t)(n0 + j) * ldk;
  const double* a = alpha0 + (size_t)r * n0;
  double s = 0.0;
  for (int i = threadIdx.x; i < n0; i += 256) s = fma(col[i], a[i], s);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    out[(size_t)(n0 + j) + (size_t)r * ldo] =
        y[(size_t)(n0 + j) + (size_t)r * ldy] - ((part[0] + part[1]) + (part[2] + part[3]));
}

// Schur complement of a skinny append (m <= 128): workgroup s sums V^T V over its slab of
// SC_SLAB rows of V into partial[s] (128 x 128 slot, entries i <= j < m), thread (ti, tj) an
// 8 x 8 micro-tile; append_schur_reduce_kernel then adds the slabs in index order
constexpr int SC_SLAB = 256, SC_CH = 16, SC_P = AS_NB + 1;
__global__ __launch_bounds__(256) void append_schur_slab_kernel(const double* __restrict__ V,
                                                                size_t ldv, int n0, int m,
                                                                double* __restrict__ partial) {
  __shared__ double ch[SC_CH * SC_P];
  const int ti = threadIdx.x & 15, tj = threadIdx.x >> 4;
  const int r0 = blockIdx.x * SC_SLAB, r1 = min(n0, r0 + SC_SLAB);
  double acc[8][8];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[a][c] = 0.0;
  for (int rr = r0; rr < r1; rr += SC_CH) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < SC_CH * AS_NB; idx += 256) {
      const int t = idx & (SC_CH - 1), c = idx >> 4;
      ch[t * SC_P + c] = (rr + t < r1 && c < m) ? V[(size_t)(rr + t) + (size_t)c * ldv] : 0.0;
    }
    __syncthreads();
    if (ti > tj) continue;  // a micro-tile wholly below the diagonal
    for (int t = 0; t < SC_CH; ++t) {
      double a[8], c[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a[e] = ch[t * SC_P + 8 * ti + e];
        c[e] = ch[t * SC_P + 8 * tj + e];
      }
#pragma unroll
      for (int x = 0; x < 8; ++x)
#pragma unroll
        for (int z = 0; z < 8; ++z) acc[x][z] = fma(a[x], c[z], acc[x][z]);
    }
  }
  if (ti > tj) return;
  double* out = partial + (size_t)blockIdx.x * AS_NB * AS_NB;
#pragma unroll
  for (int x = 0; x < 8; ++x)
#pragma unroll
    for (int z = 0; z < 8; ++z) {
      const int i = 8 * ti + x, j = 8 * tj + z;
      if (i <= j && j < m) out[i + j * AS_NB] = acc[x][z];
    }
}

// S[i, j] -= sum_s partial[s][i, j] for i <= j < m, the slabs in index order
__global__ __launch_bounds__(256) void append_schur_reduce_kernel(const double* __restrict__ partial,
                                                                  int nslab, int m,
                                                                  double* __restrict__ S, size_t lds) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int i = idx & (AS_NB - 1), j = idx >> 7;
  if (j >= m || i > j) return;
  double s = 0.0;
  for (int t = 0; t < nslab; ++t) s += partial[(size_t)t * AS_NB * AS_NB + i + j * AS_NB];
  S[(size_t)i + (size_t)j * lds] -= s;
}

// a <- R^{-1} R^{-T} a for the m <= 128 entries a of column blockIdx.x, W = R^{-1} (upper, ld 128)
__global__ __launch_bounds__(AS_NB) void append_tail_solve_kernel(const double* __restrict__ W, int m,
                                                                  double* __restrict__ a, size_t lda) {
  __shared__ double c[AS_NB], t[AS_NB];
  const int i = threadIdx.x;
  double* col = a + (size_t)blockIdx.x * lda;
  c[i] = i < m ? col[i] : 0.0;
  __syncthreads();
  double s = 0.0;
  if (i < m)
    for (int k = 0; k <= i; ++k) s = fma(W[k + i * AS_NB], c[k], s);
  t[i] = s;
  __syncthreads();
  if (i >= m) return;
  s = 0.0;
  for (int k = i; k < m; ++k) s = fma(W[i + k * AS_NB], t[k], s);
  col[i] = s;
}

// out[i, r] = sum_j V[i, j] a[j, r] for i < n0 (thread per row, j in order)
__global__ __launch_bounds__(256) void append_vtail_kernel(const double* __restrict__ V, size_t ldv,
                                                           int n0, int m, const double* __restrict__ a,
                                                           double* __restrict__ out, size_t ldo) {
  const int i = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  if (i >= n0) return;
  const double* ar = a + (size_t)r * ldo;
  double s = 0.0;
  for (int j = 0; j < m; ++j) s = fma(V[(size_t)i + (size_t)j * ldv], ar[j], s);
  out[(size_t)i + (size_t)r * ldo] = s;
}

// out[i, r] = alpha0[i, r] - out[i, r] for i < n0
__global__ __launch_bounds__(256) void append_head_kernel(const double* __restrict__ alpha0, int n0,
                                                          double* __restrict__ out, size_t ldo) {
  const int i = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
  if (i >= n0) return;
  double* p = out + (size_t)i + (size_t)r * ldo;
  *p = alpha0[(size_t)i + (size_t)r * n0] - *p;
}

// V = U^{-T} B in place (B n0 x m, ld ldb) by the single-launch sweep, 16 columns per launch
int append_sweep(gpr_ctx* ctx, const double* dU, int n0, int ldu, double* B, int m, int ldb) {
  const int nblk = (n0 + AS_NB - 1) / AS_NB;
  GPR_TRY(ensure_buf(ctx, ctx->dahand, (size_t)nblk * AS_BLK));
  int* sync = ctx->dinfo + INFO_SKINNY;
  const bool vec = ((uintptr_t)dU % 16) == 0 && (ldu % 2) == 0;
  for (int g0 = 0; g0 < m; g0 += AS_NC) {
    const int nc = std::min(AS_NC, m - g0);
    double* Bg = B + (size_t)g0 * ldb;
    HIP_TRY(ctx, hipMemsetAsync(sync, 0, INFO_SKINNY_N * sizeof(int), ctx->stream));
    if (vec)
      append_fwd_sweep_kernel<true><<<nblk, AS_THREADS, 0, ctx->stream>>>(
          dU, (size_t)ldu, n0, ctx->winv, Bg, (size_t)ldb, nc, ctx->dahand, sync);
    else
      append_fwd_sweep_kernel<false><<<nblk, AS_THREADS, 0, ctx->stream>>>(
          dU, (size_t)ldu, n0, ctx->winv, Bg, (size_t)ldb, nc, ctx->dahand, sync);
    LAUNCH_CHECK(ctx);
  }
  return 0;
}

}  // namespace

extern "C" {

int gpr_fit_append(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                   const double* dX, int n0, int m, const double* dy, int nrhs, int ldy,
                   double eps, double* dK, int ldk, const double* dalpha0, double* dalpha,
                   int* info) {
  KParams kp;
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, eps, &kp, nullptr));
  if (n0 < 1) return set_err(ctx, GPR_E_ARG, "n0=%d (needs n0 >= 1)", n0);
  if (m < 1) return set_err(ctx, GPR_E_ARG, "m=%d (needs m >= 1)", m);
  if ((long long)n0 + m > 2147483647LL) return set_err(ctx, GPR_E_ARG, "n0 + m overflows");
  const int N = n0 + m;
  if (nrhs < 1) return set_err(ctx, GPR_E_ARG, "nrhs=%d (needs nrhs >= 1)", nrhs);
  if (ldk < N) return set_err(ctx, GPR_E_ARG, "ldk=%d < n0 + m=%d", ldk, N);
  if (ldy < N) return set_err(ctx, GPR_E_ARG, "ldy=%d < n0 + m=%d", ldy, N);
  if (!dX || !dy || !dK || !dalpha0 || !dalpha)
    return set_err(ctx, GPR_E_ARG, "%s is NULL",
                   !dX ? "dX" : !dy ? "dy" : !dK ? "dK" : !dalpha0 ? "dalpha0" : "dalpha");
  if (dalpha == dalpha0) return set_err(ctx, GPR_E_ARG, "dalpha must be distinct from dalpha0");
  if (info) *info = 0;
  const int nb = ctx->nb;
  const bool small = m <= AS_NB && nb == AS_NB;  // S by the diagonal-block kernel
  // GPR_APPEND_SWEEP auto: the sweep where it measured faster than the GEMM-based route
  // (bench_append.py, profiles/r15_bench_append.json; n0 = 32768 - m, ms per solve, sweep vs
  // gpr_trsm_upper_trans): m = 1 1.78 vs 10.40, 16 2.36 vs 8.99, 32 4.70 vs 9.06, 48 7.05 vs 9.10,
  // 64 9.39 vs 9.18, 128 18.61 vs 9.28 -- one pass over U per 16 columns against a cost that
  // hardly moves with m
  constexpr int AS_AUTO_MAX_M = 48;
  const bool sweep =
      small && (ctx->append_sweep > 0 || (ctx->append_sweep < 0 && m <= AS_AUTO_MAX_M));
  hipStream_t st = ctx->stream;
  ctx->ls = st;

  // the block inverses of the old factor, in a winv that already has room for the new blocks (a
  // regrown one has lost its contents: the inverses are then computed afresh)
  if (ctx->winv.cap < (size_t)((N + nb - 1) / nb) * nb * nb) {
    ctx->fc.factor_forget_blocks();
    GPR_TRY(ensure_winv(ctx, N + N / 8, nb));
  }
  GPR_TRY(ensure_factor_inverses(ctx, dK, n0, ldk));

  // 1. the cross block, the new diagonal block (GPR_SELF form) and the strict-lower rows
  double* Kc = dK + (size_t)n0 * ldk;  // n0 x m, then V
  double* Kn = Kc + n0;                // m x m, then S, then R above its diagonal
  const double* Xn = dX + (size_t)d * n0;
  GPR_TRY(launch_kernel_matrix(ctx, kp, dX, n0, Xn, m, GPR_CROSS, Kc, ldk));
  GPR_TRY(launch_kernel_matrix(ctx, kp, Xn, m, nullptr, m, GPR_SELF, Kn, ldk));
  {
    TimerScope ts(ctx, TC_OTHER, 0.0);
    append_lower_rows_kernel<<<dim3((n0 + 31) / 32, (m + 31) / 32), 256, 0, st>>>(dK, (size_t)ldk,
                                                                                n0, m);
    LAUNCH_CHECK(ctx);
    // 2. c = y_new - K(x_new, x) alpha0, into the tail of dalpha
    append_mean_rhs_kernel<<<dim3(m, nrhs), 256, 0, st>>>(dK, (size_t)ldk, n0, dalpha0, dy,
                                                          (size_t)ldy, dalpha, (size_t)N);
    LAUNCH_CHECK(ctx);
  }
  // 3. V = U^{-T} K(x, x_new)
  {
    TimerScope ts(ctx, TC_APPEND_SOLVE, (double)n0 * n0 * m);
    if (sweep)
      GPR_TRY(append_sweep(ctx, dK, n0, ldk, Kc, m, ldk));
    else
      GPR_TRY(trsm_ut_core(ctx, dK, n0, ldk, Kc, m, ldk, nullptr, 0));
  }
  // 4. + 5. S = K_new - V^T V (upper) and its factor, in place
  int hinfo = 0;
  double* Winv = nullptr;  // R^{-1} of a small append
  if (small) {
    const int nslab = (n0 + SC_SLAB - 1) / SC_SLAB;
    GPR_TRY(ensure_buf(ctx, ctx->dscratch, (size_t)(nslab + 1) * AS_NB * AS_NB));
    Winv = ctx->dscratch;
    double* partial = Winv + AS_NB * AS_NB;
    {
      TimerScope ts(ctx, TC_OTHER, 0.0);
      append_schur_slab_kernel<<<nslab, 256, 0, st>>>(Kc, (size_t)ldk, n0, m, partial);
      LAUNCH_CHECK(ctx);
      append_schur_reduce_kernel<<<(AS_NB * m + 255) / 256, 256, 0, st>>>(partial, nslab, m, Kn,
                                                                         (size_t)ldk);
      LAUNCH_CHECK(ctx);
    }
    GPR_TRY(info_clear(ctx, st));
    GPR_TRY(diag_factor_block(ctx, dK, ldk, N, n0, Winv));  // (a failing pivot: n0 + its order)
    GPR_TRY(info_read(ctx, st, &hinfo));
  } else {
    GPR_TRY(launch_gemm_tn(ctx, syrk_upper_args(Kc, ldk, Kn, ldk, m, n0, -1.0, 1.0), TC_OTHER));
    // (the context's factor cache now describes the sub-block; re-established below)
    GPR_TRY(potrf_core(ctx, Kn, m, ldk, &hinfo));
    if (hinfo > 0) hinfo += n0;
  }
  if (hinfo != 0) {
    if (!small) ctx->fc.factor_forget();
    if (info) *info = hinfo;
    return hinfo;
  }
  // 6. alpha_tail = S^{-1} c, alpha_head = alpha0 - U^{-1} (V alpha_tail)
  double* atail = dalpha + n0;
  if (small) {
    TimerScope ts(ctx, TC_OTHER, 0.0);
    append_tail_solve_kernel<<<nrhs, AS_NB, 0, st>>>(Winv, m, atail, (size_t)N);
    LAUNCH_CHECK(ctx);
  } else {
    GPR_TRY(potrs_core(ctx, Kn, m, ldk, atail, nrhs, N));
  }
  {
    TimerScope ts(ctx, TC_OTHER, 0.0);
    append_vtail_kernel<<<dim3((n0 + 255) / 256, nrhs), 256, 0, st>>>(Kc, (size_t)ldk, n0, m, atail,
                                                                     dalpha, (size_t)N);
    LAUNCH_CHECK(ctx);
  }
  GPR_TRY(potrs_core(ctx, dK, n0, ldk, dalpha, nrhs, N, /*forward=*/false));
  {
    TimerScope ts(ctx, TC_OTHER, 0.0);
    append_head_kernel<<<dim3((n0 + 255) / 256, nrhs), 256, 0, st>>>(dalpha0, n0, dalpha, (size_t)N);
    LAUNCH_CHECK(ctx);
  }
  // the factor cache, extended: the block that straddles n0 and the new ones (potrs_core left
  // the cache on (dK, n0, ldk))
  GPR_TRY(info_clear(ctx, st));
  GPR_TRY(diag_inverse_blocks(ctx, dK, ldk, N, n0 / nb));
  ctx->fc.factor_extend(N);
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"
