// The Gram-form tile of the kernel matrix and its prepared operands, shared by the K assembly
// (assembly.hip) and the matrix-free product (kmatmul.hip): every caller evaluates the same
// element code, so an element is bit for bit the same wherever it is formed.
#pragma once
#include <algorithm>

#include "common.hpp"
#include "kexp.hpp"

namespace {

constexpr int KT = 64;  // output tile edge

// per-part exp tables s2_p * 2^(j/256) into LDS (256 threads)
__device__ __forceinline__ void load_part_tables(const KParams& kp, double* tabs) {
#if GPR_EXP32
  const double T = kp.exptab[(threadIdx.x & 31) << 3];  // compact 2^(j/32) tables
#else
  const double T = kp.exptab[threadIdx.x];
#endif
  for (int p = 0; p < kp.nse; ++p) tabs[256 * p + threadIdx.x] = (kp.sigma[p] * kp.sigma[p]) * T;
}

// ---- Gram form of the distance on FP64 MFMA ---------------------------------------------
// -D_ab = (-|y_a|^2 - |y_b|^2) + sum_k (2 y_a,k) y_b,k with y = x .* l - c, where c is the mean of
// (a bounded sample of) the part's scaled training points (distances are translation invariant; centring keeps |y|^2,
// the cancelling terms, small).  Per 16 x 16 block the sum is ceil(d/4) v_mfma_f64_16x16x4f64
// started from C = -|y_a|^2 - |y_b|^2 (one VALU add per element), so the FP64 VALU is left with
// exp (kexp_s2) and the part sum.  Rounding: |error of D| <~ (d + 1) u (|y_a|^2 + |y_b|^2),
// ~1e-15 absolute at the default hp (K within rtol 1e-13 of the reference's difference form,
// tests/test_gpu_parity.py; the worst case, (3 d + 4) u (|y_a|^2 + |y_b|^2) on top of the
// difference form's own, is what tests/test_gpu_kernel_domain.py holds the kernels to far from
// the unit cube: DESIGN 3.5.1); a same-object diagonal gets D = 0 exactly and diagonal tiles are
// made bitwise symmetric.  GPR_KBUILD_EXACT=1 selects the reference's difference form
// (x .* l - x' .* l)^2 in kmat_sym2/cross2.
// Measured (tools/kbuild_bench, SE+SE+WN N = 32768 d = 8, same box): difference form 2.43 ms,
// the same Gram sum on the VALU 2.36 ms, MFMA with the norms as a third k-step 2.07 ms.
// Operands are prepared once per call in MFMA lane order: for 16-point block b and k-step s,
// 64 doubles, lane l <-> (point 16 b + (l & 15), k = 4 s + (l >> 4)) -- every operand load is one
// coalesced 512-B wave load; points padded to a multiple of 64 (zeros).
typedef double gd4 __attribute__((ext_vector_type(4)));
#ifndef GRAM_EXPG  // exp evaluations the scheduler may interleave (register pressure)
#define GRAM_EXPG 4
#endif

// grid = nse * d workgroups of 256: c[p][k] = mean over the first min(n, GRAM_CENTER_PTS) points
// of xs[p][.][k] (fixed-order tree sum).  Any centre inside the data's spread serves (it only
// sets the size of |y|^2); a bounded sample keeps this a few microseconds at any n.
constexpr int GRAM_CENTER_PTS = 2048;
__global__ __launch_bounds__(256) void gram_center_kernel(const double* __restrict__ xs, int n,
                                                          int d, double* __restrict__ c) {
  __shared__ double red[256];
  const int p = blockIdx.x / d, k = blockIdx.x % d;
  const int cnt = min(n, GRAM_CENTER_PTS);
  double sum = 0.0;
  for (int a = threadIdx.x; a < cnt; a += 256) sum += xs[((size_t)p * n + a) * d + k];
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) c[p * d + k] = red[0] / (double)cnt;
}

// out[p][blk][s][lane] = scale * y[16 blk + (lane & 15)][4 s + (lane >> 4)] (0 past d or n);
// nrm[p][a] = -|y_a|^2 (0 for padded points)
__global__ void gram_prep_kernel(const double* __restrict__ xs, int n, int d, int S, int nblk,
                                 int nse, const double* __restrict__ c, double scale,
                                 double* __restrict__ out, double* __restrict__ nrm) {
  const size_t total = (size_t)nse * nblk * S * 64;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total;
       t += (size_t)gridDim.x * blockDim.x) {
    const int lane = (int)(t & 63);
    const size_t r = t >> 6;
    const int s = (int)(r % S);
    const size_t r2 = r / S;
    const int blk = (int)(r2 % nblk), p = (int)(r2 / nblk);
    const int a = blk * 16 + (lane & 15), k = 4 * s + (lane >> 4);
    const double* xa = xs + ((size_t)p * n + a) * d;
    const double* cp = c + (size_t)p * d;
    out[t] = (a < n && k < d) ? scale * (xa[k] - cp[k]) : 0.0;
    if (nrm && s == 0 && lane < 16) {
      double q = 0.0;
      if (a < n)
        for (int kk = 0; kk < d; ++kk) {
          const double y = xa[kk] - cp[kk];
          q = fma(y, y, q);
        }
      nrm[(size_t)p * nblk * 16 + a] = -q;
    }
  }
}

// One 64 x 64 tile of K on MFMA + VALU: v += the parts' terms, summed in part order.  Wave w owns
// the 32 x 32 quadrant (rows 32 (w & 1), cols 32 (w >> 1)): 2 x 2 blocks of 16 x 16; lane l /
// register q of block (rb, cb) <-> row 16 rb + (l >> 4) + 4 q, col 16 cb + (l & 15).  Per part the
// four accumulators start from -|y_a|^2 - |y_b|^2, take the S k-steps (k ascending per
// accumulator) and go through the part's profile.  Only the k-steps differ by SC:
//  SC > 0 (S = SC compiled in, d <= 20): all 2 x 2 x S operands in registers, each block's MFMA
//    chain right behind its accumulator's start value;
//  SC = 0 (any d): chunks of GR_CH = 4 k-steps (16 dimensions); a chunk's 2 x 4 row and 2 x 4
//    column operands are 16 coalesced 512-B wave loads, the next chunk's are issued before the
//    current chunk's MFMAs (four independent accumulators per step), and the last chunk is
//    ragged by whole k-steps: steps past S enter as zero operands, which leave every
//    accumulator bit for bit as it was (padding inside a step is already zero in the prepared
//    operands).  96 operand / accumulator registers whatever d is.
// DIAG: a diagonal tile of the symmetric K -- D = 0 exactly and eps per part on i == j,
// sigma_n^2 after the parts.
// PROD: some term is a product -- a part's value is multiplied into its term's running product,
// and the term goes into v (eps once per term) when the part closes it (kp.tendm); PROD = false
// compiles the sum of parts alone.  The running products live in tmw, the caller's tile staging
// buffer (idle while a tile is computed): 16 slots per thread, tmw[16][256], each read and
// written by its own thread only -- held in registers they cost 32 VGPRs and spilled (the full K
// of SE*PER+WN measured 1.83 x SE+PER+WN that way).  The caller puts a barrier between the last
// read of the staging buffer and this call.
constexpr int GR_CH = 4;  // k-steps per chunk
template <int SC, bool DIAG, bool MIX, bool PROD = false>
__device__ __forceinline__ void gram_tile(const KParams& kp, int S, const double* __restrict__ gA,
                                          const double* __restrict__ gB, const double* __restrict__ nA,
                                          const double* __restrict__ nB, int nblkA, int nblkB,
                                          int i0, int j0, const double* tabs, gd4 (&v)[2][2],
                                          double* tmw = nullptr) {
  constexpr int NOP = SC > 0 ? SC : GR_CH;  // k-steps of operands held per 16-block
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wr = w & 1, wc = w >> 1;
  const int ba = (i0 >> 4) + 2 * wr, bb = (j0 >> 4) + 2 * wc;  // first 16-blocks
  for (int p = 0; p < kp.nse; ++p) {
    const bool opens = !PROD || p == 0 || ((kp.tendm >> (p - 1)) & 1);
    const bool closes = !PROD || ((kp.tendm >> p) & 1);
    const double* Ap = gA + ((size_t)p * nblkA + ba) * S * 64 + lane;
    const double* Bp = gB + ((size_t)p * nblkB + bb) * S * 64 + lane;
    const double* nAp = nA + (size_t)p * nblkA * 16 + ba * 16 + (lane >> 4);
    const double* nBp = nB + (size_t)p * nblkB * 16 + bb * 16 + (lane & 15);
    // operands of 16-block h, k-steps NOP ch + [0, NOP) (wave-uniform bound: zero past S)
    auto load_ops = [&](int ch, int h, double (&a)[2][NOP], double (&b)[2][NOP]) {
#pragma unroll
      for (int s = 0; s < NOP; ++s) {
        const int st = NOP * ch + s;
        const bool in = st < S;
        a[h][s] = in ? Ap[((size_t)h * S + st) * 64] : 0.0;
        b[h][s] = in ? Bp[((size_t)h * S + st) * 64] : 0.0;
      }
    };
    // The order of the loads and of the next two loops is deliberate, and is the
    // order each form had as a function of its own.  With S compiled in, the operand loads of
    // half h come before that half's norm loads, and each block's MFMAs follow its start value
    // directly, before the next block's start value; ordered differently the symmetric kernels
    // spill up to ten more VGPRs.  With S at run time the first chunk of both halves is loaded
    // before any norm.
    double a[2][NOP], b[2][NOP], nr[2][4], nc[2];
    if constexpr (SC == 0) {
      load_ops(0, 0, a, b);
      load_ops(0, 1, a, b);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if constexpr (SC > 0) load_ops(0, h, a, b);
#pragma unroll
      for (int q = 0; q < 4; ++q) nr[h][q] = nAp[16 * h + 4 * q];
      nc[h] = nBp[16 * h];
    }
    gd4 acc[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[rb][cb][q] = nr[rb][q] + nc[cb];
        if constexpr (SC > 0) {
#pragma unroll
          for (int s = 0; s < SC; ++s)
            acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rb][s], b[cb][s], acc[rb][cb], 0, 0, 0);
        }
      }
    if constexpr (SC == 0) {
      const int nch = (S + GR_CH - 1) / GR_CH;
      for (int ch = 0; ch < nch; ++ch) {
        double an[2][GR_CH], bn[2][GR_CH];
        if (ch + 1 < nch) {  // in flight behind this chunk's MFMAs
          load_ops(ch + 1, 0, an, bn);
          load_ops(ch + 1, 1, an, bn);
        }
#pragma unroll
        for (int s = 0; s < GR_CH; ++s)
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
              acc[rb][cb] =
                  __builtin_amdgcn_mfma_f64_16x16x4f64(a[rb][s], b[cb][s], acc[rb][cb], 0, 0, 0);
        if (ch + 1 < nch) {
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < GR_CH; ++s) {
              a[h][s] = an[h][s];
              b[h][s] = bn[h][s];
            }
        }
      }
    }
    const double* ts = tabs + 256 * p;
    kprof_dispatch<MIX>(MIX ? kp.prof[p] : 0, [&](auto pf) {
      // (a factor's product and the sum it goes into round separately in every caller: which of
      // them the compiler fuses would otherwise differ from kernel to kernel)
#pragma clang fp contract(off)
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          double x = acc[rb][cb][q];  // -D
          bool on_diag = false;
          if (DIAG) {
            on_diag = wr == wc && rb == cb && (lane >> 4) + 4 * q == (lane & 15);
            if (on_diag) x = 0.0;
          }
          double t = kprof_s2<decltype(pf)::value>(-x, ts);
          if constexpr (PROD) {
            double* slot = tmw + ((rb * 2 + cb) * 4 + q) * 256 + threadIdx.x;
            if (!opens) t *= *slot;
            if (closes) {
              if (DIAG && on_diag) t += kp.eps;
              v[rb][cb][q] += t;
            } else {
              *slot = t;
            }
          } else {
            if (DIAG && on_diag) t += kp.eps;
            v[rb][cb][q] += t;
          }
          if ((q + 1) % GRAM_EXPG == 0) __builtin_amdgcn_sched_barrier(0);
        }
    });
  }
  if (DIAG && kp.has_noise && wr == wc) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if ((lane >> 4) + 4 * q == (lane & 15)) v[rb][rb][q] += kp.noise2;
  }
}

// doubles of the centres' buffer: nse x d, and never below the old fixed 4 x 64 so that no
// call inside that envelope re-allocates it
inline size_t gram_centres_cap(const KParams& kp) {
  return std::max((size_t)kp.nse * kp.d, (size_t)256);
}

// The prepared operands of one Gram build (S k-steps): the centres of the row points, the row
// operands x 2.0 with the row norms, the column operands x 1.0 -- of the same points (same: no
// second set of norms, everything carved from dgA) or of xps with their own norms (dgB).
struct GramOps {
  double *A, *nrmA, *B, *nrmB;
  int nbA, nbB;  // 16-blocks, points padded to a multiple of KT
};
int gram_prepare(gpr_ctx* ctx, const KParams& kp, int S, const double* xs, int n,
                 const double* xps, int m, int same, GramOps* o) {
  const int d = kp.d;
  const int nbA = ((n + KT - 1) / KT) * (KT / 16);
  const int nbB = same ? nbA : ((m + KT - 1) / KT) * (KT / 16);
  const size_t opA = (size_t)kp.nse * nbA * S * 64, opB = same ? 0 : (size_t)kp.nse * nbB * S * 64;
  const size_t nA = (size_t)kp.nse * nbA * 16, nB = same ? 0 : (size_t)kp.nse * nbB * 16;
  GPR_TRY(ensure_buf(ctx, ctx->dgc, gram_centres_cap(kp)));
  GPR_TRY(ensure_buf(ctx, ctx->dgA, opA + nA + (same ? opA : 0)));
  if (!same) GPR_TRY(ensure_buf(ctx, ctx->dgB, opB + nB));
  double* A = ctx->dgA;
  double* nrmA = A + opA;
  double* B = same ? nrmA + nA : ctx->dgB;
  double* nrmB = same ? nrmA : B + opB;
  gram_center_kernel<<<kp.nse * d, 256, 0, ctx->stream>>>(xs, n, d, ctx->dgc);
  auto prep = [&](const double* src, int cnt, int nblk, double scale, double* out, double* nrm) {
    const size_t total = (size_t)kp.nse * nblk * S * 64;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 8192);
    gram_prep_kernel<<<blocks, 256, 0, ctx->stream>>>(src, cnt, d, S, nblk, kp.nse, ctx->dgc,
                                                      scale, out, nrm);
  };
  prep(xs, n, nbA, 2.0, A, nrmA);
  prep(same ? xs : xps, same ? n : m, nbB, 1.0, B, same ? nullptr : nrmB);
  LAUNCH_CHECK(ctx);
  *o = GramOps{A, nrmA, B, nrmB, nbA, nbB};
  return 0;
}

}  // namespace
