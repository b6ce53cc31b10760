// Random-feature prior functions on gfx950: Out (n x ns) = Phi(X) W, the feature matrix Phi
// evaluated tile by tile in registers and never stored (pathwise posterior sampling: the prior
// half of Matheron's rule; the update half is a posterior mean, gpr_kernel_matmul's).
//
//   t_pj(x) = sum_k Omega_p[j, k] l_pk x_k,
//   Out[i, c] = sum_p (sigma_p / sqrt(F)) sum_j (A_p[j, c] cos(2 pi t_pj(x_i)) + B_p[j, c] sin(2 pi t_pj(x_i)))
// for the stationary parts p (SquaredExp, Matern-3/2, Matern-5/2) of a description, F = nfreq
// frequencies per part, W = [A_0; B_0; A_1; B_1; ...] (2 nse F rows).  gpr_rff_draw fills Omega from
// gpr_randn's stream so that (1/F) sum_j cos(2 pi (t_j(x) - t_j(x'))) -> k_p(x, x') / sigma_p^2; the
// 1 / (2 pi) sits in Omega, so that the angle's reduction is t - rint(t), exact in FP64.
//
// Three stages per 64-frequency x 64-point tile, the shape of kmatmul.hip with another middle:
//   projection  T = Omega_p (l_p o X)^T by v_mfma_f64_16x16x4 over k = d.  Both operands are
//     prepared once per call in the order the MFMA reads them (rff_prep_kernel: [part][16-block]
//     [k-step][lane], lane l <-> (index 16 blk + (l & 15), dimension 4 s + (l >> 4)), zeros past d,
//     n or F), so an operand is one coalesced 512-B wave load.  Frequencies are the A operand (the
//     tile's rows), points the B operand (its columns): register q of a 16 x 16 block in lane l is
//     T[freq 4 q + (l >> 4), point l & 15] -- and v_mfma's B operand is B[k = l >> 4][n = l & 15],
//     so that register is, as it stands, k-step q of the second product.  T never touches LDS.
//     k-steps compiled in for d <= 8, walked at run time above.
//   sincos  r = t - rint(t), then rff_sincos2pi (rff_sincos.hpp): both functions from one octant
//     reduction and two degree-8 polynomials, on the VALU.  This is what bounds the kernel.
//   product  Out^T[c, point] += A_p^T[c, freq] C[freq, point] + B_p^T[c, freq] S[freq, point]: the
//     A operand A[m = l & 15][k = l >> 4] = W[freq 4 q + (l >> 4), column 16 vb + (l & 15)] comes from
//     the weight blocks staged in LDS column by column (stride KMM_VS = 66 doubles: a half wave's
//     read touches distinct banks), the cos block then the sin block.  sigma_p / sqrt(F) (one
//     rounding from long double on the host) is folded into the weights as they are staged: one
//     product per weight, not one per part and accumulator.  C and S of one row block (2 x 4
//     registers each) are consumed right after they are formed: the NVB = 4 instances hold 32
//     accumulators, 16 prefetched weight pairs and 16 + 16 doubles of C and S.
//
// Work split.  A workgroup of 4 waves owns 64 points and one slab of the (part, 64-frequency block)
// list of the launch; wave w evaluates the quadrant (frequencies 32 (w & 1), points 32 (w >> 1)) and
// keeps Out^T accumulators (16 NVB columns x 32 points, NVB = 1 for ns <= 16, else 4) over the whole
// slab; the two waves that share points add once at the end through LDS.  The next block's weights
// are fetched into registers before the tile is evaluated and staged after the product (one block
// ahead, the fetch under the sincos).  Grid (ceil(n / 64), S): GPR_RFF_SLABS, else the fewest
// slabs that give two workgroups per CU (1 from n = 32768 on 256 CUs); with S > 1 the slabs write
// partials to ctx->dkmm and kmm_reduce_slabs adds them in slab order.  No atomics: two calls agree
// bit for bit.  Rows >= n and frequencies >= F enter as exact zeros of the operands and weights.
// Wider W repeats the pass per 64 columns; more than RFF_MAXP parts: one launch per group, adding.
//
// Memory: the prepared operands (ctx->drff: 4 ceil(d / 4) nse (n + F) doubles, padded to 64) and
// S n min(ns, 64) doubles of partials when S > 1 -- linear in n + F; nothing is sized by n F.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "kmm_vstage.hpp"
#include "randn.hpp"
#include "rff_sincos.hpp"

namespace {

constexpr int RFF_MAXP = 8;  // parts of one launch (their scales travel as kernel arguments)
struct RffScale {
  double s[RFF_MAXP];  // sigma_p / sqrt(F)
};

// ---- the draw ---------------------------------------------------------------------------------
// Element (part p, frequency j, dimension k) reads gpr_randn's stream of `seed` at
//   g = p 2^56 + j 2^24 + k                      (the direction z_k, k < d), and
//   g = p 2^56 + j 2^24 + RFF_CHI + i, i < nu    (the chi-square sum of a Matern part, nu = 3 or 5)
// -- a function of (seed, p, j, k) alone, whatever nfreq is.
constexpr uint64_t RFF_CHI = (1ull << 24) - 8;
constexpr double RFF_INV_2PI = 0.15915494309189533577;

__global__ __launch_bounds__(256) void rff_draw_kernel(uint64_t seed, int part, int prof, int d,
                                                       int nfreq, double* __restrict__ Om) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nfreq) return;
  const uint64_t base = ((uint64_t)part << 56) | ((uint64_t)j << 24);
  double scale = 1.4142135623730951 * RFF_INV_2PI;  // SE: k = exp(-D), omega ~ N(0, 2 I)
  double e, o;
  if (prof != KPROF_SE) {  // Matern nu/2: omega = z sqrt(nu / g), g ~ chi^2_nu
    const int nu = prof == KPROF_M32 ? 3 : 5;
    double g = 0.0;
    for (int i = 0; i < nu; i += 2) {
      randn_pair(seed, (base + RFF_CHI + i) >> 1, e, o);
      g = fma(e, e, g);
      if (i + 1 < nu) g = fma(o, o, g);
    }
    scale = sqrt((double)nu / g) * RFF_INV_2PI;
  }
  for (int k = 0; k < d; k += 2) {
    randn_pair(seed, (base + k) >> 1, e, o);
    Om[j + (size_t)k * nfreq] = scale * e;
    if (k + 1 < d) Om[j + (size_t)(k + 1) * nfreq] = scale * o;
  }
}

// ---- operand preparation ----------------------------------------------------------------------
// out[p][blk][s][lane] = v_p(16 blk + (lane & 15), 4 s + (lane >> 4)), 0 past cnt or d.
//   l != null (points):      v_p(a, k) = l[p][k] * src[k + a d]   (one rounding)
//   l == null (frequencies): v_p(j, k) = src[p][j + k cnt]        (Omega as drawn)
__global__ __launch_bounds__(256) void rff_prep_kernel(const double* __restrict__ src,
                                                       const double* __restrict__ l, int cnt, int d,
                                                       int S, int nblk, int nse,
                                                       double* __restrict__ out) {
  const size_t total = (size_t)nse * nblk * S * 64;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total;
       t += (size_t)gridDim.x * blockDim.x) {
    const int lane = (int)(t & 63);
    const size_t r = t >> 6;
    const int s = (int)(r % S);
    const size_t r2 = r / S;
    const int blk = (int)(r2 % nblk), p = (int)(r2 / nblk);
    const int a = blk * 16 + (lane & 15), k = 4 * s + (lane >> 4);
    double v = 0.0;
    if (a < cnt && k < d)
      v = l ? l[(size_t)p * d + k] * src[(size_t)a * d + k]
            : src[((size_t)p * d + k) * cnt + a];
    out[t] = v;
  }
}

// ---- the product ------------------------------------------------------------------------------
// xop / oop: the prepared points / frequencies of the launch's parts (nbx / 4 nfb 16-blocks per
// part); the launch's (part, frequency block) list has nblocks = parts x nfb entries, slab y walks
// [y slab_blocks, ..).  W: the launch's first part's cos block.  Out: this pass's columns; slab y
// writes at Out + y slab_stride; accum: the result is added to what Out holds.
template <int SC, int NVB>
__global__ __launch_bounds__(256, 2) void rff_matmul_kernel(
    RffScale sc, int Srt, const double* __restrict__ xop, const double* __restrict__ oop, int nbx,
    int nfb, int nblocks, int slab_blocks, int n, int nfreq, const double* __restrict__ W,
    size_t ldw, int nvc, int vec, double* __restrict__ Out, size_t ldo, size_t slab_stride,
    int accum) {
  extern __shared__ double dyn_lds[];
  double* Wc = dyn_lds;                  // cos weights: 16 NVB columns x KMM_VS
  double* Wn = Wc + 16 * NVB * KMM_VS;   // sin weights
  const int S = SC > 0 ? SC : Srt;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wr = w & 1, wc = w >> 1;
  const int i0 = blockIdx.x * KT;
  const int g_lo = blockIdx.y * slab_blocks;
  const int g_hi = min(g_lo + slab_blocks, nblocks);
  gd4 acc[NVB][2];
#pragma unroll
  for (int vb = 0; vb < NVB; ++vb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) acc[vb][cb] = gd4{0.0, 0.0, 0.0, 0.0};
  kv2 vc[2 * NVB], vs[2 * NVB];
  auto fetch = [&](int g) {
    const int p = g / nfb, fb = g - p * nfb;
    const double* Wp = W + (size_t)2 * p * nfreq;
    kmm_fetch_v<NVB>(Wp, ldw, nfreq, nvc, fb * KT, vec, vc);
    kmm_fetch_v<NVB>(Wp + nfreq, ldw, nfreq, nvc, fb * KT, vec, vs);
  };
  auto stage = [&](int g) {  // scaled by sigma_p / sqrt(F) on the way in
    const int p = g / nfb;
    double s = sc.s[0];
#pragma unroll
    for (int q = 1; q < RFF_MAXP; ++q) s = p == q ? sc.s[q] : s;
    const int pr = threadIdx.x & 31, cg = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 2 * NVB; ++k) {
      *reinterpret_cast<kv2*>(Wc + (cg + 8 * k) * KMM_VS + 2 * pr) = vc[k] * s;
      *reinterpret_cast<kv2*>(Wn + (cg + 8 * k) * KMM_VS + 2 * pr) = vs[k] * s;
    }
  };
  fetch(g_lo);
  stage(g_lo);
  __syncthreads();
  for (int g = g_lo; g < g_hi; ++g) {
    const int p = g / nfb, fb = g - p * nfb;
    const bool more = g + 1 < g_hi;
    if (more) fetch(g + 1);  // lands under the sincos
    // block cb of the wave's points: + cb S 64; block rb of its frequencies: + rb S 64
    const double* xo = xop + ((size_t)p * nbx + (i0 >> 4) + 2 * wc) * S * 64 + lane;
    const double* oo = oop + ((size_t)p * 4 * nfb + 4 * fb + 2 * wr) * S * 64 + lane;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      gd4 t[2] = {gd4{0.0, 0.0, 0.0, 0.0}, gd4{0.0, 0.0, 0.0, 0.0}};
      if constexpr (SC > 0) {
#pragma unroll
        for (int s = 0; s < SC; ++s) {
          const double a = oo[(rb * SC + s) * 64];
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
            t[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xo[(cb * SC + s) * 64], t[cb], 0, 0, 0);
        }
      } else {
        for (int s = 0; s < S; ++s) {
          const double a = oo[(size_t)(rb * S + s) * 64];
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
            t[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xo[(size_t)(cb * S + s) * 64], t[cb],
                                                         0, 0, 0);
        }
      }
      gd4 cs[2], sn[2];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          double s1, c1;
          rff_sincos2pi(t[cb][q] - __builtin_rint(t[cb][q]), s1, c1);
          sn[cb][q] = s1;
          cs[cb][q] = c1;
        }
      // Out^T += A^T C + B^T S: register q of block (rb, cb) is k-step q's B operand
      const double* wa = Wc + (lane & 15) * KMM_VS + 32 * wr + 16 * rb + (lane >> 4);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int vb = 0; vb < NVB; ++vb) {
          const double ac = wa[16 * vb * KMM_VS + 4 * q];
          const double as = wa[16 * (NVB + vb) * KMM_VS + 4 * q];
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) {
            acc[vb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac, cs[cb][q], acc[vb][cb], 0, 0, 0);
            acc[vb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(as, sn[cb][q], acc[vb][cb], 0, 0, 0);
          }
        }
    }
    __syncthreads();  // the block's weights are read
    if (more) stage(g + 1);
    __syncthreads();
  }
  // the two frequency halves' sums of a point half: wave (1, wc) hands its accumulators to (0, wc)
  double* red = Wc + wc * (NVB * 8 * 64) + lane;  // 1024 NVB doubles of the 2112 NVB
  if (wr == 1) {
#pragma unroll
    for (int vb = 0; vb < NVB; ++vb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[((vb * 2 + cb) * 4 + q) * 64] = acc[vb][cb][q];
  }
  __syncthreads();
  if (wr == 0) {
    double* O = Out + (size_t)blockIdx.y * slab_stride;
#pragma unroll
    for (int vb = 0; vb < NVB; ++vb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i0 + 32 * wc + 16 * cb + (lane & 15);
          const int c = 16 * vb + (lane >> 4) + 4 * q;
          if (i < n && c < nvc) {
            double* dst = O + (size_t)c * ldo + i;
            double s = acc[vb][cb][q] + red[((vb * 2 + cb) * 4 + q) * 64];
            if (accum) s = *dst + s;
            *dst = s;
          }
        }
  }
}

struct RffOps {
  const double *xop, *oop;  // prepared points / frequencies of all parts
  int S, nbx, nfb, n, nfreq;
};

// one pass: columns [0, nvc <= 64) of W, parts [p0, p0 + cnt) of the description
template <int SC, int NVB>
int rff_launch(gpr_ctx* ctx, const RffOps& o, const RffScale& sc, int p0, int cnt, const double* W,
               int ldw, int nvc, double* Out, int ldo, int accum) {
  const int nta = (o.n + KT - 1) / KT, nblocks = cnt * o.nfb;
  const int ncu = ctx->ncu > 0 ? ctx->ncu : 256;
  int slabs = ctx->rff_slabs > 0 ? ctx->rff_slabs : (2 * ncu + nta - 1) / nta;
  slabs = std::max(1, std::min(slabs, std::min(nblocks, KMM_MAXS)));
  const int slab_blocks = (nblocks + slabs - 1) / slabs;
  slabs = (nblocks + slab_blocks - 1) / slab_blocks;  // (no empty slab)
  double* dst = Out;
  size_t ldd = (size_t)ldo, stride = 0;
  if (slabs > 1) {
    GPR_TRY(ensure_buf(ctx, ctx->dkmm, (size_t)slabs * o.n * nvc));
    dst = ctx->dkmm;
    ldd = (size_t)o.n;
    stride = (size_t)o.n * nvc;
  }
  const double* Wp = W + (size_t)2 * p0 * o.nfreq;
  const int vec = ((uintptr_t)Wp & 15) == 0 && (ldw & 1) == 0 && (o.nfreq & 1) == 0;
  const size_t lds = sizeof(double) * 2 * 16 * NVB * KMM_VS;
  auto* kern = &rff_matmul_kernel<SC, NVB>;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return set_err(ctx, GPR_E_HIP, "gpr_rff_matmul: %zu bytes of LDS refused", lds);
  kern<<<dim3((unsigned)nta, (unsigned)slabs), 256, lds, ctx->stream>>>(
      sc, o.S, o.xop + (size_t)p0 * o.nbx * o.S * 64, o.oop + (size_t)p0 * 4 * o.nfb * o.S * 64,
      o.nbx, o.nfb, nblocks, slab_blocks, o.n, o.nfreq, Wp, (size_t)ldw, nvc, vec, dst, ldd, stride,
      slabs > 1 ? 0 : accum);
  LAUNCH_CHECK(ctx);
  if (slabs > 1) GPR_TRY(kmm_reduce_slabs(ctx, slabs, o.n, nvc, Out, ldo, accum));
  return 0;
}

template <int SC>
int rff_launch_nv(gpr_ctx* ctx, const RffOps& o, const RffScale& sc, int p0, int cnt,
                  const double* W, int ldw, int nvc, double* Out, int ldo, int accum) {
  return nvc <= 16 ? rff_launch<SC, 1>(ctx, o, sc, p0, cnt, W, ldw, nvc, Out, ldo, accum)
                   : rff_launch<SC, 4>(ctx, o, sc, p0, cnt, W, ldw, nvc, Out, ldo, accum);
}

// the stationary parts a random-feature prior exists for; a Periodic part (a line spectrum) or a
// product marker (a convolution of spectra): GPR_E_UNSUP, naming it.  *nse: the parts counted.
int rff_check_kinds(gpr_ctx* ctx, const char* what, const int* kinds, int nk, int* nse) {
  if (!kinds || nk <= 0) return set_err(ctx, GPR_E_ARG, "%s: bad kinds/nk (%d)", what, nk);
  *nse = 0;
  for (int i = 0; i < nk; ++i) {
    if (kinds[i] == GPR_PER || kinds[i] == GPR_MUL)
      return set_err(ctx, GPR_E_UNSUP, "%s takes sums of SquaredExp, Matern and WhiteNoise parts: "
                                       "part %d is %s", what, i + 1, kind_name(kinds[i]));
    if (kind_stationary(kinds[i])) ++*nse;
    else if (kinds[i] != GPR_WN) return set_err(ctx, GPR_E_ARG, "unknown kernel kind %d", kinds[i]);
  }
  if (*nse == 0)
    return set_err(ctx, GPR_E_ARG, "%s: the description has no stationary part", what);
  return 0;
}

}  // namespace

extern "C" {

int gpr_rff_draw(gpr_ctx_t ctx, const int* kinds, int nk, int d, int nfreq, uint64_t seed,
                 double* dOmega) {
  if (!ctx) return GPR_E_ARG;
  int nse = 0;
  GPR_TRY(rff_check_kinds(ctx, "gpr_rff_draw", kinds, nk, &nse));
  if (!dOmega) return set_err(ctx, GPR_E_ARG, "gpr_rff_draw: dOmega is NULL");
  if (d < 1 || (uint64_t)d > RFF_CHI) return set_err(ctx, GPR_E_ARG, "gpr_rff_draw: d=%d", d);
  if (nfreq < 1) return set_err(ctx, GPR_E_ARG, "gpr_rff_draw: nfreq=%d < 1", nfreq);
  if (nse > 256)
    return set_err(ctx, GPR_E_UNSUP, "gpr_rff_draw: %d stationary parts (the stream map has 256)",
                   nse);
  for (int i = 0, p = 0; i < nk; ++i) {
    if (!kind_stationary(kinds[i])) continue;
    rff_draw_kernel<<<(nfreq + 255) / 256, 256, 0, ctx->stream>>>(
        seed, p, kind_profile(kinds[i]), d, nfreq, dOmega + (size_t)p * nfreq * d);
    ++p;
  }
  LAUNCH_CHECK(ctx);
  return 0;
}

int gpr_rff_matmul(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                   const double* dX, int n, const double* dOmega, int nfreq, const double* dW,
                   int ns, int ldw, double* dOut, int ldo) {
  if (!ctx) return GPR_E_ARG;
  int nse = 0;
  GPR_TRY(rff_check_kinds(ctx, "gpr_rff_matmul", kinds, nk, &nse));
  if (!dX) return set_err(ctx, GPR_E_ARG, "gpr_rff_matmul: dX is NULL");
  if (!dOmega) return set_err(ctx, GPR_E_ARG, "gpr_rff_matmul: dOmega is NULL");
  if (!dW) return set_err(ctx, GPR_E_ARG, "gpr_rff_matmul: dW is NULL");
  if (!dOut) return set_err(ctx, GPR_E_ARG, "gpr_rff_matmul: dOut is NULL");
  if (n < 1) return set_err(ctx, GPR_E_ARG, "gpr_rff_matmul: n=%d < 1", n);
  if (nfreq < 1) return set_err(ctx, GPR_E_ARG, "gpr_rff_matmul: nfreq=%d < 1", nfreq);
  if (ns < 1) return set_err(ctx, GPR_E_ARG, "gpr_rff_matmul: ns=%d < 1", ns);
  if ((long long)ldw < 2ll * nse * nfreq)
    return set_err(ctx, GPR_E_ARG, "gpr_rff_matmul: ldw=%d < 2 x %d parts x nfreq=%d", ldw, nse,
                   nfreq);
  if (ldo < n) return set_err(ctx, GPR_E_ARG, "gpr_rff_matmul: ldo=%d < n=%d", ldo, n);
  KParams kp;
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, 0.0, &kp, nullptr));
  const int S = (d + 3) / 4;
  const int nbx = ((n + KT - 1) / KT) * (KT / 16), nfb = (nfreq + KT - 1) / KT;
  const size_t opx = (size_t)nse * nbx * S * 64, opo = (size_t)nse * 4 * nfb * S * 64;
  GPR_TRY(ensure_buf(ctx, ctx->drff, opx + opo));
  double* xop = ctx->drff;
  double* oop = xop + opx;
  const int bx = (int)std::min<size_t>((opx + 255) / 256, 8192);
  const int bo = (int)std::min<size_t>((opo + 255) / 256, 8192);
  rff_prep_kernel<<<bx, 256, 0, ctx->stream>>>(dX, kp.l, n, d, S, nbx, nse, xop);
  rff_prep_kernel<<<bo, 256, 0, ctx->stream>>>(dOmega, nullptr, nfreq, d, S, 4 * nfb, nse, oop);
  LAUNCH_CHECK(ctx);
  const RffOps o{xop, oop, S, nbx, nfb, n, nfreq};
  const long double rf = sqrtl((long double)nfreq);
  for (int c0 = 0; c0 < ns; c0 += 64) {
    const int nvc = std::min(64, ns - c0);
    const double* W = dW + (size_t)c0 * ldw;
    double* Out = dOut + (size_t)c0 * ldo;
    for (int p0 = 0; p0 < nse; p0 += RFF_MAXP) {
      const int cnt = std::min(RFF_MAXP, nse - p0);
      RffScale sc{};
      for (int p = 0; p < cnt; ++p) sc.s[p] = (double)((long double)kp_sigma(kp, p0 + p) / rf);
      const int accum = p0 > 0;
      // k-steps compiled in for d <= 8, walked at run time above
      if (S == 1) GPR_TRY((rff_launch_nv<1>(ctx, o, sc, p0, cnt, W, ldw, nvc, Out, ldo, accum)));
      else if (S == 2) GPR_TRY((rff_launch_nv<2>(ctx, o, sc, p0, cnt, W, ldw, nvc, Out, ldo, accum)));
      else GPR_TRY((rff_launch_nv<0>(ctx, o, sc, p0, cnt, W, ldw, nvc, Out, ldo, accum)));
    }
  }
  return 0;
}

}  // extern "C"
