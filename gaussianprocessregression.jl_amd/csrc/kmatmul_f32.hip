// The matrix-free product with FP32 kernel evaluation (GPR_KMM_PREC = 1): Out (na x nv, FP64) =
// K~(xa, xb) V, where K~ is the kernel matrix with every stationary part's profile evaluated in
// FP32 -- on the packed FP32 VALU and the hardware exponential -- widened exactly to FP64 and fed
// to the same FP64 MFMA product with FP64 accumulators as kmatmul_kernel (kmatmul.hip).
//
// Why.  At nv <= 16 kmatmul_kernel is bound by its profile evaluations on the FP64 VALU (DESIGN
// 3.16): about 54 FP64 VALU instructions per element against two FP64 MFMAs per 16 elements.
// Everything built on the product is approximate far above single precision (CG to tol 1e-6,
// Hutchinson probes), and the CG driver (cg.hip) restores FP64 residuals by iterative refinement.
//
// Operands.  Per stationary part the scaled points y = l o x - c (FP64, c the centre gram_prepare
// leaves in ctx->dgc: the same for xa and xb) are rounded once to FP32 by kmm_f32_prep_kernel into
// ctx->dkmf: [part][point][DP] floats, DP = d rounded up to a multiple of 4, points padded to a
// multiple of 64, every padding entry an exact zero ((na + nb) nse DP floats; nothing is sized by
// na nb).
//
// Element.  The difference form D~ = sum_k (y~_ak - y~_bk)^2 in FP32: pairs of k by packed
// subtract and packed fma into an (even k, odd k) pair of sums, added at the end.  (Not the Gram
// form: its cancellation costs about (3 d + 4) u32 2 max|y|^2 in FP32.)  Zero padding adds exact
// zeros.  Profiles: SquaredExp p~ = exp2(-D~ log2 e) by v_exp_f32; Matern r = v_sqrt_f32(D~),
// p~ = poly(a r) exp2(-(a log2 e) r) with a log2 e folded into one constant (one rounding fewer
// in the exponent).  p~ in [0, 1] widens exactly; the parts combine as sum_p sigma_p^2 p~_p by FP64
// fma.  v_exp_f32 flushes results below 2^-126 to zero.  On the diagonal tile of a same-object
// form the element is formed as the FP64 route forms it -- t = fl(sigma sigma) p~ (+ eps), v += t,
// sigma_n^2 after the parts -- and D~ = 0 there (y~_a and y~_b are the same numbers) gives p~ = 1
// exactly, so K~'s diagonal is bit for bit the FP64 route's.
//
// Layout.  No Gram MFMA dictates the lane-to-element map, so it is chosen for the product: register
// q of block (rb, cb) in lane l is element (row 16 rb + 4 q + (l >> 4), column 16 cb + (l & 15)) of
// the wave's quadrant, rows = summed points xb, columns = output points xa -- the B operand of
// v_mfma_f64_16x16x4_f64 as in kmatmul_kernel, so the widened tile goes straight into Out^T += V^T
// K~ with no pass through LDS.  The quadrant is evaluated and multiplied in two halves of 16 rows
// (rb): 8 elements and 8 tile registers per lane at a time, which keeps every instance free of
// scratch at two workgroups per CU.  A lane needs 2 points of xa (cb) and 4 of xb (q) per part and
// half.
// With d <= 8 (DP = 4 or 8 compiled in) both come from LDS:
//   xa, the workgroup's 64 points, staged once, k-major [part][k][64]: a read is 16 consecutive
//       floats per k, the same for the four l >> 4 groups -- conflict-free;
//   xb, the current block, [part][point][DP] as in memory: a lane reads its point's DP floats as
//       16-byte reads; a wave touches 4 consecutive points (l >> 4), 16 DP contiguous bytes, every
//       other lane by broadcast -- conflict-free.  The next block is fetched into registers (one
//       or two 16-byte loads per thread) before the tile is evaluated and written to LDS after the
//       product, beside the next V block (kmm_fetch_v / kmm_stage_v).
// Above d = 8 the k walk runs at run time in chunks of four dimensions, 16-byte loads straight
// from the FP32 points in memory (L2-resident: 64 DP floats per block and part) into 8 pairs of
// running sums per half; LDS then holds V alone.  (Measured slower than the FP64 kernel at d = 16
// and nv <= 16, DESIGN 3.20: this walk is the part to improve.)
//
// Work split, slabs, partials in ctx->dkmm added by kmm_reduce_kernel in slab order (no atomics:
// two calls agree bit for bit), NVB = 1 for nv <= 16 else 4, wider V in passes of 64 columns, parts
// in groups of KMAXP: all as kmatmul_kernel.  Two workgroups per CU.
#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "kexp.hpp"
#include "kmm_vstage.hpp"

namespace {

typedef float kf2 __attribute__((ext_vector_type(2)));
typedef float kf4 __attribute__((ext_vector_type(4)));

// out[p][a][k] = (float)(xs[p][a][k] - c[p][k]) for a < n, k < d; 0 for the padding (a < npad,
// k < DP)
__global__ __launch_bounds__(256) void kmm_f32_prep_kernel(const double* __restrict__ xs, int n,
                                                           int d, int nse, int npad, int DP,
                                                           const double* __restrict__ c,
                                                           float* __restrict__ out) {
  const size_t total = (size_t)nse * npad * DP;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total;
       t += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(t % DP);
    const size_t r = t / DP;
    const int a = (int)(r % npad), p = (int)(r / npad);
    out[t] = (a < n && k < d) ? (float)(xs[((size_t)p * n + a) * d + k] - c[(size_t)p * d + k]) : 0.f;
  }
}

// the profile of one part in FP32 from D~ >= 0 (KPROF_* codes)
template <int PF>
__device__ __forceinline__ float kprof_f32(float D) {
  if constexpr (PF == 0) {
    return __builtin_amdgcn_exp2f(D * -1.44269504088896341f);
  } else {
    const float r = __builtin_amdgcn_sqrtf(D);
    // a = sqrt(3) | sqrt(5), and a log2 e as one constant
    const float ar = (PF == 1 ? 1.73205080756887729f : 2.23606797749978970f) * r;
    const float e = __builtin_amdgcn_exp2f((PF == 1 ? -2.49882107187017998f : -3.22596419032459143f) * r);
    float poly = 1.0f + ar;
    if constexpr (PF == 2) poly = __builtin_fmaf(ar * ar, 1.0f / 3.0f, poly);
    return e * poly;
  }
}

// SC > 0: DP = 4 SC compiled in (d <= 8), points from LDS; SC = 0: DP at run time, from memory.
// fb / npb: the summed points xb (the tile's rows); fa / npa: the output points xa (its columns).
// The rest as kmatmul_kernel.
template <int SC, bool MIX, int NVB>
__global__ __launch_bounds__(256, 2) void kmatmul_f32_kernel(
    KParams kp, const float* __restrict__ fb, const float* __restrict__ fa, int npb, int npa,
    int DPrt, int na, int nb, int diag, int slab_blocks, const double* __restrict__ V, size_t ldv,
    int nvc, int vec, double* __restrict__ Out, size_t ldo, size_t slab_stride, int accum) {
  extern __shared__ double dyn_lds[];
  constexpr int DPC = 4 * SC;                  // floats per point (SC > 0)
  constexpr int NXR = SC > 0 ? (KMAXP * 16 * DPC + 255) / 256 : 1;  // 16-byte units per thread of an xb block
  double* Vs = dyn_lds;                        // 16 NVB columns x KMM_VS
  float* XAs = reinterpret_cast<float*>(Vs + 16 * NVB * KMM_VS);  // [part][k][64]
  kf4* XBs = reinterpret_cast<kf4*>(XAs + kp.nse * DPC * 64);     // [part][point][SC]
  const int DP = SC > 0 ? DPC : DPrt;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wr = w & 1, wc = w >> 1;
  const int i0 = blockIdx.x * KT;
  const int jb_lo = blockIdx.y * slab_blocks;
  const int jb_hi = min(jb_lo + slab_blocks, (nb + KT - 1) / KT);
  const int xunits = kp.nse * 16 * DPC;        // 16-byte units of one xb block
  // this thread's units of the xb block at j0: unit u = part u / (16 DPC), 16 bytes u % (16 DPC) of
  // the part's 64 points (contiguous in memory, and in LDS in the same order)
  auto fetch_xb = [&](int j0, kf4 (&r)[NXR]) {
    if constexpr (SC > 0) {
#pragma unroll
      for (int i = 0; i < NXR; ++i) {
        const int u = threadIdx.x + 256 * i;
        if (u < xunits) {
          const int p = u / (16 * DPC), o = u % (16 * DPC);
          r[i] = reinterpret_cast<const kf4*>(fb + ((size_t)p * npb + j0) * DPC)[o];
        }
      }
    }
  };
  auto stage_xb = [&](const kf4 (&r)[NXR]) {
    if constexpr (SC > 0) {
#pragma unroll
      for (int i = 0; i < NXR; ++i) {
        const int u = threadIdx.x + 256 * i;
        if (u < xunits) XBs[u] = r[i];
      }
    }
  };
  if constexpr (SC > 0) {  // the workgroup's xa points, transposed to k-major
    for (int t = threadIdx.x; t < kp.nse * 64 * DPC; t += 256) {
      const int k = t % DPC, a = (t / DPC) % 64, p = t / (64 * DPC);
      XAs[(p * DPC + k) * 64 + a] = fa[((size_t)p * npa + i0 + a) * DPC + k];
    }
  }
  gd4 acc[NVB][2];
#pragma unroll
  for (int vb = 0; vb < NVB; ++vb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) acc[vb][cb] = gd4{0.0, 0.0, 0.0, 0.0};
  kv2 vr[2 * NVB];
  kf4 xr[NXR];
  kmm_fetch_v<NVB>(V, ldv, nb, nvc, jb_lo * KT, vec, vr);
  fetch_xb(jb_lo * KT, xr);
  kmm_stage_v<NVB>(vr, Vs);
  stage_xb(xr);
  __syncthreads();
  const int ca = 32 * wc + (lane & 15), rbq = 32 * wr + (lane >> 4);  // + 16 cb; + 16 rb + 4 q
  for (int jb = jb_lo; jb < jb_hi; ++jb) {
    const int j0 = jb * KT;
    const bool more = jb + 1 < jb_hi;
    if (more) {  // land under the tile
      kmm_fetch_v<NVB>(V, ldv, nb, nvc, j0 + KT, vec, vr);
      fetch_xb(j0 + KT, xr);
    }
    const bool dtile = diag && j0 == i0;
    // the tile in two halves of 16 rows (rb): evaluate 8 elements per lane, multiply them in --
    // half the tile's registers, and no instance of d <= 8 spills at two workgroups per CU
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      gd4 v[2] = {gd4{0.0, 0.0, 0.0, 0.0}, gd4{0.0, 0.0, 0.0, 0.0}};
#pragma nounroll
      for (int p = 0; p < kp.nse; ++p) {
        float D[2][4];  // D~ of the half's elements (cb, q)
        if constexpr (SC > 0) {
          kf2 ya[2][2 * SC];
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int k = 0; k < DPC; ++k)
              ya[cb][k >> 1][k & 1] = XAs[(p * DPC + k) * 64 + ca + 16 * cb];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            kf4 yb[SC];
#pragma unroll
            for (int s = 0; s < SC; ++s) yb[s] = XBs[(p * 64 + rbq + 16 * rb + 4 * q) * SC + s];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
              kf2 s2 = {0.f, 0.f};
#pragma unroll
              for (int s = 0; s < SC; ++s) {
                const kf2 d0 = ya[cb][2 * s] - kf2{yb[s][0], yb[s][1]};
                const kf2 d1 = ya[cb][2 * s + 1] - kf2{yb[s][2], yb[s][3]};
                s2 = __builtin_elementwise_fma(d0, d0, s2);
                s2 = __builtin_elementwise_fma(d1, d1, s2);
              }
              D[cb][q] = s2[0] + s2[1];
            }
          }
        } else {
          kf2 s2[2][4];
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) s2[cb][q] = kf2{0.f, 0.f};
          const int nch = DP >> 2;
          const kf4* pa = reinterpret_cast<const kf4*>(fa + ((size_t)p * npa + i0 + ca) * DP);
          const kf4* pb =
              reinterpret_cast<const kf4*>(fb + ((size_t)p * npb + j0 + rbq + 16 * rb) * DP);
          for (int c = 0; c < nch; ++c) {
            kf4 ya[2];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) ya[cb] = pa[(size_t)16 * cb * nch + c];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const kf4 yb = pb[(size_t)4 * q * nch + c];
#pragma unroll
              for (int cb = 0; cb < 2; ++cb) {
                const kf2 d0 = kf2{ya[cb][0], ya[cb][1]} - kf2{yb[0], yb[1]};
                const kf2 d1 = kf2{ya[cb][2], ya[cb][3]} - kf2{yb[2], yb[3]};
                s2[cb][q] = __builtin_elementwise_fma(d0, d0, s2[cb][q]);
                s2[cb][q] = __builtin_elementwise_fma(d1, d1, s2[cb][q]);
              }
            }
          }
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) D[cb][q] = s2[cb][q][0] + s2[cb][q][1];
        }
        // the profile, widened, into the tile
        const double sg2 = kp.sigma[p] * kp.sigma[p];
        kprof_dispatch<MIX>(MIX ? kp.prof[p] : 0, [&](auto pf) {
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const double pr = (double)kprof_f32<decltype(pf)::value>(D[cb][q]);
              if (dtile) {
                // (as gram_tile's diagonal tile: the product and the sums round on their own)
#pragma clang fp contract(off)
                const bool on_diag = wr == wc && rb == cb && (lane >> 4) + 4 * q == (lane & 15);
                double t = sg2 * (on_diag ? 1.0 : pr);
                if (on_diag) t += kp.eps;
                v[cb][q] += t;
              } else {
                v[cb][q] = fma(sg2, pr, v[cb][q]);
              }
            }
        });
      }
      if (dtile && kp.has_noise && wr == wc) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if ((lane >> 4) + 4 * q == (lane & 15)) v[rb][q] += kp.noise2;
      }
      // Out^T += V^T K~: the half's register q of block cb is k-step q's B operand
      const double* va = Vs + (lane & 15) * KMM_VS + 32 * wr + 16 * rb + (lane >> 4);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int vb = 0; vb < NVB; ++vb) {
          const double a = va[16 * vb * KMM_VS + 4 * q];
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
            acc[vb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, v[cb][q], acc[vb][cb], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);  // (the halves stay apart)
    }
    __syncthreads();  // the block's V and points are read
    if (more) {
      kmm_stage_v<NVB>(vr, Vs);
      stage_xb(xr);
    }
    __syncthreads();
  }
  // the two row halves' sums of a column half: wave (1, wc) hands its accumulators to (0, wc)
  double* red = Vs + wc * (NVB * 8 * 64) + lane;  // 1024 NVB doubles of the 1056 NVB
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
          if (i < na && c < nvc) {
            double* dst = O + (size_t)c * ldo + i;
            double s = acc[vb][cb][q] + red[((vb * 2 + cb) * 4 + q) * 64];
            if (accum) s = *dst + s;
            *dst = s;
          }
        }
  }
}

// one pass: columns [0, nvc <= 64) of V, the parts of g (<= KMAXP) at part offset p0
template <int SC, int NVB>
int kmm_f32_launch(gpr_ctx* ctx, const KmmOps& o, const KParams& g, int p0, const double* V,
                   int ldv, int nvc, double* Out, int ldo, int accum) {
  KmmSlabPlan pl;
  GPR_TRY(kmm_slab_plan(ctx, o.na, o.nb, V, ldv, nvc, Out, ldo, accum, &pl));
  const float* fb = o.fb + (size_t)p0 * o.fpb * o.fdp;
  const float* fa = o.fa + (size_t)p0 * o.fpa * o.fdp;
  const size_t lds = sizeof(double) * 16 * NVB * KMM_VS +
                     (SC > 0 ? sizeof(float) * 2 * g.nse * 64 * 4 * SC : 0);
  const dim3 grid((unsigned)pl.nta, (unsigned)pl.slabs);
  kmix_dispatch(g.mix, [&](auto mix) {
    kmatmul_f32_kernel<SC, decltype(mix)::value, NVB><<<grid, 256, lds, ctx->stream>>>(
        g, fb, fa, o.fpb, o.fpa, o.fdp, o.na, o.nb, o.same != GPR_CROSS, pl.slab_blocks, V,
        (size_t)ldv, nvc, pl.vec, pl.dst, pl.ldd, pl.stride, pl.accum);
  });
  LAUNCH_CHECK(ctx);
  if (pl.slabs > 1) GPR_TRY(kmm_reduce_slabs(ctx, pl.slabs, o.na, nvc, Out, ldo, accum));
  return 0;
}

template <int SC>
int kmm_f32_launch_nv(gpr_ctx* ctx, const KmmOps& o, const KParams& g, int p0, const double* V,
                      int ldv, int nvc, double* Out, int ldo, int accum) {
  return nvc <= 16 ? kmm_f32_launch<SC, 1>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum)
                   : kmm_f32_launch<SC, 4>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum);
}

}  // namespace

int kmm_f32_prepare(gpr_ctx* ctx, KmmOps* o) {
  const KParams& kp = o->kp;
  const int DP = (kp.d + 3) / 4 * 4;
  const int npa = (o->na + KT - 1) / KT * KT;
  const int npb = o->same != GPR_CROSS ? npa : (o->nb + KT - 1) / KT * KT;
  const size_t fa = (size_t)kp.nse * npa * DP, fb = o->same != GPR_CROSS ? 0 : (size_t)kp.nse * npb * DP;
  GPR_TRY(ensure_buf(ctx, ctx->dkmf, (fa + fb + 1) / 2));
  float* A = reinterpret_cast<float*>(ctx->dkmf.p);
  float* B = o->same != GPR_CROSS ? A : A + fa;
  auto prep = [&](const double* xs, int n, int npad, float* out) {
    const size_t total = (size_t)kp.nse * npad * DP;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 8192);
    kmm_f32_prep_kernel<<<blocks, 256, 0, ctx->stream>>>(xs, n, kp.d, kp.nse, npad, DP, ctx->dgc,
                                                         out);
  };
  prep(o->xa, o->na, npa, A);
  if (o->same == GPR_CROSS) prep(o->xb, o->nb, npb, B);
  LAUNCH_CHECK(ctx);
  o->fa = A;
  o->fb = B;
  o->fpa = npa;
  o->fpb = npb;
  o->fdp = DP;
  return 0;
}

int kmm_f32_apply(gpr_ctx* ctx, const KmmOps& o, const double* dV, int nv, int ldv, double* dOut,
                  int ldo) {
  const KParams& kp = o.kp;
  for (int c0 = 0; c0 < nv; c0 += 64) {
    const int nvc = std::min(64, nv - c0);
    const double* V = dV + (size_t)c0 * ldv;
    double* Out = dOut + (size_t)c0 * ldo;
    for (int p0 = 0, cnt = 0; p0 < kp.nse; p0 += cnt) {
      KParams g = kp;
      cnt = kp.nse;
      if (kp.nse > KMAXP) {  // groups of parts; the last one carries the noise
        cnt = std::min(KMAXP, kp.nse - p0);
        g = kparams_group(kp, p0, cnt, p0 + cnt >= kp.nse ? kp.has_noise : 0);
      }
      const int accum = p0 > 0;
      if (o.fdp == 4) GPR_TRY((kmm_f32_launch_nv<1>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum)));
      else if (o.fdp == 8) GPR_TRY((kmm_f32_launch_nv<2>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum)));
      else GPR_TRY((kmm_f32_launch_nv<0>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum)));
    }
  }
  return 0;
}
