// What the K-assembly kernels (assembly.hip) and the fused MLL gradient (mll.hip) share:
//  - exp(-dist) scaled by a part's sigma^2 via an LDS table, so both evaluate the kernel with
//    the same ~1-ulp exponential, and the radial profiles built on it (kprof_*);
//  - the per-part profile dispatch (kprof_dispatch) and its host half (kmix_dispatch);
//  - the walk over the upper-triangle tiles (tri_tile).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#ifndef GPR_EXP32  // 1: 32-entry exp tables (conflict-free LDS gathers, 2 more FMAs)
#define GPR_EXP32 0
#endif
// Tang's reduction with x = -dist (already in range): kf = x 256/ln2 + 1.5 2^52 holds
// n = rint(x 256/ln2) in its low word (magic-constant rounding: no rndne / cvt), r = x -
// n ln2/256 in two Cody-Waite steps, a degree-4 expm1 (truncation < 0.2 ulp), exp(x) =
// 2^(n >> 8) T[n & 255] (1 + expm1(r)) with sigma^2 folded into the table (fl(fl(sigma sigma)
// T[j]): two roundings on top of T[j]'s own).  Error budget and its test: DESIGN 3.5.1.
static __device__ __forceinline__ double kexp_core(double x, const double* ts) {
  const double kf = fma(x, 369.3299304675746, 6755399441055744.0);
  const double nf = kf - 6755399441055744.0;
  double r = fma(nf, -0.00270760617331689, x);
  r = fma(nf, -7.453964567463233e-13, r);
  const int ni = (int)(unsigned)__double_as_longlong(kf);
  double p = fma(r, 0.041666666666666664, 0.16666666666666666);
  p = fma(r, p, 0.5);
  p = r * p;
  const double q = fma(r, p, r);  // expm1(r)
  const double t = ts[ni & 255];
  return __builtin_ldexp(fma(t, q, t), ni >> 8);
}

// s2 * exp(-dist) with the part's table ts[j] = s2 * 2^(j/256): x = -dist clamped at -800 (exp
// underflows to 0 long before; a NaN dist fails the compare and propagates).  16 VALU + 1 LDS
// read per element.
static __device__ __forceinline__ double kexp_s2(double dist, const double* ts) {
#ifdef GPR_KBUILD_NOEXP
  return ts[0] * fma(dist, -1e-3, 1.0);
#elif GPR_EXP32
  // 32-entry table 2^(j/32) (every entry in its own LDS bank pair: conflict-free gathers),
  // |r| <= ln2/64, degree-6 expm1 (truncation < 0.03 ulp); tab[j] = ts[8 j]
  const double x = dist > 800.0 ? -800.0 : -dist;
  const double kf = fma(x, 46.16624130844683, 6755399441055744.0);
  const double nf = kf - 6755399441055744.0;
  double r = fma(nf, -0.02166084938653512, x);  // ln2/32 = L1 (32 bits) + L2
  r = fma(nf, -5.9631716539705866e-12, r);
  const int ni = (int)(unsigned)__double_as_longlong(kf);
  double p = fma(r, 1.3888888888888889e-03, 8.3333333333333332e-03);
  p = fma(r, p, 0.041666666666666664);
  p = fma(r, p, 0.16666666666666666);
  p = fma(r, p, 0.5);
  p = r * p;
  const double q = fma(r, p, r);
  const double t = ts[ni & 31];
  return __builtin_ldexp(fma(t, q, t), ni >> 5);
#else
  return kexp_core(dist > 800.0 ? -800.0 : -dist, ts);
#endif
}

// ---- radial profiles of the stationary parts -----------------------------------------------
// k = sigma^2 f(D) of the ARD-scaled squared distance D = sum_k (l_k (x_k - x'_k))^2, and
// W = -dk/dD (what the length-scale derivatives need: dk/dl_k = -2 l_k W (x_k - x'_k)^2):
//   PF = 0  SquaredExp  k = s2 exp(-D)                           W = k
//   PF = 1  Matern-3/2  k = s2 (1 + a r) exp(-a r),     a = 3^.5  W = s2 (3/2) exp(-a r)
//   PF = 2  Matern-5/2  k = s2 (1 + a r + (a r)^2 / 3) exp(-a r), a = 5^.5
//                                                                W = s2 (5/6) (1 + a r) exp(-a r)
// with r = sqrt(max(D, 0)) (the codes are KPROF_* of common.hpp).  The clamp matters: the Gram
// form of the distance returns D a few 1e-16 BELOW zero for coincident points, which exp never
// noticed and a square root turns into NaN.  (A NaN D fails the compare and propagates.)  The
// exponential is the table one above with s2 folded in, so a Matern element costs the SE
// element plus one FP64 square root and two or three FMAs.  The profile is per part, i.e.
// wave-uniform: callers branch on it once per part (kprof_dispatch), outside their element
// loops, and the element code is compiled per profile.
template <int PF>
static __device__ __forceinline__ double kprof_s2(double D, const double* ts) {
  if constexpr (PF == 0) {
    return kexp_s2(D, ts);
  } else {
    const double ar = (PF == 1 ? 1.7320508075688772 : 2.23606797749979) *
                      __builtin_sqrt(D < 0.0 ? 0.0 : D);
    const double e = kexp_s2(ar, ts);
    double poly = 1.0 + ar;
    if constexpr (PF == 2) poly = fma(ar * ar, 1.0 / 3.0, poly);
    return e * poly;
  }
}

// the same, also returning W = -dk/dD (finite at r = 0)
template <int PF>
static __device__ __forceinline__ double kprof_s2_w(double D, const double* ts, double* W) {
  if constexpr (PF == 0) {
    const double k = kexp_s2(D, ts);
    *W = k;
    return k;
  } else {
    const double ar = (PF == 1 ? 1.7320508075688772 : 2.23606797749979) *
                      __builtin_sqrt(D < 0.0 ? 0.0 : D);
    const double e = kexp_s2(ar, ts);
    double poly = 1.0 + ar;
    if constexpr (PF == 1) {
      *W = 1.5 * e;
    } else {
      *W = (5.0 / 6.0) * (e * poly);
      poly = fma(ar * ar, 1.0 / 3.0, poly);
    }
    return e * poly;
  }
}

// the same with the profile as a run-time, wave-uniform code (the product-term phases of the
// gradient kernels, which walk the factors of a term in one loop)
static __device__ __forceinline__ double kprof_s2_w_rt(int prof, double D, const double* ts,
                                                       double* W) {
  if (prof == 1) return kprof_s2_w<1>(D, ts, W);
  if (prof == 2) return kprof_s2_w<2>(D, ts, W);
  return kprof_s2_w<0>(D, ts, W);
}

// The scaled squared distance of one pair for one part, as the gradient kernels' wide passes form
// it: sum_k l_k^2 r_k^2 on raw x (xa, xb), or for a Periodic part (per, wave-uniform) sum_k l_k^2
// ((cos a - cos b)^2 + (sin a - sin b)^2) on the unit features (ca, cb: [cos | sin], d each).  Two
// partial sums, even and odd k.  Used where a product term needs every factor's value per pair.
static __device__ __forceinline__ double kpair_dist(bool per, int d, const double* __restrict__ l2,
                                                    const double* __restrict__ xa,
                                                    const double* __restrict__ xb,
                                                    const double* __restrict__ ca,
                                                    const double* __restrict__ cb) {
  double a0 = 0.0, a1 = 0.0;
  if (per) {
    for (int k = 0; k < d; ++k) {
      const double dc = ca[k] - cb[k], ds = ca[d + k] - cb[d + k];
      const double t = fma(dc, dc, ds * ds);
      if (k & 1) a1 = fma(l2[k], t, a1);
      else a0 = fma(l2[k], t, a0);
    }
  } else {
    for (int k = 0; k < d; ++k) {
      const double r = xa[k] - xb[k];
      if (k & 1) a1 = fma(l2[k], r * r, a1);
      else a0 = fma(l2[k], r * r, a0);
    }
  }
  return a0 + a1;
}

// the profiles with the library exponential (the difference-form fallback kernels, dK/dtheta):
// prof is a run-time, wave-uniform code
static __device__ __forceinline__ double kprof_exact_w(int prof, double s2, double D, double* W) {
  if (prof == 0) {
    const double k = s2 * exp(-1.0 * D);
    *W = k;
    return k;
  }
  const double ar = (prof == 1 ? 1.7320508075688772 : 2.23606797749979) *
                    __builtin_sqrt(D < 0.0 ? 0.0 : D);
  const double e = s2 * exp(-1.0 * ar);
  double poly = 1.0 + ar;
  if (prof == 1) {
    *W = 1.5 * e;
  } else {
    *W = (5.0 / 6.0) * (e * poly);
    poly = fma(ar * ar, 1.0 / 3.0, poly);
  }
  return e * poly;
}

// f(tag) with tag = kprof_tag<profile>: one scalar branch per call.  MIX =
// false compiles the SquaredExp body alone (the instantiations SE-only descriptions launch).
template <int PF>
struct kprof_tag {
  static constexpr int value = PF;
};
template <bool MIX, class F>
static __device__ __forceinline__ void kprof_dispatch(int prof, F&& f) {
  if constexpr (!MIX) {
    f(kprof_tag<0>{});
  } else {
    if (prof == 1) f(kprof_tag<1>{});
    else if (prof == 2) f(kprof_tag<2>{});
    else f(kprof_tag<0>{});
  }
}

// Host side of MIX: f(std::bool_constant<MIX>) with MIX = the description has a non-SquaredExp
// profile (KParams::mix) -- the one place a launcher picks between a kernel's two instantiations.
template <class F>
static inline auto kmix_dispatch(bool mix, F&& f) {
  return mix ? f(std::true_type{}) : f(std::false_type{});
}

// Host side of MIX and PROD: f(bool_constant<MIX>, bool_constant<PROD>).  A description with a
// product term (KParams::prod) launches the MIX instantiation whatever its profiles are -- MIX
// reads each part's profile at run time, SquaredExp included -- so PROD adds one instantiation
// per kernel, not two; without a product this is kmix_dispatch.
template <class F>
static inline auto kmixprod_dispatch(bool mix, bool prod, F&& f) {
  if (prod) return f(std::true_type{}, std::true_type{});
  return mix ? f(std::true_type{}, std::false_type{}) : f(std::false_type{}, std::false_type{});
}

// all four combinations (the Gram tile kernels: a product of SquaredExp-profile parts keeps the
// MIX = false kernels' launch bounds)
template <class F>
static inline auto kmixprod_dispatch_full(bool mix, bool prod, F&& f) {
  if (prod) return mix ? f(std::true_type{}, std::true_type{}) : f(std::false_type{}, std::true_type{});
  return mix ? f(std::true_type{}, std::false_type{}) : f(std::false_type{}, std::false_type{});
}

// the same without the clamp (3 VALU fewer), for callers that have bounded dist < 5.8e6, so
// that n fits the int32 low word: below -745 the ldexp underflows to 0 as in the clamped form,
// and a NaN propagates
static __device__ __forceinline__ double kexp_s2_nc(double dist, const double* ts) {
#if defined(GPR_KBUILD_NOEXP) || GPR_EXP32
  return kexp_s2(dist, ts);
#else
  return kexp_core(-dist, ts);
#endif
}

// Upper-triangle tile bid -> (bi <= bj), column-by-column order (bid = bj (bj + 1) / 2 + bi).
// The tile walk shared by the symmetric K kernels and the MLL gradient pass.  SCALAR: the
// results are pinned to SGPRs (readfirstlane; bid is wave-uniform either way).  The kernels that
// decoded the index in place before this function existed call it with SCALAR = false and keep
// the register allocation they had: several sit at their launch bounds' VGPR limit, where the
// pinned form moved spills (kmat_sym2_kernel<16, true>: 303 -> 307).
template <bool SCALAR = true>
static __device__ __forceinline__ void tri_tile(int bid, int* bi, int* bj) {
  int j = (int)((sqrt(8.0 * bid + 1.0) - 1.0) * 0.5);
  while ((j + 1) * (j + 2) / 2 <= bid) ++j;
  while (j * (j + 1) / 2 > bid) --j;
  int i = bid - j * (j + 1) / 2;
  if (SCALAR) {
    j = __builtin_amdgcn_readfirstlane(j);
    i = __builtin_amdgcn_readfirstlane(bid - j * (j + 1) / 2);
  }
  *bj = j;
  *bi = i;
}
