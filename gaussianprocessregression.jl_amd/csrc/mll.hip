// Negative log marginal likelihood and its fused hyper-parameter gradient on gfx950.
//
// Value: loss(MLL, kchol, y, alpha) = 0.5 (y.alpha + logdet + N log 2pi)
//        src/loss_grad.jl:39-41 via src/cost.jl:113-117.
// Gradient: the reference loops over the D hyper-parameters, materialising dK_i
// (src/deriv_covar.jl:20-32) and doing a GEMV + a Frobenius dot per i
// (src/loss_grad.jl:43-52, src/cost.jl:119-126): D x 3 passes over N^2 matrices.
// Here all D components come out of ONE pass over the upper triangle of K^{-1}:
//   g_i = -0.5 sum_ab M_ab dK_i,ab,   M = alpha alpha^T - K^{-1}
// with dK recomputed in registers from x:  dK/dsigma = (2/|sigma|) K_p (incl. eps on the
// diagonal), dK/dl_k = -2 l_k W_p (x_k,a - x_k,b)^2 (raw x; W = -dk/dD of the part's profile,
// kexp.hpp: K_p itself for SquaredExp), dK/dsigma_n = 2 sigma_n I.
// Off-diagonal tiles count twice (symmetry).  Per-workgroup partial sums are reduced in a
// fixed order by a second kernel (deterministic).
#include <cmath>

#include "common.hpp"
#include "kexp.hpp"

namespace {

constexpr int GT = 64;

__global__ __launch_bounds__(1024) void mll_terms_kernel(const double* __restrict__ U, size_t ldu,
                                                         int n, const double* __restrict__ y,
                                                         const double* __restrict__ alpha,
                                                         double* __restrict__ out) {
  __shared__ double r0[16], r1[16];
  double s_dot = 0.0, s_log = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    s_dot = fma(y[i], alpha[i], s_dot);
    s_log += log(U[(size_t)i + (size_t)i * ldu]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    s_dot += __shfl_xor(s_dot, o);
    s_log += __shfl_xor(s_log, o);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    r0[w] = s_dot;
    r1[w] = s_log;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < 16; ++i) {
      a += r0[i];
      b += r1[i];
    }
    out[0] = a;
    out[1] = b;
  }
}

// ---- the pieces of the gradient kernels, written once --------------------------------------
// (mll_grad_wide_kernel, which is the wide and the Periodic pass, uses all of them;
// mll_grad_tiles_kernel the tile index and the reduction, see there.  grad_tile, grad_fill_tabs
// and grad_store_wn therefore exist a second time, written out in mll_grad_tiles_kernel: a fix
// to one of them must be made in both places.)
// A thread's place in the pass: one workgroup per upper tile (bi <= bj), lane = row i0 + lane,
// wave wv = the 16 columns j0 + wv + 4c.  Columns past n are clamped to point n - 1 with zero
// weight.
struct GradTile {
  int bi, bj, i0, j0, lane, wv, i;
  bool irow;    // i < n
  size_t irc;   // the row, clamped
  double wgt;   // off-diagonal tiles count twice (symmetry)
  double ai;    // alpha_i (0 past n)
  double s_wn;  // WhiteNoise term: alpha_a^2 - Kinv_aa from the thread whose columns hold a
                // (diagonal tiles only)
};
__device__ __forceinline__ GradTile grad_tile(int n, const double* __restrict__ Kinv, size_t ldk,
                                              const double* __restrict__ alpha) {
  GradTile g;
  tri_tile<false>(blockIdx.x, &g.bi, &g.bj);
  g.i0 = g.bi * GT;
  g.j0 = g.bj * GT;
  g.lane = threadIdx.x & 63;
  g.wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  g.i = g.i0 + g.lane;
  g.irow = g.i < n;
  g.irc = (size_t)min(g.i, n - 1);
  g.wgt = (g.bi == g.bj) ? 1.0 : 2.0;
  g.ai = g.irow ? alpha[g.i] : 0.0;
  g.s_wn = 0.0;
  if (g.bi == g.bj && g.irow && ((g.lane - g.wv) & 3) == 0)
    g.s_wn = g.ai * g.ai - Kinv[(size_t)g.i + (size_t)g.i * ldk];
  return g;
}

// the exp tables sigma_p^2 2^(j/256) of the group of up to KMAXP parts that starts at part p0
__device__ __forceinline__ void grad_fill_tabs(const KParams& kp, int p0, double (*tabs)[256]) {
  for (int g = p0; g < min(kp.nse, p0 + KMAXP); ++g)
    tabs[g - p0][threadIdx.x] = (kp.sig[g] * kp.sig[g]) * kp.exptab[threadIdx.x];
}

// A part's sums to its slots: acc_s (already summed over the wave) and the N per-thread sums
// acc[] through red[wave][1 + N] to out[dst(t)] for t in [t0, nt) (dst(t) < 0: no slot), the four
// waves added in a fixed order.
template <int N, int W, class Dst>
__device__ __forceinline__ void grad_reduce(int lane, int wv, double acc_s, double (&acc)[N],
                                            double (&red)[4][W], int t0, int nt,
                                            double* __restrict__ out, Dst&& dst) {
#pragma unroll
  for (int k = 0; k < N; ++k)
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
  __syncthreads();
  if (lane == 0) {
    red[wv][0] = acc_s;
#pragma unroll
    for (int k = 0; k < N; ++k) red[wv][1 + k] = acc[k];
  }
  __syncthreads();
  for (int t = threadIdx.x + t0; t < nt; t += 256) {
    const int s = dst(t);
    if (s >= 0) out[s] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
  }
}

// WhiteNoise term: sum_a (alpha_a^2 - Kinv_aa) (only diagonal tiles contribute), through the
// last column of red
template <int W>
__device__ __forceinline__ void grad_store_wn(const GradTile& g, double (&red)[4][W],
                                              double* __restrict__ out) {
  double s_wn = g.s_wn;
  for (int o = 32; o > 0; o >>= 1) s_wn += __shfl_xor(s_wn, o);
  __syncthreads();
  if (g.lane == 0) red[g.wv][W - 1] = s_wn;
  __syncthreads();
  if (threadIdx.x == 0) *out = red[0][W - 1] + red[1][W - 1] + red[2][W - 1] + red[3][W - 1];
}

// (This kernel shares tri_tile and grad_reduce only.  Its prologue, table fill and WhiteNoise
// epilogue are the lines of grad_tile, grad_fill_tabs and grad_store_wn written out: taken through
// those helpers, every instance kept its register counts within a few SGPR spills, but the
// compiler scheduled the column loop differently, and gpr_mll_grad measured 1.1 % slower at
// d = 32 and 0.6 % at d = 16 with a Matern part.  As it stands the column loop compiles to the
// instructions and registers it had before the helpers existed in 18 of the 20 instances.
// A fix to one of the three helpers must be repeated in the lines marked [grad_tile],
// [grad_fill_tabs] and [grad_store_wn] below.)
// partial[bid][slot]: slot layout = for each stationary part p: [S_sigma, S_l1..S_ld], then
// S_wn.  S_sigma sums mv K_p, S_lk sums mv W_p r_k^2.  MIX: the description has a Matern part
// (each part's profile from the device table, one scalar branch per part); SE-only
// descriptions launch MIX = false, the kernel they always launched.
// EXACT: d == D (no per-feature bound checks).  Branch-free inner loop: columns past n are
// clamped to point n - 1 with zero weight, K_p by the K-assembly's table exponential.
template <int D, bool EXACT, bool MIX>
__global__ __launch_bounds__(256) void mll_grad_tiles_kernel(KParams kp, const double* __restrict__ X,
                                                             int n, const double* __restrict__ Kinv,
                                                             size_t ldk, const double* __restrict__ alpha,
                                                             double* __restrict__ partial, int nslot) {
  __shared__ double red[4][D + 2];
  __shared__ double tabs[KMAXP][256];  // sigma_p^2 2^(j/256)
  const int bid = blockIdx.x;
  // [grad_tile] from here to s_wn
  int bi, bj;
  tri_tile<false>(bid, &bi, &bj);
  const int i0 = bi * GT, j0 = bj * GT;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int d = EXACT ? D : kp.d;
  const int i = i0 + lane;
  const bool irow = i < n;
  const double wgt = (bi == bj) ? 1.0 : 2.0;
  // (the tables of the first KMAXP parts; further groups of KMAXP re-fill them below)
  // [grad_fill_tabs]
  for (int p = 0; p < min(kp.nse, KMAXP); ++p)
    tabs[p][threadIdx.x] = (kp.sig[p] * kp.sig[p]) * kp.exptab[threadIdx.x];

  // WhiteNoise term: alpha_a^2 - Kinv_aa from the thread whose columns hold a (diagonal tiles)
  const double ai = irow ? alpha[i] : 0.0;
  double s_wn = 0.0;
  if (bi == bj && irow && ((lane - wv) & 3) == 0) s_wn = ai * ai - Kinv[(size_t)i + (size_t)i * ldk];

  double xr[D];
#pragma unroll
  for (int k = 0; k < D; ++k) xr[k] = (irow && (EXACT || k < d)) ? X[(size_t)i * d + k] : 0.0;
  __syncthreads();  // tabs

  int slot = 0;
  for (int p = 0; p < kp.nse; ++p) {
    if (p > 0 && (p & (KMAXP - 1)) == 0) {  // next group of parts: its exp tables
      __syncthreads();
      for (int g = p; g < min(kp.nse, p + KMAXP); ++g)  // [grad_fill_tabs]
        tabs[g - p][threadIdx.x] = (kp.sig[g] * kp.sig[g]) * kp.exptab[threadIdx.x];
      __syncthreads();
    }
    const double* ts = tabs[p & (KMAXP - 1)];
    const double* l2p = kp.l2 + (size_t)p * d;
    double acc_s = 0.0;
    double acc_l[D];
#pragma unroll
    for (int k = 0; k < D; ++k) acc_l[k] = 0.0;
    // (not unrolled: unrolled, the wave-uniform point loads of all 16 columns were hoisted
    // into SGPRs and spilled)
    // K^-1's entries one column ahead (a global load's latency behind the current column's
    // distance and exponential instead of in front of its weight)
    const size_t irc = (size_t)min(i, n - 1);
    double kin = Kinv[irc + (size_t)min(j0 + wv, n - 1) * ldk];
    kprof_dispatch<MIX>(MIX ? __builtin_amdgcn_readfirstlane((int)kp.pf[p]) : 0, [&](auto pf) {
#pragma unroll 1
    for (int c = 0; c < 16; ++c) {
      const int jr = j0 + wv + 4 * c;
      const int j = min(jr, n - 1);  // wave-uniform: scalar loads of the point
      const double kcur = kin;
      if (c < 15) kin = Kinv[irc + (size_t)min(jr + 4, n - 1) * ldk];
      // M_ab = w (alpha_a alpha_b - Kinv_ab), 0 past n
      const double mv = (irow && jr < n) ? wgt * (ai * alpha[j] - kcur) : 0.0;
      const double* xc = X + (size_t)j * d;
      // D = sum_k l_k^2 r_k^2 over the raw differences r_k (l_k^2 from the kernel arguments,
      // four partial sums: no 16-long dependent chain, no scaled copy of the row point held
      // in registers); dK/dl_k's r_k^2 recomputed after the exponential
      double dpart[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < D; ++k) {
        if (EXACT || k < d) {
          const double r = xr[k] - xc[k];
          dpart[k & 3] = fma(l2p[k], r * r, dpart[k & 3]);
        }
      }
      const double dist = (dpart[0] + dpart[1]) + (dpart[2] + dpart[3]);
      double Wp;
      const double Kp = kprof_s2_w<decltype(pf)::value>(dist, ts, &Wp) + (i == j ? kp.eps : 0.0);
      const double mk = mv * Kp;
      acc_s += mk;
      // (SquaredExp: W = K_p, and eps meets r = 0 only -- the weight it always had)
      const double mw = decltype(pf)::value == 0 ? mk : mv * Wp;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        if (EXACT || k < d) {
          const double r = xr[k] - xc[k];
          acc_l[k] = fma(mw, r * r, acc_l[k]);
        }
      }
    }
    });
    // workgroup reduction of (acc_s, acc_l[0..d)) -> partial slots
    for (int o = 32; o > 0; o >>= 1) acc_s += __shfl_xor(acc_s, o);
    grad_reduce(lane, wv, acc_s, acc_l, red, 0, d + 1, partial + (size_t)bid * nslot + slot,
                [](int t) { return t; });
    slot += d + 1;
  }
  // [grad_store_wn] WhiteNoise term: sum_a (alpha_a^2 - Kinv_aa) (only diagonal tiles contribute)
  for (int o = 32; o > 0; o >>= 1) s_wn += __shfl_xor(s_wn, o);
  __syncthreads();
  if (lane == 0) red[wv][D + 1] = s_wn;
  __syncthreads();
  if (threadIdx.x == 0)
    partial[(size_t)bid * nslot + slot] = red[0][D + 1] + red[1][D + 1] + red[2][D + 1] + red[3][D + 1];
}

// The same pass for any d, for d > 32 (where the row point and its d sums no longer fit in
// registers) and for a description with a Periodic part (PER).  Per part and 64 x 64 tile, two
// phases:
//  1. each thread's 16 weights mk_c = w (alpha_a alpha_b - Kinv_ab) W_p,ab (K_p,ab for
//     SquaredExp; S_sigma sums the K_p ones), the distance by a
//     run-time loop over all d (row point from global memory / L1, column point wave-uniform);
//     the Kinv tile is read once per part; the 16 values go to the thread's own LDS slots (no
//     barrier: each thread reads back only what it wrote) -- held in a register array they
//     forced both column loops to be unrolled, and the unrolled wave-uniform point loads were
//     hoisted into SGPRs and spilled (1686 SGPR spills);
//  2. per chunk of GW = 32 dimensions: the row point's 32 features into registers, acc_l[k] +=
//     mk_c (x_ka - x_kb)^2 over the 16 columns (column points re-read from L2, scalar loads),
//     reduced as in mll_grad_tiles_kernel into slots 1 + 32 chunk + k.
// S_sigma and the WhiteNoise slot are written once.  Same slot layout, same reduction kernel.
// PER: one wave-uniform branch per part on "is periodic"; the other parts run the two phases
// above on raw x unchanged.  cs: per part and point the unit features [cos a_k | sin a_k],
// a_k = 2 pi x_k / p_k (launch_embed_unit; 2d wide, only Periodic parts' rows are read) -- no
// pair evaluates a transcendental but the exponential.
// Periodic part, slots [S_sigma, S_l1..S_ld, S_p1..S_pd]:
//  1. D = sum_k l_k^2 chord_k^2, chord_k^2 = (cos a - cos b)^2 + (sin a - sin b)^2
//     = (2 sin(pi r_k / p_k))^2, GP dimensions at a time; weights mk = mv K_p as for SquaredExp;
//  2. per chunk of GP = 8 dimensions (row point's x, cos, sin and two sums: 40 doubles; at 16
//     the unrolled wave-uniform column loads cost 50 more SGPR spills for no fewer passes that
//     matter):
//     S_lk += mk chord_k^2, S_pk += mk r_k sin(a_k - b_k), sin(a - b) = sin a cos b - cos a sin b.
// PROD: the description has a product term (launched with MIX: profiles at run time).  Part p is
// a factor of the term of parts [t0, t1], whose exp tables are filled when the term opens.  Phase
// 1 evaluates EVERY factor of the term for each of the thread's 16 pairs (kpair_dist), forms the
// cofactor C = prod_{g != p} K_g as a product, sums mv (K_p C + eps on the diagonal) into S_sigma
// and leaves mv W_p C as phase 2's weight: a term of F factors costs F^2 evaluations per pair
// (the cofactor is re-evaluated per factor rather than F value arrays of 16 x 256 held in LDS:
// DESIGN 3.13).  Phase 2, the slots and the reduction are unchanged.
constexpr int GW = 32;
constexpr int GP = 8;
template <bool MIX, bool PER, bool PROD = false>
__global__ __launch_bounds__(256) void mll_grad_wide_kernel(KParams kp, const double* __restrict__ X,
                                                            const double* __restrict__ cs, int n,
                                                            const double* __restrict__ Kinv,
                                                            size_t ldk, const double* __restrict__ alpha,
                                                            double* __restrict__ partial, int nslot) {
  __shared__ double red[4][GW + 2];
  __shared__ double tabs[KMAXP][256];  // sigma_p^2 2^(j/256)
  __shared__ double mks[16][256];      // mk_c of every thread
  const GradTile g = grad_tile(n, Kinv, ldk, alpha);
  const int d = kp.dx, de = kp.de;
  const int i = g.i, j0 = g.j0, wv = g.wv;
  const bool irow = g.irow;
  const double wgt = g.wgt, ai = g.ai;
  const size_t irc = g.irc;
  const double* xrow = X + irc * d;

  double* out = partial + (size_t)blockIdx.x * nslot;
  int t0 = 0, t1 = -1;  // PROD: the open term's parts
  for (int p = 0; p < kp.nse; ++p) {
    if constexpr (PROD) {
      if (p > t1) {  // part p opens a term: its last factor (<= KMAXP per term), its exp tables
        t0 = t1 = p;
        while (t1 + 1 < kp.nse && t1 - t0 + 1 < KMAXP &&
               __builtin_amdgcn_readfirstlane((int)kp.tend[t1]) == 0)
          ++t1;
        __syncthreads();
        for (int g = t0; g <= t1; ++g)
          tabs[g - t0][threadIdx.x] = (kp.sig[g] * kp.sig[g]) * kp.exptab[threadIdx.x];
        __syncthreads();
      }
    } else if ((p & (KMAXP - 1)) == 0) {  // this group of parts' exp tables
      __syncthreads();
      grad_fill_tabs(kp, p, tabs);
      __syncthreads();
    }
    const double* ts = tabs[PROD ? p - t0 : p & (KMAXP - 1)];
    const double* l2p = kp.l2 + (size_t)p * d;
    const bool per = PER && __builtin_amdgcn_readfirstlane((int)kp.per[p]) != 0;
    // this part's unit features (cs is null without a Periodic part)
    const double* csp = PER ? cs + (size_t)p * n * de : nullptr;
    const double* crow = PER ? csp + irc * de : nullptr;
    // phase 1: the 16 weights.  A Periodic part's 16 distances first, GP dimensions of the row
    // point's cos / sin in registers at a time (the row point is read once per chunk, not once
    // per column), accumulated in the thread's own mks slots
    if (!PROD && per) {
      for (int k0 = 0; k0 < d; k0 += GP) {
        const int kn = min(GP, d - k0);  // wave-uniform
        double cr[GP], sr[GP];
#pragma unroll
        for (int k = 0; k < GP; ++k) {
          cr[k] = k < kn ? crow[k0 + k] : 0.0;
          sr[k] = k < kn ? crow[d + k0 + k] : 0.0;
        }
#pragma unroll 1
        for (int c = 0; c < 16; ++c) {
          const int j = min(j0 + wv + 4 * c, n - 1);
          const double* cc = csp + (size_t)j * de + k0;
          double a0 = 0.0, a1 = 0.0;
#pragma unroll
          for (int k = 0; k < GP; ++k) {
            const double cb = k < kn ? cc[k] : 0.0, sb = k < kn ? cc[d + k] : 0.0;
            const double l2 = k < kn ? l2p[k0 + k] : 0.0;
            const double dc = cr[k] - cb, ds = sr[k] - sb;
            if (k & 1) a1 = fma(l2, fma(dc, dc, ds * ds), a1);
            else a0 = fma(l2, fma(dc, dc, ds * ds), a0);
          }
          const double prev = k0 ? mks[c][threadIdx.x] : 0.0;
          mks[c][threadIdx.x] = prev + (a0 + a1);
        }
      }
    }
    double acc_s = 0.0;
    if constexpr (PROD) {
#pragma unroll 1
      for (int c = 0; c < 16; ++c) {
        const int jr = j0 + wv + 4 * c;
        const int j = min(jr, n - 1);  // wave-uniform
        const double kin = Kinv[irc + (size_t)j * ldk];
        const double mv = (irow && jr < n) ? wgt * (ai * alpha[j] - kin) : 0.0;
        double Kp = 0.0, Wp = 0.0, C = 1.0;
        for (int g = t0; g <= t1; ++g) {
          const bool perg = PER && __builtin_amdgcn_readfirstlane((int)kp.per[g]) != 0;
          const double* csg = PER ? cs + (size_t)g * n * de : nullptr;
          const double dist = kpair_dist(perg, d, kp.l2 + (size_t)g * d, xrow, X + (size_t)j * d,
                                         PER ? csg + irc * de : nullptr,
                                         PER ? csg + (size_t)j * de : nullptr);
          double Wg;
          const double Kg = kprof_s2_w_rt(__builtin_amdgcn_readfirstlane((int)kp.pf[g]), dist,
                                          tabs[g - t0], &Wg);
          if (g == p) {
            Kp = Kg;
            Wp = Wg;
          } else {
            C *= Kg;
          }
        }
        acc_s += mv * (Kp * C + (i == j ? kp.eps : 0.0));
        mks[c][threadIdx.x] = mv * (Wp * C);  // phase 2's weight
      }
    } else {
    kprof_dispatch<MIX>(MIX ? __builtin_amdgcn_readfirstlane((int)kp.pf[p]) : 0, [&](auto pf) {
#pragma unroll 1
    for (int c = 0; c < 16; ++c) {
      const int jr = j0 + wv + 4 * c;
      const int j = min(jr, n - 1);  // wave-uniform: scalar loads of the point
      const double kin = Kinv[irc + (size_t)j * ldk];
      const double mv = (irow && jr < n) ? wgt * (ai * alpha[j] - kin) : 0.0;
      double dist;
      if (per) {
        dist = mks[c][threadIdx.x];
      } else {
        // D = sum_k l_k^2 r_k^2 in four partial sums, element k into dpart[k & 3]
        const double* xc = X + (size_t)j * d;
        double dpart[4] = {0.0, 0.0, 0.0, 0.0};
        int k = 0;
#pragma unroll 1
        for (; k + 4 <= d; k += 4) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const double r = xrow[k + u] - xc[k + u];
            dpart[u] = fma(l2p[k + u], r * r, dpart[u]);
          }
        }
        for (; k < d; ++k) {
          const double r = xrow[k] - xc[k];
          dpart[k & 3] = fma(l2p[k], r * r, dpart[k & 3]);
        }
        dist = (dpart[0] + dpart[1]) + (dpart[2] + dpart[3]);
      }
      double Wp;
      const double Kp = kprof_s2_w<decltype(pf)::value>(dist, ts, &Wp) + (i == j ? kp.eps : 0.0);
      const double mk = mv * Kp;
      mks[c][threadIdx.x] = decltype(pf)::value == 0 ? mk : mv * Wp;  // phase 2's weight
      acc_s += mk;
    }
    });
    }
    for (int o = 32; o > 0; o >>= 1) acc_s += __shfl_xor(acc_s, o);
    if (per) {
      // phase 2, Periodic: both sums (acc[k], acc[GP + k]) of GP dimensions at a time
      for (int k0 = 0; k0 < d; k0 += GP) {
        const int kn = min(GP, d - k0);  // wave-uniform
        double xr[GP], cr[GP], sr[GP], acc[2 * GP];
#pragma unroll
        for (int k = 0; k < GP; ++k) {
          xr[k] = k < kn ? xrow[k0 + k] : 0.0;
          cr[k] = k < kn ? crow[k0 + k] : 0.0;
          sr[k] = k < kn ? crow[d + k0 + k] : 0.0;
          acc[k] = acc[GP + k] = 0.0;
        }
#pragma unroll 1
        for (int c = 0; c < 16; ++c) {
          const int j = min(j0 + wv + 4 * c, n - 1);
          const double* xc = X + (size_t)j * d + k0;
          const double* cc = csp + (size_t)j * de + k0;
          const double mk = mks[c][threadIdx.x];
#pragma unroll
          for (int k = 0; k < GP; ++k) {
            const double cb = k < kn ? cc[k] : 0.0, sb = k < kn ? cc[d + k] : 0.0;
            const double r = xr[k] - (k < kn ? xc[k] : 0.0);
            const double dc = cr[k] - cb, ds = sr[k] - sb;
            acc[k] = fma(mk, fma(dc, dc, ds * ds), acc[k]);
            acc[GP + k] = fma(mk * r, fma(sr[k], cb, -(cr[k] * sb)), acc[GP + k]);
          }
        }
        // slot 0 of the part (S_sigma) with the first chunk, then this chunk's kn + kn sums
        grad_reduce(g.lane, g.wv, acc_s, acc, red, k0 ? 1 : 0, 1 + 2 * GP, out, [&](int t) {
          const int k = (t - 1) % GP;
          return t == 0 ? 0 : k >= kn ? -1 : t <= GP ? 1 + k0 + k : 1 + d + k0 + k;
        });
      }
      out += 2 * d + 1;
      continue;
    }
    // phase 2: the length-scale sums, GW dimensions at a time
    for (int k0 = 0; k0 < d; k0 += GW) {
      const int kn = min(GW, d - k0);  // wave-uniform
      double xr[GW], acc_l[GW];
#pragma unroll
      for (int k = 0; k < GW; ++k) {
        xr[k] = k < kn ? xrow[k0 + k] : 0.0;
        acc_l[k] = 0.0;
      }
#pragma unroll 1
      for (int c = 0; c < 16; ++c) {
        const int j = min(j0 + wv + 4 * c, n - 1);
        const double* xc = X + (size_t)j * d + k0;
        const double mk = mks[c][threadIdx.x];
#pragma unroll
        for (int k = 0; k < GW; ++k) {
          const double r = xr[k] - (k < kn ? xc[k] : 0.0);
          acc_l[k] = fma(mk, r * r, acc_l[k]);
        }
      }
      // slot 0 of the part (S_sigma) with the first chunk, then this chunk's kn sums
      grad_reduce(g.lane, g.wv, acc_s, acc_l, red, k0 ? 1 : 0, kn + 1, out,
                  [&](int t) { return t ? k0 + t : 0; });
    }
    out += d + 1;
  }
  grad_store_wn(g, red, out);
}

// out[slot] = sum_b partial[b][slot]  (fixed order)
__global__ void reduce_partials_kernel(const double* __restrict__ partial, int nblk, int nslot,
                                       double* __restrict__ out) {
  __shared__ double red[256];
  const int slot = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) s += partial[(size_t)b * nslot + slot];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[slot] = red[0];
}

// The gradient pass of one description into partial[nblk][nslot]: a Periodic part takes the wide
// kernel's PER form on the unit features cs; else the kernel compiled for the next D >= d (EXACT
// where d == D) up to d = 32, the wide kernel above.
template <bool MIX>
void launch_grad_pass(gpr_ctx* ctx, const KParams& kp, const double* X, const double* cs, int n,
                      const double* Kinv, int ldk, const double* alpha, double* partial, int nslot,
                      long long nblk) {
  const int d = kp.d;
  const unsigned grid = (unsigned)nblk;
  auto tiles = [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    auto* k = d == D ? &mll_grad_tiles_kernel<D, true, MIX> : &mll_grad_tiles_kernel<D, false, MIX>;
    k<<<grid, 256, 0, ctx->stream>>>(kp, X, n, Kinv, (size_t)ldk, alpha, partial, nslot);
  };
  if (kp.prod) {  // (a product term: the wide kernel's PROD form, profiles at run time)
    if constexpr (MIX) {
      auto* k = kp.nper ? &mll_grad_wide_kernel<true, true, true> : &mll_grad_wide_kernel<true, false, true>;
      k<<<grid, 256, 0, ctx->stream>>>(kp, X, kp.nper ? cs : nullptr, n, Kinv, (size_t)ldk, alpha,
                                       partial, nslot);
    }
  } else if (kp.nper)
    mll_grad_wide_kernel<MIX, true><<<grid, 256, 0, ctx->stream>>>(kp, X, cs, n, Kinv, (size_t)ldk,
                                                                    alpha, partial, nslot);
  else if (d <= 2) tiles(std::integral_constant<int, 2>{});
  else if (d <= 4) tiles(std::integral_constant<int, 4>{});
  else if (d <= 8) tiles(std::integral_constant<int, 8>{});
  else if (d <= 16) tiles(std::integral_constant<int, 16>{});
  else if (d <= 32) tiles(std::integral_constant<int, 32>{});
  else
    mll_grad_wide_kernel<MIX, false><<<grid, 256, 0, ctx->stream>>>(kp, X, nullptr, n, Kinv,
                                                                     (size_t)ldk, alpha, partial, nslot);
}

}  // namespace

// The host part of the fused gradient: launch, fixed-order reduction, assembly in hp order, log
// scale.  Shared by gpr_mll_grad (M = K^{-1}, a = alpha) and gpr_loo_grad (loo.hip: a = 0 and its
// own weight matrix); the kernels and their template arguments are the same for both.
int weighted_dk_sums(gpr_ctx* ctx, const KParams& kp, int D, const int* kinds, int nk,
                     const double* hp, int d, const double* dX, int n, const double* dKinv, int ldk,
                     const double* dalpha, int log_scale, double* grad) {
  const int nt = (n + GT - 1) / GT;
  const long long nblk = (long long)nt * (nt + 1) / 2;
  // per stationary part its hp width (d + 1; Periodic 2d + 1), then the WhiteNoise slot
  const int nslot = kp.nse * (d + 1) + kp.nper * d + 1;
  GPR_TRY(ensure_buf(ctx, ctx->dscratch, (size_t)nblk * nslot + nslot + 64));
  double* partial = ctx->dscratch;
  double* sums = ctx->dscratch + (size_t)nblk * nslot;
  {
    TimerScope ts(ctx, TC_OTHER, 0.0);
    if (kp.nper) GPR_TRY(launch_embed_unit(ctx, kp, dX, n));  // (into ctx->dxs)
    kmix_dispatch(kp.mix || kp.prod, [&](auto mix) {
      launch_grad_pass<decltype(mix)::value>(ctx, kp, dX, ctx->dxs, n, dKinv, ldk, dalpha, partial,
                                             nslot, nblk);
    });
    LAUNCH_CHECK(ctx);
  }
  reduce_partials_kernel<<<nslot, 256, 0, ctx->stream>>>(partial, (int)nblk, nslot, sums);
  LAUNCH_CHECK(ctx);
  std::vector<double> s(nslot);
  HIP_TRY(ctx, hipMemcpyAsync(s.data(), sums, nslot * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // assemble in hp order (kinds order)
  int off = 0, so = 0;
  for (int t = 0; t < nk; ++t) {
    if (kinds[t] == GPR_MUL) continue;  // (a marker owns neither hp nor slots)
    if (kinds[t] != GPR_WN) {
      const double* ss = s.data() + so;
      const double sig = hp[off];
      grad[off] = -0.5 * (2.0 / std::fabs(sig)) * ss[0];
      for (int k = 0; k < d; ++k) grad[off + 1 + k] = -0.5 * (-2.0 * hp[off + 1 + k]) * ss[1 + k];
      if (kinds[t] == GPR_PER)  // dK/dp_k = (4 pi l_k^2 / p_k^2) K r_k sin(2 pi r_k / p_k)
        for (int k = 0; k < d; ++k) {
          const double l = hp[off + 1 + k], pk = hp[off + 1 + d + k];
          grad[off + 1 + d + k] = -0.5 * (4.0 * M_PI * l * l / (pk * pk)) * ss[1 + d + k];
        }
      off += kind_hp_width(kinds[t], d);
      so += kind_hp_width(kinds[t], d);
    } else {
      // every WhiteNoise part's gradient is 2 sigma_n I (src/deriv_covar.jl:31-32)
      grad[off] = -0.5 * (2.0 * hp[off]) * s[nslot - 1];
      off += 1;
    }
  }
  if (log_scale)
    for (int i = 0; i < D; ++i) grad[i] *= hp[i];
  return 0;
}

extern "C" {

int gpr_mll(gpr_ctx_t ctx, const double* dU, int n, int ldu, const double* dy,
            const double* dalpha, double* out) {
  if (n <= 0 || ldu < n || !dU || !dy || !dalpha || !out) return set_err(ctx, GPR_E_ARG, "bad args");
  GPR_TRY(ensure_buf(ctx, ctx->dscratch, 64));
  mll_terms_kernel<<<1, 1024, 0, ctx->stream>>>(dU, (size_t)ldu, n, dy, dalpha, ctx->dscratch);
  LAUNCH_CHECK(ctx);
  double h[2];
  HIP_TRY(ctx, hipMemcpyAsync(h, ctx->dscratch, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *out = 0.5 * (h[0] + 2.0 * h[1] + (double)n * std::log(2.0 * M_PI));
  return 0;
}

int gpr_mll_grad(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                 const double* dX, int n, const double* dKinv, int ldk, const double* dalpha,
                 double eps, int log_scale, double* grad) {
  KParams kp;
  int D = 0;
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, eps, &kp, &D));
  if (n <= 0 || ldk < n || !dX || !dKinv || !dalpha || !grad) return set_err(ctx, GPR_E_ARG, "bad args");
  return weighted_dk_sums(ctx, kp, D, kinds, nk, hp, d, dX, n, dKinv, ldk, dalpha, log_scale, grad);
}

}  // extern "C"
