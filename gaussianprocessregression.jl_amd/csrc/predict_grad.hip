// Gradients of the posterior mean and diagonal variance with respect to the test inputs, gfx950.
//
// With alpha = K^{-1} y and Q = K^{-1} K(x, xp) (n x m), summed over the stationary parts p:
//   d mu     / d xp_kj =      sum_p sum_i alpha_i (-W_p(xp_j, x_i)) dD_p/dxp_kj
//   d sigma2 / d xp_kj = -2   sum_p sum_i Q_ij    (-W_p(xp_j, x_i)) dD_p/dxp_kj
// W = -dk/dD of the part's profile (kexp.hpp), and on raw x with r_k = xp_kj - x_ki
//   SquaredExp / Matern:  dD/dxp_k = 2 l_k^2 r_k
//   Periodic:             dD/dxp_k = (4 pi l_k^2 / p_k) sin(2 pi r_k / p_k) = 2 l_k^2 (2 pi / p_k) sin(..)
// so both are ONE weighted cross-kernel reduction, never materialising a dK matrix,
//   G[k, j] = c sum_p sum_i w(i, j) W_p(xp_j, x_i) l_pk^2 f_pk(xp_j, x_i),   f = r_k or (2 pi / p_k) sin
// with w = alpha_i, c = -2 (mean) or w = Q_ij, c = 4 (variance).  A WhiteNoise part contributes
// nothing (the cross kernel has no noise); a Matern part at a coincident point has a finite W and
// r = 0.  The factors r_k and sin(2 pi r_k / p_k) are formed as differences per pair (sin(a - b) =
// sin a cos b - cos a sin b on the unit features of launch_embed_unit), never as x S_0 - S_k.
//
// Layout (modelled on mll.hip): a workgroup is 64 test points (lane = test point: its coordinates
// and its d sums in registers) times one slab of `slab` training points; wave wv takes the
// training points i0 + wv + 4c of every 64-point tile, wave-uniformly (scalar loads of the point).
// Q's 64 x 64 tile is read once, coalesced along i, and turned through LDS.  Every wave writes its
// own partial sums partial[(slab index, wave)][j][k] -- no atomics -- and pgrad_reduce_kernel adds
// the slots in a fixed order: two calls on the same inputs agree bit for bit.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "kexp.hpp"

namespace {

constexpr int PT = 64;   // tile edge: test points per workgroup, training points per tile
constexpr int PGW = 32;  // dimensions a thread holds at a time in the wide kernel
constexpr int PGP = 16;  // ... for a Periodic part (cos, sin and the sum per dimension)

// the exp tables sigma_p^2 2^(j/256) of the launch's (up to KMAXP) parts
__device__ __forceinline__ void pgrad_fill_tabs(const KParams& kp, double (*tabs)[256]) {
  for (int p = 0; p < min(kp.nse, KMAXP); ++p)
    tabs[p][threadIdx.x] = (kp.sig[p] * kp.sig[p]) * kp.exptab[threadIdx.x];
}

// Q[i0 + lane, j0 + wv + 4c], c < 16, of one tile into q[] (0 past i_end / m)
__device__ __forceinline__ void pgrad_load_q(const double* __restrict__ Q, size_t ldq, int i0,
                                             int i_end, int j0, int m, int lane, int wv,
                                             double (&q)[16]) {
  const int ii = i0 + lane;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const int jj = j0 + wv + 4 * c;
    q[c] = (ii < i_end && jj < m) ? Q[(size_t)ii + (size_t)jj * ldq] : 0.0;
  }
}

// d <= 32 without a Periodic part: the kernel compiled for the next D >= d (EXACT: d == D, no
// per-feature bound checks).  MIX as in mll.hip (SE-only descriptions launch MIX = false); QW:
// the weights are Q's (else alpha's, wave-uniform).  Rows past the slab's end are clamped to point
// n - 1 with zero weight, test points past m to point m - 1 and not stored.
template <int D, bool EXACT, bool MIX, bool QW>
__global__ __launch_bounds__(256) void pgrad_tiles_kernel(KParams kp, const double* __restrict__ X,
                                                          int n, const double* __restrict__ Xp,
                                                          int m, const double* __restrict__ wsrc,
                                                          size_t ldq, int slab,
                                                          double* __restrict__ partial) {
  __shared__ double tabs[KMAXP][256];
  __shared__ double qs[QW ? PT : 1][PT + 1];  // [test point][training point], conflict-free both ways
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int d = EXACT ? D : kp.d;
  const int j0 = blockIdx.x * PT;
  const int j = j0 + lane;
  const size_t jc = (size_t)min(j, m - 1);
  const int i_begin = blockIdx.y * slab;
  const int i_end = min(n, i_begin + slab);
  pgrad_fill_tabs(kp, tabs);

  double xr[D], acc[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    xr[k] = (EXACT || k < d) ? Xp[jc * d + k] : 0.0;
    acc[k] = 0.0;
  }
  double qn[16];
  if (QW) pgrad_load_q(wsrc, ldq, i_begin, i_end, j0, m, lane, wv, qn);
  __syncthreads();  // tabs

  for (int i0 = i_begin; i0 < i_end; i0 += PT) {
    if (QW) {
      __syncthreads();  // the previous tile has been read
#pragma unroll
      for (int c = 0; c < 16; ++c) qs[wv + 4 * c][lane] = qn[c];
      __syncthreads();
      // the next tile's loads in flight behind this tile's exponentials
      if (i0 + PT < i_end) pgrad_load_q(wsrc, ldq, i0 + PT, i_end, j0, m, lane, wv, qn);
    }
    for (int p = 0; p < kp.nse; ++p) {
      const double* ts = tabs[p];
      const double* l2p = kp.l2 + (size_t)p * d;
      double tacc[D];
#pragma unroll
      for (int k = 0; k < D; ++k) tacc[k] = 0.0;
      kprof_dispatch<MIX>(MIX ? __builtin_amdgcn_readfirstlane((int)kp.pf[p]) : 0, [&](auto pf) {
        // (not unrolled: the wave-uniform point loads stay scalar loads of one column)
#pragma unroll 1
        for (int c = 0; c < 16; ++c) {
          const int ir = i0 + wv + 4 * c;
          const int i = min(ir, n - 1);  // wave-uniform
          double w;
          if (QW) w = qs[lane][wv + 4 * c];
          else w = wsrc[i];
          if (ir >= i_end) w = 0.0;
          const double* xc = X + (size_t)i * d;
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
          (void)kprof_s2_w<decltype(pf)::value>(dist, ts, &Wp);
          const double gw = w * Wp;
#pragma unroll
          for (int k = 0; k < D; ++k) {
            if (EXACT || k < d) tacc[k] = fma(gw, xr[k] - xc[k], tacc[k]);
          }
        }
      });
#pragma unroll
      for (int k = 0; k < D; ++k) {
        if (EXACT || k < d) acc[k] = fma(l2p[k], tacc[k], acc[k]);
      }
    }
  }
  if (j < m) {
    double* out = partial + (((size_t)blockIdx.y * 4 + wv) * m + j) * d;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      if (EXACT || k < d) out[k] = acc[k];
    }
  }
}

// The same pass for any d and for a description with a Periodic part (PER).  Per tile and part,
// two phases as in mll_grad_wide_kernel:
//  1. each thread's 16 weights w W_p, the distance by a run-time loop over all d (test point from
//     global memory / L1, training point wave-uniform), into the thread's own LDS slots;
//  2. PGW = 32 dimensions at a time (Periodic: PGP = 16): the test point's features into
//     registers, the 16 weighted differences summed, and the chunk's sums added into the wave's
//     own partial slot in global memory (read and written by this thread alone, in program order).
// cs / csp: per part and training / test point the unit features [cos a_k | sin a_k], a_k =
// 2 pi x_k / p_k (embed_inputs_kernel's unit form; only Periodic parts' rows are read).
// PROD: the launch's group holds a product term (launched with MIX: profiles at run time; a
// term never straddles two groups).  Phase 1 evaluates every factor of part p's term [t0, t1]
// for the pair (kpair_dist), forms the cofactor C = prod_{g != p} K_g as a product and leaves
// w W_p C for phase 2, which is unchanged for both branches.
template <bool MIX, bool PER, bool QW, bool PROD = false>
__global__ __launch_bounds__(256) void pgrad_wide_kernel(KParams kp, const double* __restrict__ X,
                                                         const double* __restrict__ cs, int n,
                                                         const double* __restrict__ Xp,
                                                         const double* __restrict__ csp, int m,
                                                         const double* __restrict__ wsrc, size_t ldq,
                                                         int slab, double* __restrict__ partial) {
  __shared__ double tabs[KMAXP][256];
  __shared__ double qs[QW ? PT : 1][PT + 1];
  __shared__ double mks[16][256];  // w W_p of every thread's 16 training points
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int d = kp.dx, de = kp.de;
  const int j0 = blockIdx.x * PT;
  const int j = j0 + lane;
  const bool jrow = j < m;
  const size_t jc = (size_t)min(j, m - 1);
  const int i_begin = blockIdx.y * slab;
  const int i_end = min(n, i_begin + slab);
  const double* xrow = Xp + jc * d;
  double* out = partial + (((size_t)blockIdx.y * 4 + wv) * m + jc) * d;
  pgrad_fill_tabs(kp, tabs);
  __syncthreads();

  for (int i0 = i_begin; i0 < i_end; i0 += PT) {
    if (QW) {
      double q[16];
      pgrad_load_q(wsrc, ldq, i0, i_end, j0, m, lane, wv, q);
      __syncthreads();  // the previous tile has been read
#pragma unroll
      for (int c = 0; c < 16; ++c) qs[wv + 4 * c][lane] = q[c];
      __syncthreads();
    }
    for (int p = 0; p < kp.nse; ++p) {
      const bool fresh = i0 == i_begin && p == 0;  // the slot's first sums: stored, not added
      const double* ts = tabs[p];
      const double* l2p = kp.l2 + (size_t)p * d;
      const bool per = PER && __builtin_amdgcn_readfirstlane((int)kp.per[p]) != 0;
      const double* ctr = PER ? cs + (size_t)p * n * de : nullptr;
      const double* crow = PER ? csp + ((size_t)p * m + jc) * de : nullptr;
      // phase 1
      if constexpr (PROD) {
        int t0 = p, t1 = p;  // the part's term (kp.tendm: the group's mask, wave-uniform)
        while (t0 > 0 && !((kp.tendm >> (t0 - 1)) & 1)) --t0;
        while (t1 + 1 < kp.nse && !((kp.tendm >> t1) & 1)) ++t1;
#pragma unroll 1
        for (int c = 0; c < 16; ++c) {
          const int ir = i0 + wv + 4 * c;
          const int i = min(ir, n - 1);  // wave-uniform
          double w;
          if (QW) w = qs[lane][wv + 4 * c];
          else w = wsrc[i];
          if (ir >= i_end) w = 0.0;
          double Wp = 0.0, C = 1.0;
          for (int g = t0; g <= t1; ++g) {
            const bool perg = PER && __builtin_amdgcn_readfirstlane((int)kp.per[g]) != 0;
            const double dist = kpair_dist(perg, d, kp.l2 + (size_t)g * d, xrow, X + (size_t)i * d,
                                           PER ? csp + ((size_t)g * m + jc) * de : nullptr,
                                           PER ? cs + ((size_t)g * n + i) * de : nullptr);
            double Wg;
            const double Kg = kprof_s2_w_rt(kp.prof[g], dist, tabs[g], &Wg);
            if (g == p) Wp = Wg;
            else C *= Kg;
          }
          mks[c][threadIdx.x] = w * (Wp * C);
        }
      } else
      kprof_dispatch<MIX>(MIX ? __builtin_amdgcn_readfirstlane((int)kp.pf[p]) : 0, [&](auto pf) {
#pragma unroll 1
        for (int c = 0; c < 16; ++c) {
          const int ir = i0 + wv + 4 * c;
          const int i = min(ir, n - 1);  // wave-uniform
          double w;
          if (QW) w = qs[lane][wv + 4 * c];
          else w = wsrc[i];
          if (ir >= i_end) w = 0.0;
          double a0 = 0.0, a1 = 0.0;
          if (per) {
            // D = sum_k l_k^2 chord_k^2, chord_k^2 = (cos a - cos b)^2 + (sin a - sin b)^2
            const double* cc = ctr + (size_t)i * de;
            for (int k = 0; k < d; ++k) {
              const double dc = crow[k] - cc[k], ds = crow[d + k] - cc[d + k];
              const double t = fma(dc, dc, ds * ds);
              if (k & 1) a1 = fma(l2p[k], t, a1);
              else a0 = fma(l2p[k], t, a0);
            }
          } else {
            const double* xc = X + (size_t)i * d;
            for (int k = 0; k < d; ++k) {
              const double r = xrow[k] - xc[k];
              if (k & 1) a1 = fma(l2p[k], r * r, a1);
              else a0 = fma(l2p[k], r * r, a0);
            }
          }
          double Wp;
          (void)kprof_s2_w<decltype(pf)::value>(a0 + a1, ts, &Wp);
          mks[c][threadIdx.x] = w * Wp;
        }
      });
      // phase 2
      if (per) {
        const double* pkp = kp.pk + (size_t)p * d;
        for (int k0 = 0; k0 < d; k0 += PGP) {
          const int kn = min(PGP, d - k0);  // wave-uniform
          double cr[PGP], sr[PGP], tacc[PGP];
#pragma unroll
          for (int k = 0; k < PGP; ++k) {
            cr[k] = k < kn ? crow[k0 + k] : 0.0;
            sr[k] = k < kn ? crow[d + k0 + k] : 0.0;
            tacc[k] = 0.0;
          }
#pragma unroll 1
          for (int c = 0; c < 16; ++c) {
            const int i = min(i0 + wv + 4 * c, n - 1);
            const double* cc = ctr + (size_t)i * de + k0;
            const double gw = mks[c][threadIdx.x];
#pragma unroll
            for (int k = 0; k < PGP; ++k) {
              const double cb = k < kn ? cc[k] : 0.0, sb = k < kn ? cc[d + k] : 0.0;
              // sin(a - b) = sin a cos b - cos a sin b
              tacc[k] = fma(gw, fma(sr[k], cb, -(cr[k] * sb)), tacc[k]);
            }
          }
          if (jrow) {
#pragma unroll
            for (int k = 0; k < PGP; ++k) {
              if (k < kn) {
                const double v = (l2p[k0 + k] * (2.0 * M_PI / pkp[k0 + k])) * tacc[k];
                out[k0 + k] = fresh ? v : out[k0 + k] + v;
              }
            }
          }
        }
        continue;
      }
      for (int k0 = 0; k0 < d; k0 += PGW) {
        const int kn = min(PGW, d - k0);  // wave-uniform
        double xr[PGW], tacc[PGW];
#pragma unroll
        for (int k = 0; k < PGW; ++k) {
          xr[k] = k < kn ? xrow[k0 + k] : 0.0;
          tacc[k] = 0.0;
        }
#pragma unroll 1
        for (int c = 0; c < 16; ++c) {
          const int i = min(i0 + wv + 4 * c, n - 1);
          const double* xc = X + (size_t)i * d + k0;
          const double gw = mks[c][threadIdx.x];
#pragma unroll
          for (int k = 0; k < PGW; ++k) tacc[k] = fma(gw, xr[k] - (k < kn ? xc[k] : 0.0), tacc[k]);
        }
        if (jrow) {
#pragma unroll
          for (int k = 0; k < PGW; ++k) {
            if (k < kn) {
              const double v = l2p[k0 + k] * tacc[k];
              out[k0 + k] = fresh ? v : out[k0 + k] + v;
            }
          }
        }
      }
    }
  }
}

// out[e] = scale * sum_s partial[s][e], e < len, the slots in index order
__global__ __launch_bounds__(256) void pgrad_reduce_kernel(const double* __restrict__ partial,
                                                           int nslot, size_t len, double scale,
                                                           double* __restrict__ out) {
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < len;
       e += (size_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int t = 0; t < nslot; ++t) s += partial[(size_t)t * len + e];
    out[e] = scale * s;
  }
}

// One group of up to KMAXP parts into its partial slots: a Periodic part in the description, or
// d > 32, takes the wide kernel; else the kernel compiled for the next D >= d.
template <bool MIX, bool QW>
void launch_pgrad_group(gpr_ctx* ctx, const KParams& kp, const double* X, const double* cs, int n,
                        const double* Xp, const double* csp, int m, const double* wsrc, int slab,
                        int nslab, double* partial) {
  const int d = kp.dx;
  const dim3 grid((unsigned)((m + PT - 1) / PT), (unsigned)nslab);
  auto tiles = [&](auto dc) {
    constexpr int D = decltype(dc)::value;
    auto* k = d == D ? &pgrad_tiles_kernel<D, true, MIX, QW> : &pgrad_tiles_kernel<D, false, MIX, QW>;
    k<<<grid, 256, 0, ctx->stream>>>(kp, X, n, Xp, m, wsrc, (size_t)n, slab, partial);
  };
  if (kp.prod) {  // (a product term in the group: the wide kernel's PROD form)
    if constexpr (MIX) {
      auto* k = kp.nper ? &pgrad_wide_kernel<true, true, QW, true> : &pgrad_wide_kernel<true, false, QW, true>;
      k<<<grid, 256, 0, ctx->stream>>>(kp, X, kp.nper ? cs : nullptr, n, Xp, kp.nper ? csp : nullptr,
                                       m, wsrc, (size_t)n, slab, partial);
    }
  } else if (kp.nper)
    pgrad_wide_kernel<MIX, true, QW><<<grid, 256, 0, ctx->stream>>>(kp, X, cs, n, Xp, csp, m, wsrc,
                                                                   (size_t)n, slab, partial);
  else if (d <= 2) tiles(std::integral_constant<int, 2>{});
  else if (d <= 4) tiles(std::integral_constant<int, 4>{});
  else if (d <= 8) tiles(std::integral_constant<int, 8>{});
  else if (d <= 16) tiles(std::integral_constant<int, 16>{});
  else if (d <= 32) tiles(std::integral_constant<int, 32>{});
  else
    pgrad_wide_kernel<MIX, false, QW><<<grid, 256, 0, ctx->stream>>>(kp, X, nullptr, n, Xp, nullptr,
                                                                    m, wsrc, (size_t)n, slab, partial);
}

// G (d x m) = scale * the weighted reduction, weights alpha (n) or Q (n x m, ld n; qw): the
// parts in groups of KMAXP, every group into slots of its own, then the fixed-order sum.  cs /
// csp: the unit features of the training / test points (null without a Periodic part).
int pgrad_pass(gpr_ctx* ctx, const KParams& kp, const double* X, const double* cs, int n,
               const double* Xp, const double* csp, int m, const double* wsrc, bool qw, double scale,
               double* G, int timing_class) {
  const int d = kp.dx;
  const int slab = (std::max(ctx->pgrad_slab, PT) + PT - 1) / PT * PT;
  const int nslab = (n + slab - 1) / slab;
  // (groups of up to KMAXP parts, cut at term boundaries: a product term stays in one launch)
  std::vector<int> gp0;
  for (int p0 = 0; p0 < kp.nse; p0 += kparams_group_count(kp, p0)) gp0.push_back(p0);
  const int ngroup = (int)gp0.size();
  const size_t len = (size_t)m * d;
  const size_t per_group = (size_t)nslab * 4 * len;
  GPR_TRY(ensure_buf(ctx, ctx->dscratch, per_group * ngroup + 64));
  double* partial = ctx->dscratch;
  TimerScope ts(ctx, timing_class, 0.0);
  for (int g = 0; g < ngroup; ++g) {
    const int p0 = gp0[g];
    const KParams kg = kparams_group(kp, p0, kparams_group_count(kp, p0), 0);
    const double* csg = cs ? cs + (size_t)p0 * n * kp.de : nullptr;
    const double* cspg = csp ? csp + (size_t)p0 * m * kp.de : nullptr;
    kmix_dispatch(kg.mix || kg.prod, [&](auto mix) {
      constexpr bool MIX = decltype(mix)::value;
      if (qw)
        launch_pgrad_group<MIX, true>(ctx, kg, X, csg, n, Xp, cspg, m, wsrc, slab, nslab,
                                      partial + per_group * g);
      else
        launch_pgrad_group<MIX, false>(ctx, kg, X, csg, n, Xp, cspg, m, wsrc, slab, nslab,
                                       partial + per_group * g);
    });
    LAUNCH_CHECK(ctx);
  }
  const int blocks = (int)std::min<size_t>((len + 255) / 256, 65535);
  pgrad_reduce_kernel<<<blocks, 256, 0, ctx->stream>>>(partial, ngroup * nslab * 4, len, scale, G);
  LAUNCH_CHECK(ctx);
  return 0;
}

// *Q = K^{-1} B for B (n x m, ld n; overwritten) from the factor U.  potrs_core sweeps U once per
// pair of columns (m / 2 passes over the 4 n^2 bytes of the triangle: measured 26.7 s at n = 32768,
// m = 8192), so beyond a few columns the solve goes through the library's MFMA paths instead:
// Z = U^{-T} (the identity's solve, as gpr_potri_upper), V = U^{-T} B, Q = Z^T V -- n^3 / 3 +
// 3 n^2 m flops, n^2 + n m doubles of workspace in ctx->dbig, and *Q points there.  The sweeps
// cost ~4 n^2 m bytes of traffic, the products' fixed part n^3 / 3 flops: at the measured rates
// (~1.3 TB/s, ~60 TF/s) they cross at m ~ n / 500.  GPR_PGRAD_SOLVE forces either.
int pgrad_solve(gpr_ctx* ctx, const double* dU, int n, int ldu, double* B, int m, const double** Q) {
  TimerScope ts(ctx, TC_PGRAD_SOLVE, 0.0);
  const bool products = ctx->pgrad_solve >= 0 ? ctx->pgrad_solve != 0 : m > std::max(16, n / 512);
  *Q = B;
  if (!products) return potrs_core(ctx, dU, n, ldu, B, m, n);
  GPR_TRY(ensure_buf(ctx, ctx->dbig, (size_t)n * n + (size_t)n * m));
  double* Z = ctx->dbig;
  double* out = Z + (size_t)n * n;
  GPR_TRY(launch_set_identity(ctx, Z, n, n));
  GPR_TRY(trsm_ut_core(ctx, dU, n, ldu, Z, n, n, nullptr, 1));  // Z = U^{-T} (lower triangular)
  GPR_TRY(trsm_ut_core(ctx, dU, n, ldu, B, m, n, nullptr, 0));  // V = U^{-T} B
  GemmArgs g{};
  g.P = Z; g.ldp = n;
  g.Q = B; g.ldq = n;
  g.C = out; g.ldc = n;
  g.M = n; g.N = m; g.K = n;
  g.alpha = 1.0; g.beta = 0.0;
  GPR_TRY(launch_gemm_tn(ctx, g, TC_OTHER));  // Q = Z^T V = U^{-1} V
  *Q = out;
  return 0;
}

}  // namespace

extern "C" {

int gpr_predict_grad(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                     const double* dX, int n, const double* dU, int ldu, const double* dwt,
                     int nrhs, const double* dXp, int m, int want_var, double eps, double* dgmu,
                     double* dgvar, double* dwork) {
  KParams kp;
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, eps, &kp, nullptr));
  if (n <= 0) return set_err(ctx, GPR_E_ARG, "n=%d (needs n >= 1)", n);
  if (m <= 0) return set_err(ctx, GPR_E_ARG, "m=%d (needs m >= 1)", m);
  if (nrhs <= 0) return set_err(ctx, GPR_E_ARG, "nrhs=%d (needs nrhs >= 1)", nrhs);
  if (ldu < n) return set_err(ctx, GPR_E_ARG, "ldu=%d < n=%d", ldu, n);
  if (!dX || !dU || !dwt || !dXp)
    return set_err(ctx, GPR_E_ARG, "%s is NULL", !dX ? "dX" : !dU ? "dU" : !dwt ? "dwt" : "dXp");
  if (!dgmu) return set_err(ctx, GPR_E_ARG, "dgmu is NULL");
  if (want_var && !dgvar) return set_err(ctx, GPR_E_ARG, "dgvar is NULL (want_var != 0)");
  // Q = K^{-1} K(x, xp) first: the cross build leaves its own scaled points in the context's
  // point buffers, which the unit features of a Periodic part then replace.  Always the cross
  // kernel, also for dXp == dX (see the header)
  const double* Q = nullptr;
  if (want_var) {
    double* B = dwork;
    if (!B) {
      GPR_TRY(ensure_buf(ctx, ctx->dbig2, (size_t)n * m));
      B = ctx->dbig2;
    }
    GPR_TRY(launch_kernel_matrix(ctx, kp, dX, n, dXp, m, 0, B, n));
    GPR_TRY(pgrad_solve(ctx, dU, n, ldu, B, m, &Q));
  }
  const double *cs = nullptr, *csp = nullptr;
  if (kp.nper) {
    GPR_TRY(launch_embed_unit_to(ctx, kp, dX, n, ctx->dxs));
    GPR_TRY(launch_embed_unit_to(ctx, kp, dXp, m, ctx->dxps));
    cs = ctx->dxs;
    csp = ctx->dxps;
  }
  for (int c = 0; c < nrhs; ++c)
    GPR_TRY(pgrad_pass(ctx, kp, dX, cs, n, dXp, csp, m, dwt + (size_t)c * n, false, -2.0,
                       dgmu + (size_t)c * d * m, TC_PGRAD_MEAN));
  if (want_var)
    GPR_TRY(pgrad_pass(ctx, kp, dX, cs, n, dXp, csp, m, Q, true, 4.0, dgvar, TC_PGRAD_VAR));
  return 0;
}

}  // extern "C"
