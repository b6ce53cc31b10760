// Matrix-free hyper-parameter gradients on gfx950: the bilinear form
//     g_j = sum_ab (A B^T)_ab dK_ab/dtheta_j        for all D hyper-parameters in one pass,
// A and B skinny n x r factors, with neither K, nor dK, nor the n x n weight M = A B^T stored --
// and on top of it the negative log-marginal-likelihood gradient from conjugate-gradient solves
// alone (gpr_mll_grad_free, at the end of this file).
//
// What is summed.  For a stationary part p with value K_p and W_p = -dK_p/dD (kexp.hpp):
//     dK/dsigma_p = (2 / |sigma_p|) (K_p + eps I)       ->  S_sigma,p = sum M o (K_p + eps I)
//     dK/dl_p,k   = -(2 / l_k) W_p (y_ak - y_bk)^2       ->  S_l,pk    = sum M o W_p (y_ak - y_bk)^2
//     dK/dsigma_n = 2 sigma_n I                          ->  S_n       = sum_a M_aa
// y = l .* x - c being the centred, scaled points the Gram form of the distance is built from
// (gram_tile.hpp).  The fused dense pass (mll.hip) forms (x_ak - x_bk)^2 per pair and dimension on
// the vector ALU.  Here the length-scale sums go to the matrix pipe by the separation the Gram
// form uses for the distance itself: with G = M o W_p,
//     sum_ab G_ab (y_ak - y_bk)^2 = sum_a y_ak^2 (G 1)_a + sum_a (G Y.^2)_ak - 2 sum_a y_ak (G Y)_ak,
// so a tile of G goes straight from registers into a second FP64 MFMA against V = [Y | Y.^2],
// kmatmul.hip's operand arrangement: the tile's rows are the summed points b, its columns the
// points a a lane keeps, register q of a 16 x 16 block is k-step q's B operand, and the A operand
// comes from the staged V block.  The per-point dots with y_a and y_a^2 are taken once, at the end
// of a workgroup's slab.  The diagonal's terms are exact zeros (y_a - y_a) and are dropped.
//
// Work split, as kmatmul: a workgroup of 4 waves owns 64 points a and one slab of 64-point row
// blocks b, wave w the tile quadrant (rows 32 (w & 1), columns 32 (w >> 1)); grid (ceil(n / 64),
// slabs).  Per tile:
//   1. M_tile = B_block A_block^T by v_mfma_f64_16x16x4 over r in k-steps of 4 (zero past r).
//      Both operands are (point l & 15, factor column 4 s + (l >> 4)), so the result lands in the
//      layout the distance chain leaves -- lane l, register q <-> row 16 rb + 4 q + (l >> 4),
//      column 16 cb + (l & 15) -- and the elementwise products below move no data.  The A-side
//      block (fixed for the workgroup) keeps its first 16 factor columns in registers for the
//      whole slab, which is all of it for r <= 16 (the default 15 probes + alpha); the B-side
//      block's first 16 columns are fetched one tile ahead, into the registers the weight tile
//      has just consumed, so the fetch runs under the exponentials.  Wider factors walk the rest
//      per tile in chunks of 16 columns read in operand order (128-byte runs; an element has
//      two readers, so LDS would buy nothing, and 64 x r does not fit it for r = n + 1).  (32
//      columns a side in registers, as first planned, do not fit 256 registers beside H, M and
//      the tile: the report below.)
//      M is made once per tile and serves every part.
//   2. per part: -D by the Gram-form MFMA chain from the prepared operands (kgf_neg_dist: the
//      chain of gram_tile, which sums the parts and so cannot be called here), K_p and W_p by
//      kprof_s2_w, S_sigma,p and the row sums (G 1)_a as per-lane sums (a lane's column a is
//      the same for all of a block's registers), G in place of -D, then H_p^T += V_p^T G.
//      V_p's 64 rows are staged in LDS column by column (stride 66 doubles); the next block's
//      values are fetched before the parts are walked and written after the products.
// A launch takes PG = 4 / NVB parts with NVB = 1, 2, 4 blocks of 16 columns of V per part (2d <=
// 16, 32, 64), so H is 32 accumulator registers whatever d is; more parts go in groups of PG, and
// more than 32 dimensions repeat the pass per 32 dimensions (64 columns of V) with the
// exponentials recomputed -- at d > 32 the distance chain is as long as the exponentials, and a
// pass that kept G would have to store it.
// At the slab's end the two waves that share output points add H and the row sums through LDS,
// eight threads per slot take the per-point dots in a fixed order, and the workgroup writes its
// slots to workspace; kgf_reduce_kernel adds the workgroups' slots in a fixed order.  No atomics:
// two calls agree bit for bit.  Slabs: GPR_KGF_SLABS, else the fewest that give two workgroups
// per CU (<= 64).  S_n is a dot of A's and B's rows by a small kernel of its own.
//
// Memory: the product's scaled points and operands, n_wg (nse (d + 1) + 1) doubles of partial
// slots with n_wg = ceil(n / 64) slabs <= max(n / 64, 2 CUs + n / 64): linear in n.
// Registers (compiler report, two workgroups per CU): every instance sits at 256 VGPRs and spills
// -- 188-220 bytes a lane for SquaredExp-only descriptions at d <= 8, 368 with a Matern part,
// 448-508 at run-time S.  Which values spill has not been looked at; it is the first thing to tune.
// Not done: K(x, x) is evaluated in full (no symmetry saving); Periodic parts and product terms
// are refused (their derivatives with respect to p and the cofactors are separable too).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "common.hpp"
#include "gram_tile.hpp"
#include "kexp.hpp"

namespace {

constexpr int KGF_VS = KT + 2;  // LDS stride (doubles) between the staged V block's columns
constexpr int KGF_MAXS = 64;    // most slabs of one launch
constexpr int KGF_RC = 4;       // k-steps (of 4 factor columns) per chunk of r
typedef double kgv2 __attribute__((ext_vector_type(2)));

// -D of part p for the tile (rows i0.., columns j0..) into acc: gram_tile's chain for one part
// (same operands, same k order: the distance is bit for bit the K assembly's).
template <int SC>
__device__ __forceinline__ void kgf_neg_dist(int S, const double* __restrict__ gR,
                                             const double* __restrict__ gC,
                                             const double* __restrict__ nR,
                                             const double* __restrict__ nC, int nblk, int p, int i0,
                                             int j0, gd4 (&acc)[2][2]) {
  constexpr int NOP = SC > 0 ? SC : GR_CH;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ba = (i0 >> 4) + 2 * (w & 1), bb = (j0 >> 4) + 2 * (w >> 1);
  const double* Ap = gR + ((size_t)p * nblk + ba) * S * 64 + lane;
  const double* Bp = gC + ((size_t)p * nblk + bb) * S * 64 + lane;
  const double* nAp = nR + (size_t)p * nblk * 16 + ba * 16 + (lane >> 4);
  const double* nBp = nC + (size_t)p * nblk * 16 + bb * 16 + (lane & 15);
  auto load_ops = [&](int ch, int h, double (&a)[2][NOP], double (&b)[2][NOP]) {
#pragma unroll
    for (int s = 0; s < NOP; ++s) {
      const int st = NOP * ch + s;
      const bool in = st < S;
      a[h][s] = in ? Ap[((size_t)h * S + st) * 64] : 0.0;
      b[h][s] = in ? Bp[((size_t)h * S + st) * 64] : 0.0;
    }
  };
  double a[2][NOP], b[2][NOP], nr[2][4], nc[2];
  load_ops(0, 0, a, b);
  load_ops(0, 1, a, b);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int q = 0; q < 4; ++q) nr[h][q] = nAp[16 * h + 4 * q];
    nc[h] = nBp[16 * h];
  }
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
}

// Factor columns 16 ch + [0, 16) of the 32 points from p0 on, in MFMA operand order: o[h][s] of
// lane l = F[point p0 + 16 h + (l & 15), column 16 ch + 4 s + (l >> 4)], zero past n or r (and
// nothing past them is read: a padded leading dimension may hold anything).
__device__ __forceinline__ void kgf_load_fac(const double* __restrict__ F, size_t ld, int n, int r,
                                             int p0, int ch, double (&o)[2][KGF_RC]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int s = 0; s < KGF_RC; ++s) {
      const int pt = p0 + 16 * h + (lane & 15), c = 4 * (KGF_RC * ch + s) + (lane >> 4);
      o[h][s] = (pt < n && c < r) ? F[(size_t)c * ld + pt] : 0.0;
    }
}

// This thread's share of the V block of rows [j0, j0 + 64): the row pair 2 (t & 31) of the four
// (part, dimension) pairs (t >> 5) + 8 k -- y of part pair / W, dimension k0 + pair % W; zero past
// n, d or the launch's parts.
template <int NVB>
__device__ __forceinline__ void kgf_fetch_v(const KParams& kp, const double* __restrict__ xs,
                                            const double* __restrict__ cen, int n, int k0, int j0,
                                            kgv2 (&r)[4]) {
  constexpr int W = 8 * NVB;
  const int j = j0 + 2 * (int)(threadIdx.x & 31), cg = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int pr = cg + 8 * k, g = pr / W, dim = k0 + pr % W;
    kgv2 e = {0.0, 0.0};
    if (g < kp.nse && dim < kp.d && j < n) {
      const double c = cen[g * kp.d + dim];
      const double* src = xs + ((size_t)g * n + j) * kp.d + dim;
      e[0] = src[0] - c;
      if (j + 1 < n) e[1] = src[kp.d] - c;
    }
    r[k] = e;
  }
}

// ... into LDS: column g 2W + w holds y, column g 2W + W + w its square
template <int NVB>
__device__ __forceinline__ void kgf_stage_v(const kgv2 (&r)[4], double* Vs) {
  constexpr int W = 8 * NVB;
  const int rp = threadIdx.x & 31, cg = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int pr = cg + 8 * k, col = (pr / W) * 2 * W + pr % W;
    *reinterpret_cast<kgv2*>(Vs + col * KGF_VS + 2 * rp) = r[k];
    *reinterpret_cast<kgv2*>(Vs + (col + W) * KGF_VS + 2 * rp) = r[k] * r[k];
  }
}

// gR / nrmR: the prepared operands (x 1) and norms of the points as the tile's rows b; gC / nrmC:
// (x 2) as its columns a -- all from the launch's first part on, as xs (scaled points) and cen
// (centres).  partial: this launch's slots, [workgroup][nslot] from the first part's S_sigma on.
// Dimensions [k0, k0 + 8 NVB) of every part; S_sigma is written by the pass with k0 = 0.
template <int SC, bool MIX, int NVB>
__global__ __launch_bounds__(256, 2) void kgradform_kernel(
    KParams kp, int Srt, const double* __restrict__ gR, const double* __restrict__ gC,
    const double* __restrict__ nrmR, const double* __restrict__ nrmC, int nblk, int n,
    int slab_blocks, const double* __restrict__ xs, const double* __restrict__ cen, int k0,
    const double* __restrict__ Af, size_t lda, const double* __restrict__ Bf, size_t ldb, int r,
    double* __restrict__ partial, int nslot) {
  constexpr int W = 8 * NVB, PG = 4 / NVB;
  __shared__ double Vs[64 * KGF_VS];  // V: PG parts x 16 NVB columns; at the end H (64 x 64)
  __shared__ double tabs[256 * PG];
  __shared__ double rsum_s[2][PG][64];
  __shared__ double ssig_s[4][PG];
  const int S = SC > 0 ? SC : Srt;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wr = w & 1, wc = w >> 1;
  const int i0 = blockIdx.x * KT;
  const int jb_lo = blockIdx.y * slab_blocks;
  const int jb_hi = min(jb_lo + slab_blocks, (n + KT - 1) / KT);
  const int d = kp.d;
  load_part_tables(kp, tabs);

  gd4 H[PG][NVB][2];
  double rs[PG][2], ss[PG];
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    ss[g] = 0.0;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      rs[g][cb] = 0.0;
#pragma unroll
      for (int vb = 0; vb < NVB; ++vb) H[g][vb][cb] = gd4{0.0, 0.0, 0.0, 0.0};
    }
  }
  double ar[2][KGF_RC], bq[2][KGF_RC];
  kgf_load_fac(Af, lda, n, r, i0 + 32 * wc, 0, ar);
  kgf_load_fac(Bf, ldb, n, r, jb_lo * KT + 32 * wr, 0, bq);
  kgv2 vr[4];
  kgf_fetch_v<NVB>(kp, xs, cen, n, k0, jb_lo * KT, vr);
  kgf_stage_v<NVB>(vr, Vs);
  __syncthreads();  // V and the tables

  for (int jb = jb_lo; jb < jb_hi; ++jb) {
    const int j0 = jb * KT;
    const bool more = jb + 1 < jb_hi;
    if (more) kgf_fetch_v<NVB>(kp, xs, cen, n, k0, j0 + KT, vr);  // lands under the tile
    // the weight tile M = B_block A_block^T
    gd4 M[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) M[rb][cb] = gd4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < KGF_RC; ++s)
      if (4 * s < r) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
            M[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(bq[rb][s], ar[cb][s], M[rb][cb], 0, 0, 0);
      }
    // the next block's first chunk into the registers just consumed: under the exponentials
    if (more) kgf_load_fac(Bf, ldb, n, r, j0 + KT + 32 * wr, 0, bq);
    for (int ch = 1; 4 * KGF_RC * ch < r; ++ch) {
      double a2[2][KGF_RC], b2[2][KGF_RC];
      kgf_load_fac(Af, lda, n, r, i0 + 32 * wc, ch, a2);
      kgf_load_fac(Bf, ldb, n, r, j0 + 32 * wr, ch, b2);
#pragma unroll
      for (int s = 0; s < KGF_RC; ++s)
        if (4 * (KGF_RC * ch + s) < r) {
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
              M[rb][cb] =
                  __builtin_amdgcn_mfma_f64_16x16x4f64(b2[rb][s], a2[cb][s], M[rb][cb], 0, 0, 0);
        }
    }
    const bool dtile = j0 == i0 && wr == wc;  // this wave's quadrant holds K's diagonal
#pragma unroll 1
    for (int p = 0; p < kp.nse; ++p) {
      gd4 acc[2][2];
      kgf_neg_dist<SC>(S, gR, gC, nrmR, nrmC, nblk, p, j0, i0, acc);
      const double* ts = tabs + 256 * p;
      double s_loc = 0.0, r_loc[2] = {0.0, 0.0};
      kprof_dispatch<MIX>(MIX ? kp.prof[p] : 0, [&](auto pf) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const bool on_diag = dtile && rb == cb && (lane >> 4) + 4 * q == (lane & 15);
              const double x = on_diag ? 0.0 : acc[rb][cb][q];  // -D
              double Wv;
              double Kv = kprof_s2_w<decltype(pf)::value>(-x, ts, &Wv);
              if (on_diag) Kv += kp.eps;
              const double m = M[rb][cb][q];
              s_loc = fma(m, Kv, s_loc);
              const double g = on_diag ? 0.0 : m * Wv;  // (y_a - y_a)^2 = 0 exactly
              r_loc[cb] += g;
              acc[rb][cb][q] = g;
              if ((q + 1) % GRAM_EXPG == 0) __builtin_amdgcn_sched_barrier(0);
            }
      });
      // H_p^T += V_p^T G: register q of block (rb, cb) is k-step q's B operand
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int g = 0; g < PG; ++g)
        if (p == g) {
          ss[g] += s_loc;
          rs[g][0] += r_loc[0];
          rs[g][1] += r_loc[1];
          const double* va = Vs + (g * 2 * W + (lane & 15)) * KGF_VS + 32 * wr + (lane >> 4);
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int vb = 0; vb < NVB; ++vb) {
                const double a = va[16 * vb * KGF_VS + 16 * rb + 4 * q];
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
                  H[g][vb][cb] =
                      __builtin_amdgcn_mfma_f64_16x16x4f64(a, acc[rb][cb][q], H[g][vb][cb], 0, 0, 0);
              }
        }
    }
    __syncthreads();  // the block's V is read
    if (more) kgf_stage_v<NVB>(vr, Vs);
    __syncthreads();
  }

  // ---- the slab's end: per-wave sums, the two row halves through LDS, the per-point dots ----
#pragma unroll
  for (int g = 0; g < PG; ++g) {
    double s = ss[g];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) ssig_s[w][g] = s;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      double v = rs[g][cb];  // the wave's 32 rows: the four lane groups hold rows (l >> 4) + 4 q
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (lane < 16) rsum_s[wr][g][32 * wc + 16 * cb + lane] = v;
    }
  }
  // Hs[(g 16 NVB + v) 64 + a], v = 16 vb + (l >> 4) + 4 q the column of V, a the point
  double* Hs = Vs;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if (wr == 1 - pass) {
#pragma unroll
      for (int g = 0; g < PG; ++g)
#pragma unroll
        for (int vb = 0; vb < NVB; ++vb)
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              double* dst = Hs + (g * 16 * NVB + 16 * vb + (lane >> 4) + 4 * q) * 64 + 32 * wc +
                            16 * cb + (lane & 15);
              *dst = pass ? H[g][vb][cb][q] + *dst : H[g][vb][cb][q];  // rows 0..31 + rows 32..63
            }
    }
    __syncthreads();
  }
  // slot (g, k0 + kk) by the eight threads 8 (g W + kk) + [0, 8): points sub + 8 i in order, then
  // a fixed tree over sub
  {
    const int sidx = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const int g = sidx / W, kk = sidx % W, dim = k0 + kk;
    const bool valid = g < kp.nse && dim < d;
    double sum = 0.0;
    if (valid) {
      const double c = cen[g * d + dim];
      for (int i = 0; i < 8; ++i) {
        const int a = sub + 8 * i, pt = i0 + a;
        if (pt < n) {
          const double y = xs[((size_t)g * n + pt) * d + dim] - c;
          const double rsv = rsum_s[0][g][a] + rsum_s[1][g][a];
          const double hy = Hs[(g * 2 * W + kk) * 64 + a], hy2 = Hs[(g * 2 * W + W + kk) * 64 + a];
          sum += fma(y * y, rsv, hy2) - 2.0 * (y * hy);
        }
      }
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    sum += __shfl_xor(sum, 4);
    double* out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * nslot;
    if (valid && sub == 0) out[g * (d + 1) + 1 + dim] = sum;
    if (k0 == 0 && (int)threadIdx.x < kp.nse)
      out[threadIdx.x * (d + 1)] = (ssig_s[0][threadIdx.x] + ssig_s[1][threadIdx.x]) +
                                   (ssig_s[2][threadIdx.x] + ssig_s[3][threadIdx.x]);
  }
}

// part[blk] = this block's share of sum_a sum_c A_ac B_ac (each thread a fixed stride of rows,
// then a fixed tree)
__global__ __launch_bounds__(256) void kgf_trace_kernel(const double* __restrict__ Af, size_t lda,
                                                        const double* __restrict__ Bf, size_t ldb,
                                                        int n, int r, double* __restrict__ part) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    for (int c = 0; c < r; ++c) s = fma(Af[(size_t)c * lda + i], Bf[(size_t)c * ldb + i], s);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// out[slot] = sum over the workgroups (slab by slab) of partial[wg][slot], fixed order
__global__ __launch_bounds__(256) void kgf_reduce_kernel(const double* __restrict__ partial,
                                                         int nwg, int nslot,
                                                         double* __restrict__ out) {
  __shared__ double red[256];
  const int slot = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nwg; b += 256) s += partial[(size_t)b * nslot + slot];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[slot] = red[0];
}

// X[t] *= s, t < count
__global__ __launch_bounds__(256) void kgf_scale_kernel(double* __restrict__ X, size_t count,
                                                        double s) {
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < count;
       t += (size_t)gridDim.x * blockDim.x)
    X[t] *= s;
}

struct KgfLaunch {
  const KmmOps* o;
  int slabs, slab_blocks;
  const double *Af, *Bf;
  int lda, ldb, r;
  double* partial;
  int nslot;
};

// one pass: parts [p0, p0 + g.nse) (<= 4 / NVB), dimensions [k0, k0 + 8 NVB)
template <int SC, int NVB>
int kgf_launch(gpr_ctx* ctx, const KgfLaunch& L, const KParams& g, int p0, int k0) {
  const KmmOps& o = *L.o;
  const int S = o.S, n = o.na, d = o.kp.d;
  const size_t op = (size_t)p0 * o.nbA * S * 64, nr = (size_t)p0 * o.nbA * 16;
  const dim3 grid((unsigned)((n + KT - 1) / KT), (unsigned)L.slabs);
  kmix_dispatch(g.mix != 0, [&](auto mix) {
    kgradform_kernel<SC, decltype(mix)::value, NVB><<<grid, 256, 0, ctx->stream>>>(
        g, S, o.B + op, o.A + op, o.nrmB + nr, o.nrmA + nr, o.nbA, n, L.slab_blocks,
        o.xa + (size_t)p0 * n * d, ctx->dgc.p + (size_t)p0 * d, k0, L.Af, (size_t)L.lda, L.Bf,
        (size_t)L.ldb, L.r, L.partial + (size_t)p0 * (d + 1), L.nslot);
  });
  LAUNCH_CHECK(ctx);
  return 0;
}

template <int SC, int NVB>
int kgf_passes(gpr_ctx* ctx, const KgfLaunch& L) {
  constexpr int W = 8 * NVB, PG = 4 / NVB;
  const KParams& kp = L.o->kp;
  for (int p0 = 0; p0 < kp.nse; p0 += PG) {
    const int cnt = std::min(PG, kp.nse - p0);
    const KParams g = kparams_group(kp, p0, cnt, 0);
    for (int k0 = 0; k0 < kp.d; k0 += W) GPR_TRY((kgf_launch<SC, NVB>(ctx, L, g, p0, k0)));
  }
  return 0;
}

// a Periodic part or a product marker: GPR_E_UNSUP, naming the part
int kgf_refuse(gpr_ctx* ctx, const int* kinds, int nk, const char* what) {
  if (!kinds) return 0;  // (make_kparams names it)
  for (int i = 0; i < nk; ++i)
    if (kinds[i] == GPR_PER || kinds[i] == GPR_MUL)
      return set_err(ctx, GPR_E_UNSUP,
                     "%s takes sums of SquaredExp, Matern and WhiteNoise parts: part %d is %s",
                     what, i + 1, kind_name(kinds[i]));
  return 0;
}

// grad[D] (host) = scale * the form, in hp order with gpr_mll_grad's conventions.  Synchronises.
int kgf_form(gpr_ctx* ctx, const KParams& kp, const int* kinds, int nk, const double* hp, int d,
             const double* dX, int n, const double* dA, int lda, const double* dB, int ldb, int r,
             int log_scale, double scale, double* grad) {
  KmmOps o;
  GPR_TRY(kmm_prepare(ctx, kp, dX, n, nullptr, n, GPR_SELF, &o));
  const int nta = (n + KT - 1) / KT;
  const int ncu = ctx->ncu > 0 ? ctx->ncu : 256;
  int slabs = ctx->kgf_slabs > 0 ? ctx->kgf_slabs : (2 * ncu + nta - 1) / nta;
  slabs = std::max(1, std::min(slabs, std::min(nta, KGF_MAXS)));
  const int slab_blocks = (nta + slabs - 1) / slabs;
  slabs = (nta + slab_blocks - 1) / slab_blocks;  // (no empty slab)
  const int nslot = kp.nse * (d + 1) + 1;
  const size_t nwg = (size_t)nta * slabs;
  const int ntr = std::max(1, std::min(256, (n + 1023) / 1024));
  // partial slots | the trace's partials | the sums
  GPR_TRY(ensure_buf(ctx, ctx->dkmm, nwg * nslot + 256 + nslot));
  double* partial = ctx->dkmm;
  double* tpart = partial + nwg * nslot;
  double* sums = tpart + 256;
  const KgfLaunch L{&o, slabs, slab_blocks, dA, dB, lda, ldb, r, partial, nslot};
  if (o.S == 1) GPR_TRY((kgf_passes<1, 1>(ctx, L)));
  else if (o.S == 2) GPR_TRY((kgf_passes<2, 1>(ctx, L)));
  else if (d <= 16) GPR_TRY((kgf_passes<0, 2>(ctx, L)));
  else GPR_TRY((kgf_passes<0, 4>(ctx, L)));
  kgf_trace_kernel<<<ntr, 256, 0, ctx->stream>>>(dA, (size_t)lda, dB, (size_t)ldb, n, r, tpart);
  kgf_reduce_kernel<<<nslot - 1, 256, 0, ctx->stream>>>(partial, (int)nwg, nslot, sums);
  kgf_reduce_kernel<<<1, 256, 0, ctx->stream>>>(tpart, ntr, 1, sums + nslot - 1);
  LAUNCH_CHECK(ctx);
  std::vector<double> s(nslot);
  HIP_TRY(ctx, hipMemcpyAsync(s.data(), sums, nslot * sizeof(double), hipMemcpyDeviceToHost,
                              ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // in hp order: dK/dsigma = (2 / |sigma|) (K_p + eps I), dK/dl_k = -(2 / l_k) W_p (y_ak - y_bk)^2
  // (= -2 l_k W_p (x_ak - x_bk)^2, gpr_mll_grad's), dK/dsigma_n = 2 sigma_n I for every WhiteNoise
  int off = 0, so = 0;
  for (int t = 0; t < nk; ++t) {
    if (kinds[t] != GPR_WN) {
      grad[off] = scale * (2.0 / std::fabs(hp[off])) * s[so];
      for (int k = 0; k < d; ++k) grad[off + 1 + k] = scale * (-2.0 / hp[off + 1 + k]) * s[so + 1 + k];
      off += d + 1;
      so += d + 1;
    } else {
      grad[off] = scale * (2.0 * hp[off]) * s[nslot - 1];
      off += 1;
    }
  }
  if (log_scale)
    for (int i = 0; i < off; ++i) grad[i] *= hp[i];
  return 0;
}

}  // namespace

extern "C" {

int gpr_kernel_grad_form(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                         const double* dX, int n, const double* dA, int lda, const double* dB,
                         int ldb, int r, double eps, int log_scale, double* grad) {
  GPR_TRY(kgf_refuse(ctx, kinds, nk, "gpr_kernel_grad_form"));
  KParams kp;
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, eps, &kp, nullptr));
  if (!dX) return set_err(ctx, GPR_E_ARG, "dX is NULL");
  if (!dA) return set_err(ctx, GPR_E_ARG, "dA is NULL");
  if (!dB) return set_err(ctx, GPR_E_ARG, "dB is NULL");
  if (!grad) return set_err(ctx, GPR_E_ARG, "grad is NULL");
  if (n < 1) return set_err(ctx, GPR_E_ARG, "n=%d < 1", n);
  if (r < 1) return set_err(ctx, GPR_E_ARG, "r=%d < 1", r);
  if (lda < n) return set_err(ctx, GPR_E_ARG, "lda=%d < n=%d", lda, n);
  if (ldb < n) return set_err(ctx, GPR_E_ARG, "ldb=%d < n=%d", ldb, n);
  return kgf_form(ctx, kp, kinds, nk, hp, d, dX, n, dA, lda, dB, ldb, r, log_scale, 1.0, grad);
}

int gpr_mll_grad_free(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                      const double* dX, int n, const double* dy, double eps, int m, int seed,
                      const double* dZ, double tol, int maxit, int log_scale, double* grad,
                      int* iters, double* relres) {
  GPR_TRY(kgf_refuse(ctx, kinds, nk, "gpr_mll_grad_free"));
  KParams kp;
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, eps, &kp, nullptr));
  if (!dX) return set_err(ctx, GPR_E_ARG, "dX is NULL");
  if (!dy) return set_err(ctx, GPR_E_ARG, "dy is NULL");
  if (!grad) return set_err(ctx, GPR_E_ARG, "grad is NULL");
  if (n < 1) return set_err(ctx, GPR_E_ARG, "n=%d < 1", n);
  if (m < 1) return set_err(ctx, GPR_E_ARG, "m=%d < 1", m);
  if (seed < 0) return set_err(ctx, GPR_E_ARG, "seed=%d < 0", seed);
  if (!(tol > 0.0)) return set_err(ctx, GPR_E_ARG, "tol=%g is not positive", tol);
  if (maxit < 0) return set_err(ctx, GPR_E_ARG, "maxit=%d < 0", maxit);
  const int r = 1 + m;
  const size_t nn = (size_t)n * r;
  // B = [y | Z] (then [alpha | Z]) and A = K^{-1} B (then [alpha | -U / m]), n x r each
  GPR_TRY(ensure_buf(ctx, ctx->dgf, 2 * nn));
  double* Bm = ctx->dgf;
  double* Am = Bm + nn;
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipMemcpyAsync(Bm, dy, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  if (dZ)
    HIP_TRY(ctx, hipMemcpyAsync(Bm + n, dZ, sizeof(double) * (size_t)n * m,
                                hipMemcpyDeviceToDevice, st));
  else
    GPR_TRY(gpr_randn(ctx, (uint64_t)seed, 0, Bm + n, (size_t)n * m));
  GPR_TRY(gpr_solve_cg(ctx, kinds, nk, hp, d, dX, n, Bm, r, n, eps, tol, maxit, Am, n, iters,
                       relres));
  HIP_TRY(ctx, hipMemcpyAsync(Bm, Am, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  const size_t cnt = (size_t)n * m;
  kgf_scale_kernel<<<(int)std::min<size_t>((cnt + 255) / 256, 4096), 256, 0, st>>>(Am + n, cnt,
                                                                                 -1.0 / m);
  LAUNCH_CHECK(ctx);
  // the CG call made its own description since: this call's tables again
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, eps, &kp, nullptr));
  return kgf_form(ctx, kp, kinds, nk, hp, d, dX, n, Am, n, Bm, n, r, log_scale, -0.5, grad);
}

}  // extern "C"
