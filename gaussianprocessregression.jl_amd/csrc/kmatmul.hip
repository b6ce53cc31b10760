// Matrix-free kernel products on gfx950: Out (na x nv) = K(xa, xb) V with K evaluated tile by
// tile in registers and never stored.
//
// Every path that multiplied by a kernel matrix wrote the matrix first: n m doubles for a
// posterior mean, n^2 for a fit.  Here a 64 x 64 tile of K exists only as the 16 accumulator
// registers per lane that gram_tile (gram_tile.hpp, the K assembly's own tile: every kind, product
// terms, any d, any number of parts) leaves, and those registers are, as they stand, the B operand
// of a second FP64 MFMA:
//
//   gram_tile leaves v[rb][cb][q] in lane l = tile element (row 16 rb + 4 q + (l >> 4),
//   col 16 cb + (l & 15)), and v_mfma_f64_16x16x4 takes B[k = l >> 4][n = l & 15].  With the
//   summed points xb on the tile's ROWS and the output points xa on its COLUMNS, register q of
//   block (rb, cb) is k-step q of the product
//       Out^T[vcol, xa col] += V^T[vcol, xb row] K[xb row, xa col],
//   whose A operand A[m = l & 15][k = l >> 4] = V[row 16 rb + 4 q + (l >> 4), vcol 16 vb + (l & 15)]
//   comes from the staged V block, and whose result D (lane l, register q' = vcol 16 vb + (l >> 4)
//   + 4 q', xa col 16 cb + (l & 15)) stores as 128-byte runs along Out's columns.
//
// So K takes no pass through LDS or memory.  An element is bit for bit the one gpr_kernel's Gram
// route writes for K(xa, xb): the operands are prepared by the same gram_prepare call (xa as the
// assembly's rows, xb as its columns), and gram_tile forms -D from the same products (2 y_a,k)
// y_b,k in the same k order whichever of the two operands sits on the tile's rows.  (The profiles
// round each operation on its own -- contraction is off in kprof_s2 and in gram_tile's element
// loop -- because the compiler fused 1 + a r of the Matern profiles here and not in the assembly's
// kernels; tests/test_gpu_kernel_matmul_bits.py compares the two bit for bit.)
//
// Work split.  A workgroup of 4 waves owns 64 output points and one slab of xb, which it walks in
// 64-point blocks; wave w evaluates the tile quadrant (rows 32 (w & 1), columns 32 (w >> 1)) and
// keeps Out^T accumulators for its 32 output points (16 NVB x 32, NVB = 1 or 4 blocks of 16
// columns of V) over the whole slab.  The two waves that share output points add their
// accumulators once at the end through LDS, wave 0's plus wave 1's.  V's 64 x 16 NVB block is
// staged in LDS column by column (stride 66 doubles: the operand reads of a half wave touch 64
// distinct banks); the next block's rows are fetched into registers (16-B loads where V allows
// them) before the tile is evaluated and written to LDS after the product, so the fetch runs under
// the exponentials.  Rows >= nb enter as exact zeros and are never read from memory; nv is padded
// to 16 NVB in LDS only.  Wider V repeats the pass per 64 columns.
// The grid is (ceil(na / 64), S slabs).  With S > 1 every slab writes its partial product to
// workspace and kmm_reduce_kernel adds the partials in slab order: no atomics, so two calls agree
// bit for bit.  S: GPR_KMM_SLABS, or by default the smallest count that gives two workgroups per
// CU.  More than KMAXP stationary parts: one pass per group of parts (kparams_group, as the
// assembly's accumulate launches), each adding to Out.
//
// Memory: the scaled points and prepared operands of xa and xb (ctx->dxs, dxps, dgA, dgB:
// (nse (de + 4 ceil(de / 4) + 1)) doubles per point) and S na min(nv, 64) doubles of partials
// (ctx->dkmm, only when S > 1, and S <= 64 falls to 1 as na grows) -- linear in na + nb; nothing
// on this path is sized by na nb.
//
// kmatmul_kernel evaluates K(x, x) in full; kmatmul_sym_kernel (below, GPR_KMM_SYM) evaluates the
// tiles on and above the diagonal and transposes each in registers for the other triangle.
#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "gram_tile.hpp"
#include "kexp.hpp"
#include "kmm_vstage.hpp"

namespace {

// Two workgroups per CU (256 registers a lane), except the run-time-d tile with 64 columns of V,
// whose operand chunks and 32 accumulators do not fit them (about 200 bytes a lane of scratch):
// one workgroup.
// gB / nrmB: the operands of the summed points xb (the tile's rows); gA / nrmA: of the output
// points xa (its columns).  diag: a same-object form -- the tile with equal block indices is
// K's diagonal tile (eps per term, sigma_n^2 when kp.has_noise).  Out: this call's columns;
// slab y writes at Out + y * slab_stride; accum: the result is added to what Out holds.
template <int SC, bool MIX, bool PROD, int NVB>
__global__ __launch_bounds__(256, SC == 0 && NVB == 4 ? 1 : 2) void kmatmul_kernel(
    KParams kp, int Srt, const double* __restrict__ gB, const double* __restrict__ gA,
    const double* __restrict__ nrmB, const double* __restrict__ nrmA, int nblkB, int nblkA, int na,
    int nb, int diag, int slab_blocks, const double* __restrict__ V, size_t ldv, int nvc, int vec,
    double* __restrict__ Out, size_t ldo, size_t slab_stride, int accum) {
  extern __shared__ double dyn_lds[];
  double* Vs = dyn_lds;                    // 16 NVB columns x KMM_VS
  double* tabs = Vs + 16 * NVB * KMM_VS;   // nse exp tables
  double* tmw = tabs + 256 * kp.nse;       // PROD: the running products (16 x 256)
  const int S = SC > 0 ? SC : Srt;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wr = w & 1, wc = w >> 1;
  const int i0 = blockIdx.x * KT;
  const int jb_lo = blockIdx.y * slab_blocks;
  const int jb_hi = min(jb_lo + slab_blocks, (nb + KT - 1) / KT);
  load_part_tables(kp, tabs);
  gd4 acc[NVB][2];
#pragma unroll
  for (int vb = 0; vb < NVB; ++vb)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) acc[vb][cb] = gd4{0.0, 0.0, 0.0, 0.0};
  kv2 vr[2 * NVB];
  kmm_fetch_v<NVB>(V, ldv, nb, nvc, jb_lo * KT, vec, vr);
  kmm_stage_v<NVB>(vr, Vs);
  __syncthreads();
  for (int jb = jb_lo; jb < jb_hi; ++jb) {
    const int j0 = jb * KT;
    const bool more = jb + 1 < jb_hi;
    if (more) kmm_fetch_v<NVB>(V, ldv, nb, nvc, j0 + KT, vec, vr);  // lands under the tile
    gd4 v[2][2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) v[rb][cb] = gd4{0.0, 0.0, 0.0, 0.0};
    if (diag && j0 == i0)
      gram_tile<SC, true, MIX, PROD>(kp, S, gB, gA, nrmB, nrmA, nblkB, nblkA, j0, i0, tabs, v, tmw);
    else
      gram_tile<SC, false, MIX, PROD>(kp, S, gB, gA, nrmB, nrmA, nblkB, nblkA, j0, i0, tabs, v, tmw);
    // Out^T += V^T K: the tile's register q of block (rb, cb) is k-step q's B operand
    const double* va = Vs + (lane & 15) * KMM_VS + 32 * wr + (lane >> 4);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int vb = 0; vb < NVB; ++vb) {
          const double a = va[16 * vb * KMM_VS + 16 * rb + 4 * q];
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
            acc[vb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, v[rb][cb][q], acc[vb][cb], 0, 0, 0);
        }
    __syncthreads();  // the block's V is read
    if (more) kmm_stage_v<NVB>(vr, Vs);
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

// Out[i, c] (+)= W_0[i, c] + W_1[i, c] + ... in slab order (W_s: na x nvc, ld na)
__global__ __launch_bounds__(256) void kmm_reduce_kernel(const double* __restrict__ W, int nslab,
                                                         int na, int nvc, double* __restrict__ Out,
                                                         size_t ldo, int accum) {
  const size_t total = (size_t)na * nvc;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total;
       t += (size_t)gridDim.x * blockDim.x) {
    const size_t c = t / na, i = t - c * na;
    double s = W[t];
    for (int k = 1; k < nslab; ++k) s += W[(size_t)k * total + t];
    double* dst = Out + c * ldo + i;
    *dst = accum ? *dst + s : s;
  }
}

// one pass: columns [0, nvc <= 64) of V, the parts of g (<= KMAXP, whole terms) at part offset p0
template <int SC, int NVB>
int kmm_launch(gpr_ctx* ctx, const KmmOps& o, const KParams& g, int p0, const double* V, int ldv,
               int nvc, double* Out, int ldo, int accum) {
  const int S = o.S;
  KmmSlabPlan pl;
  GPR_TRY(kmm_slab_plan(ctx, o.na, o.nb, V, ldv, nvc, Out, ldo, accum, &pl));
  const size_t opB = (size_t)p0 * o.nbB * S * 64, opA = (size_t)p0 * o.nbA * S * 64;
  const size_t nB = (size_t)p0 * o.nbB * 16, nA = (size_t)p0 * o.nbA * 16;
  const dim3 grid((unsigned)pl.nta, (unsigned)pl.slabs);
  int rc = 0;
  kmixprod_dispatch_full(g.mix, g.prod, [&](auto mix, auto prod) {
    constexpr bool MIX = decltype(mix)::value, PROD = decltype(prod)::value;
    const size_t lds = sizeof(double) * (16 * NVB * KMM_VS + 256 * g.nse + (PROD ? 16 * 256 : 0));
    auto* kern = &kmatmul_kernel<SC, MIX, PROD, NVB>;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess) {
      rc = set_err(ctx, GPR_E_HIP, "kernel_matmul: %zu bytes of LDS refused", lds);
      return;
    }
    kern<<<grid, 256, lds, ctx->stream>>>(g, S, o.B + opB, o.A + opA, o.nrmB + nB, o.nrmA + nA,
                                          o.nbB, o.nbA, o.na, o.nb, o.same != GPR_CROSS,
                                          pl.slab_blocks, V, (size_t)ldv, nvc, pl.vec, pl.dst,
                                          pl.ldd, pl.stride, pl.accum);
  });
  GPR_TRY(rc);
  LAUNCH_CHECK(ctx);
  if (pl.slabs > 1) GPR_TRY(kmm_reduce_slabs(ctx, pl.slabs, o.na, nvc, Out, ldo, accum));
  return 0;
}

template <int SC>
int kmm_launch_nv(gpr_ctx* ctx, const KmmOps& o, const KParams& g, int p0, const double* V,
                  int ldv, int nvc, double* Out, int ldo, int accum) {
  return nvc <= 16 ? kmm_launch<SC, 1>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum)
                   : kmm_launch<SC, 4>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum);
}

// ---- the symmetric route: K(x, x) V from the tiles I <= J alone (GPR_KMM_SYM) -------------------
// A tile T (rows: block J, columns: block I) serves Out[I] += T^T V[J] as above and, transposed,
// Out[J] += T V[I].  The second product sums over the tile's columns, and both MFMA operand
// layouts carry the summed index on l >> 4, the tile's row axis: it needs T^T in the tile's own
// register layout.  Four MFMAs per 16 x 16 block against a constant give exactly that: register q
// taken as the A operand is A[m = l & 15][k = l >> 4] = T[4 q + k][m]; with B_q[k][n] =
// (n == 4 q + k) the four products sum to D[m][n] = T[n][m], and D's register layout
// (m = 4 q' + (l >> 4), n = l & 15) is the tile's.  Products by 1.0 and sums with zeros: exact.
// Block (rb, cb) of a wave's quadrant is block (cb, rb) of the transposed quadrant, so nothing
// leaves the wave (no LDS, no barrier).
//
// Work split.  A workgroup owns a band of G consecutive blocks I (kmm_sym_g: 4, 2 or 1) and one slab of the band's walk
// over J >= the band's first block.  V of the band's blocks is staged in LDS once, V[J] per step
// with the register prefetch above.  Per J it evaluates the band's tiles with I <= J (the tile
// I == J by the DIAG instance, direct product only: it is whole and symmetric in itself), each into
// the persistent Out[I] accumulators (8 registers per block of the band) and, transposed, into one
// Out[J] accumulator, which the two waves that share those rows add through LDS (wc = 0 plus
// wc = 1) and store once per J: one 64 x 16 flush per G tiles, n^2 nv / (64 G) doubles in all
// each way.  The grid is (slabs, bands of this launch); nobody waits on another workgroup.  Walks
// shorten as the band index grows: bands launch in index order, the longest first.
// Workspace (ctx->dkmm, linear in n): at most KMS_P bands per launch, each with one n x nvc
// partial of Out[J] (its slabs write disjoint rows of it) and one (64 G) x nvc partial of Out[I]
// per slab; kmm_sym_reduce_kernel adds them in band, then slab order, and the next launch's
// bands reuse the space in stream order.  No atomics: two calls agree bit for bit.
// blocks per band: the most whose accumulators the instance's registers hold without scratch,
// two workgroups per CU (256 registers a lane) as kmatmul_kernel
template <int SC, bool MIX, bool PROD>
constexpr int kmm_sym_g() { return SC == 0 ? 1 : (MIX || PROD ? 2 : 4); }
constexpr int KMS_P = 64;  // most bands of one launch

template <int SC, bool MIX, bool PROD, int G>
__global__ __launch_bounds__(256, 2) void kmatmul_sym_kernel(
    KParams kp, int Srt, const double* __restrict__ gR, const double* __restrict__ gC,
    const double* __restrict__ nrm, int nblk16, int n, int band0, int nslab,
    const double* __restrict__ V, size_t ldv, int nvc, int vec, double* __restrict__ Wt,
    double* __restrict__ Wd) {
  extern __shared__ double dyn_lds[];
  double* Vs = dyn_lds;                  // V[J]: 16 columns x KMM_VS
  double* Vb = Vs + 16 * KMM_VS;         // V of the band: G x 16 x KMM_VS
  double* red = Vb + G * 16 * KMM_VS;    // Out[J] hand-over: 2 row halves x 8 x 64
  double* tabs = red + 1024;             // nse exp tables
  double* tmw = tabs + 256 * kp.nse;     // PROD: the running products (16 x 256)
  const int S = SC > 0 ? SC : Srt;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wr = w & 1, wc = w >> 1;
  const int nblk = (n + KT - 1) / KT;
  const int ib0 = (band0 + (int)blockIdx.y) * G;  // < nblk
  const int sb = (nblk - ib0 + nslab - 1) / nslab;
  const int jb_lo = ib0 + blockIdx.x * sb;
  const int jb_hi = min(jb_lo + sb, nblk);  // (an empty slab writes zeros)
  load_part_tables(kp, tabs);
  kv2 vr[2];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    kmm_fetch_v<1>(V, ldv, n, nvc, (ib0 + g) * KT, vec, vr);
    kmm_stage_v<1>(vr, Vb + g * 16 * KMM_VS);
  }
  kmm_fetch_v<1>(V, ldv, n, nvc, jb_lo * KT, vec, vr);
  kmm_stage_v<1>(vr, Vs);
  gd4 ai[G][2];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) ai[g][cb] = gd4{0.0, 0.0, 0.0, 0.0};
  double idq[4];  // B_q[k = l >> 4][n = l & 15] = (n == 4 q + k)
#pragma unroll
  for (int q = 0; q < 4; ++q) idq[q] = (lane & 15) == 4 * q + (lane >> 4) ? 1.0 : 0.0;
  __syncthreads();
  double* Wtp = Wt + (size_t)blockIdx.y * n * nvc;
  for (int jb = jb_lo; jb < jb_hi; ++jb) {
    const int j0 = jb * KT;
    const bool more = jb + 1 < jb_hi;
    if (more) kmm_fetch_v<1>(V, ldv, n, nvc, j0 + KT, vec, vr);  // lands under the tiles
    gd4 aj[2] = {gd4{0.0, 0.0, 0.0, 0.0}, gd4{0.0, 0.0, 0.0, 0.0}};
    const double* va = Vs + (lane & 15) * KMM_VS + 32 * wr + (lane >> 4);
    auto kmm_sym_tile = [&](int g) {
      const int ib = ib0 + g;
      if (ib > jb) return;  // the band's own super-block: I <= J only (and I < nblk with it)
      gd4 v[2][2];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) v[rb][cb] = gd4{0.0, 0.0, 0.0, 0.0};
      if (ib == jb)
        gram_tile<SC, true, MIX, PROD>(kp, S, gR, gC, nrm, nrm, nblk16, nblk16, j0, ib * KT, tabs, v, tmw);
      else
        gram_tile<SC, false, MIX, PROD>(kp, S, gR, gC, nrm, nrm, nblk16, nblk16, j0, ib * KT, tabs, v, tmw);
      __builtin_amdgcn_sched_barrier(0);  // (no operand of the products is loaded above: registers)
      // Out[I]^T += V[J]^T T, as kmatmul_kernel
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double a = va[16 * rb + 4 * q];
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
            ai[0][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, v[rb][cb][q], ai[0][cb], 0, 0, 0);
        }
      if (ib == jb) return;
      __builtin_amdgcn_sched_barrier(0);
      // Out[J]^T += V[I]^T T^T: block (rb, cb) transposed is block (cb, rb) of T^T, whose rows
      // (the summed points) are I's 32 wc + 16 cb + [0, 16) and whose columns are J's
      // 32 wr + 16 rb + [0, 16)
      const double* vi = Vb + (g * 16 + (lane & 15)) * KMM_VS + 32 * wc + (lane >> 4);
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          gd4 t = gd4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int q = 0; q < 4; ++q)
            t = __builtin_amdgcn_mfma_f64_16x16x4f64(v[rb][cb][q], idq[q], t, 0, 0, 0);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            aj[rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(vi[16 * cb + 4 * q], t[q], aj[rb], 0, 0, 0);
        }
    };
    // (a loop at run time: one copy of the tile code, whose accumulator is ai[0] -- the G
    // accumulators rotate by one per step, G steps per J)
#pragma nounroll
    for (int g = 0; g < G; ++g) {
      kmm_sym_tile(g);
      const gd4 r0 = ai[0][0], r1 = ai[0][1];
#pragma unroll
      for (int h = 0; h + 1 < G; ++h) {
        ai[h][0] = ai[h + 1][0];
        ai[h][1] = ai[h + 1][1];
      }
      ai[G - 1][0] = r0;
      ai[G - 1][1] = r1;
    }
    // the two column halves' sums of a row half: wave (wr, 1) hands Out[J] to (wr, 0)
    double* rj = red + wr * 512 + lane;
    if (wc == 1) {
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int q = 0; q < 4; ++q) rj[(rb * 4 + q) * 64] = aj[rb][q];
    }
    __syncthreads();  // the block's V is read, the hand-over written
    if (more) kmm_stage_v<1>(vr, Vs);
    if (wc == 0) {
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = j0 + 32 * wr + 16 * rb + (lane & 15);
          const int c = (lane >> 4) + 4 * q;
          if (i < n && c < nvc) Wtp[(size_t)c * n + i] = aj[rb][q] + rj[(rb * 4 + q) * 64];
        }
    }
    __syncthreads();
  }
  // Out[I]: the two row halves' sums of a column half, as kmatmul_kernel, over the band's V
  double* rd = Vb + wc * (G * 512) + lane;  // 1024 G doubles of the 1056 G
  if (wr == 1) {
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) rd[((g * 2 + cb) * 4 + q) * 64] = ai[g][cb][q];
  }
  __syncthreads();
  if (wr == 0) {
    double* Wdp = Wd + ((size_t)blockIdx.y * nslab + blockIdx.x) * ((size_t)G * KT * nvc);
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int il = g * KT + 32 * wc + 16 * cb + (lane & 15);
          const int c = (lane >> 4) + 4 * q;
          if (c < nvc) Wdp[(size_t)c * (G * KT) + il] = ai[g][cb][q] + rd[((g * 2 + cb) * 4 + q) * 64];
        }
  }
}

// Out[i, c] (+)= the Out[J] partials of this launch's bands that reach row i (band order), then
// the Out[I] partials of i's own band (slab order) where that band is in this launch
__global__ __launch_bounds__(256) void kmm_sym_reduce_kernel(
    const double* __restrict__ Wt, const double* __restrict__ Wd, int band0, int nbands, int nslab,
    int G, int n, int nvc, double* __restrict__ Out, size_t ldo, int accum) {
  const size_t total = (size_t)n * nvc, wd = (size_t)G * KT * nvc;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total;
       t += (size_t)gridDim.x * blockDim.x) {
    const size_t c = t / n, i = t - c * n;
    const int band = (int)(i / KT) / G;
    if (band < band0) continue;  // every band of this launch starts below row i
    const int np = min(nbands, band - band0 + 1);
    double s = Wt[t];
    for (int k = 1; k < np; ++k) s += Wt[(size_t)k * total + t];
    if (band < band0 + nbands) {
      const double* wp = Wd + (size_t)(band - band0) * nslab * wd + c * ((size_t)G * KT) +
                         (i - (size_t)band * G * KT);
      for (int k = 0; k < nslab; ++k) s += wp[(size_t)k * wd];
    }
    double* dst = Out + c * ldo + i;
    *dst = accum ? *dst + s : s;
  }
}

// one symmetric pass: columns [0, nvc <= 16) of V, a same-points form (o.na == o.nb, one set of
// norms), the parts of g at part offset p0
template <int SC, bool MIX, bool PROD>
int kmm_sym_launch_g(gpr_ctx* ctx, const KmmOps& o, const KParams& g, int p0, const double* V,
                     int ldv, int nvc, double* Out, int ldo, int accum) {
  constexpr int G = kmm_sym_g<SC, MIX, PROD>();
  const int S = o.S, n = o.na;
  const int nblk = (n + KT - 1) / KT, nband = (nblk + G - 1) / G;
  const int ncu = ctx->ncu > 0 ? ctx->ncu : 256;
  // slabs of a launch's walks: GPR_KMM_SLABS, else two workgroups per CU, never more than the
  // launch's longest walk has blocks
  auto slabs_of = [&](int band0, int nb) {
    const int want = ctx->kmm_slabs > 0 ? ctx->kmm_slabs : (2 * ncu + nb - 1) / nb;
    return std::max(1, std::min(want, std::min(nblk - band0 * G, KMM_MAXS)));
  };
  const size_t wt = (size_t)std::min(nband, KMS_P) * n * nvc, wd1 = (size_t)G * KT * nvc;
  size_t wd = 0;
  for (int b0 = 0; b0 < nband; b0 += KMS_P) {
    const int nb = std::min(KMS_P, nband - b0);
    wd = std::max(wd, (size_t)nb * slabs_of(b0, nb) * wd1);
  }
  GPR_TRY(ensure_buf(ctx, ctx->dkmm, wt + wd));
  double* Wt = ctx->dkmm;
  double* Wd = Wt + wt;
  const int vec = ((uintptr_t)V & 15) == 0 && (ldv & 1) == 0;
  const double* gR = o.B + (size_t)p0 * o.nbB * S * 64;
  const double* gC = o.A + (size_t)p0 * o.nbA * S * 64;
  const double* nrm = o.nrmA + (size_t)p0 * o.nbA * 16;
  const size_t lds =
      sizeof(double) * ((G + 1) * 16 * KMM_VS + 1024 + 256 * g.nse + (PROD ? 16 * 256 : 0));
  auto* kern = &kmatmul_sym_kernel<SC, MIX, PROD, G>;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return set_err(ctx, GPR_E_HIP, "kernel_matmul: %zu bytes of LDS refused", lds);
  for (int b0 = 0; b0 < nband; b0 += KMS_P) {
    const int nb = std::min(KMS_P, nband - b0), slabs = slabs_of(b0, nb);
    kern<<<dim3((unsigned)slabs, (unsigned)nb), 256, lds, ctx->stream>>>(
        g, S, gR, gC, nrm, o.nbA, n, b0, slabs, V, (size_t)ldv, nvc, vec, Wt, Wd);
    LAUNCH_CHECK(ctx);
    const int blocks = (int)std::min<size_t>(((size_t)n * nvc + 255) / 256, 4096);
    kmm_sym_reduce_kernel<<<blocks, 256, 0, ctx->stream>>>(Wt, Wd, b0, nb, slabs, G, n, nvc, Out,
                                                           (size_t)ldo, accum || b0 > 0);
    LAUNCH_CHECK(ctx);
  }
  return 0;
}

// one symmetric pass: columns [0, nvc <= 16) of V, a same-points form (o.na == o.nb, one set of
// norms), the parts of g at part offset p0
template <int SC>
int kmm_sym_launch(gpr_ctx* ctx, const KmmOps& o, const KParams& g, int p0, const double* V,
                   int ldv, int nvc, double* Out, int ldo, int accum) {
  return kmixprod_dispatch_full(g.mix, g.prod, [&](auto mix, auto prod) {
    return kmm_sym_launch_g<SC, decltype(mix)::value, decltype(prod)::value>(ctx, o, g, p0, V, ldv,
                                                                             nvc, Out, ldo, accum);
  });
}

}  // namespace

int kmm_slab_plan(gpr_ctx* ctx, int na, int nb, const double* V, int ldv, int nvc, double* Out,
                  int ldo, int accum, KmmSlabPlan* pl) {
  const int nta = (na + KT - 1) / KT, nbb = (nb + KT - 1) / KT;
  const int ncu = ctx->ncu > 0 ? ctx->ncu : 256;
  int slabs = ctx->kmm_slabs > 0 ? ctx->kmm_slabs : (2 * ncu + nta - 1) / nta;
  slabs = std::max(1, std::min(slabs, std::min(nbb, KMM_MAXS)));
  const int slab_blocks = (nbb + slabs - 1) / slabs;
  slabs = (nbb + slab_blocks - 1) / slab_blocks;  // (no empty slab)
  *pl = KmmSlabPlan{nta, slabs, slab_blocks, ((uintptr_t)V & 15) == 0 && (ldv & 1) == 0,
                    slabs > 1 ? 0 : accum, Out, (size_t)ldo, 0};
  if (slabs > 1) {
    GPR_TRY(ensure_buf(ctx, ctx->dkmm, (size_t)slabs * na * nvc));
    pl->dst = ctx->dkmm;
    pl->ldd = (size_t)na;
    pl->stride = (size_t)na * nvc;
  }
  return 0;
}

int kmm_reduce_slabs(gpr_ctx* ctx, int slabs, int na, int nvc, double* Out, int ldo, int accum) {
  const int blocks = (int)std::min<size_t>(((size_t)na * nvc + 255) / 256, 4096);
  kmm_reduce_kernel<<<blocks, 256, 0, ctx->stream>>>(ctx->dkmm, slabs, na, nvc, Out, (size_t)ldo,
                                                     accum);
  LAUNCH_CHECK(ctx);
  return 0;
}

int kmm_prepare(gpr_ctx* ctx, const KParams& kpx, const double* dXa, int na, const double* dXb,
                int nb, int same, KmmOps* o, bool f32) {
  KParams kp = kparams_features(kpx);
  if (same == GPR_SAME_OBJECT) kp.has_noise = 0;  // eps per term, no noise (gpr_kernel's rule)
  GPR_TRY(launch_scaled_points(ctx, kpx, dXa, na, ctx->dxs));
  if (!same) GPR_TRY(launch_scaled_points(ctx, kpx, dXb, nb, ctx->dxps));
  const int S = (kp.d + 3) / 4;
  GramOps g;
  GPR_TRY(gram_prepare(ctx, kp, S, ctx->dxs, na, same ? nullptr : ctx->dxps.p, nb, same != 0, &g));
  *o = KmmOps{kp, na, nb, same, S, ctx->dxs, same ? ctx->dxs.p : ctx->dxps.p,
              g.A, g.nrmA, g.B, g.nrmB, g.nbA, g.nbB};
  // GPR_KMM_PREC: the FP32 points beside them, where the description is inside that route's envelope
  if (f32 && ctx->kmm_prec && kmm_f32_takes(kp)) GPR_TRY(kmm_f32_prepare(ctx, o));  // (after gram_prepare: its centres)
  return 0;
}

int kmm_apply(gpr_ctx* ctx, const KmmOps& o, const double* dV, int nv, int ldv, double* dOut,
              int ldo, int prec) {
  if (prec != 0 && o.fa) return kmm_f32_apply(ctx, o, dV, nv, ldv, dOut, ldo);
  const KParams& kp = o.kp;
  for (int c0 = 0; c0 < nv; c0 += 64) {
    const int nvc = std::min(64, nv - c0);
    const double* V = dV + (size_t)c0 * ldv;
    double* Out = dOut + (size_t)c0 * ldo;
    for (int p0 = 0, cnt = 0; p0 < kp.nse; p0 += cnt) {
      KParams g = kp;
      cnt = kp.nse;
      if (kp.nse > KMAXP) {  // groups of whole terms; the last one carries the noise
        cnt = kparams_group_count(kp, p0);
        g = kparams_group(kp, p0, cnt, p0 + cnt >= kp.nse ? kp.has_noise : 0);
      }
      // k-steps compiled in for d <= 8, walked at run time above (zero steps change no bit)
      const int accum = p0 > 0;
      if (ctx->kmm_sym && o.same != GPR_CROSS && nvc <= 16) {  // (wider passes: MFMA-bound)
        if (o.S == 1) GPR_TRY((kmm_sym_launch<1>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum)));
        else if (o.S == 2) GPR_TRY((kmm_sym_launch<2>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum)));
        else GPR_TRY((kmm_sym_launch<0>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum)));
        continue;
      }
      if (o.S == 1) GPR_TRY((kmm_launch_nv<1>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum)));
      else if (o.S == 2) GPR_TRY((kmm_launch_nv<2>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum)));
      else GPR_TRY((kmm_launch_nv<0>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum)));
    }
  }
  return 0;
}

extern "C" {

int gpr_kernel_matmul(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                      const double* dXa, int na, const double* dXb, int nb, int same, double eps,
                      const double* dV, int nv, int ldv, double* dOut, int ldo) {
  KParams kp;
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, eps, &kp, nullptr));
  if (same != GPR_CROSS && same != GPR_SELF && same != GPR_SAME_OBJECT)
    return set_err(ctx, GPR_E_ARG, "same=%d is not GPR_CROSS, GPR_SELF or GPR_SAME_OBJECT", same);
  if (!dXa) return set_err(ctx, GPR_E_ARG, "dXa is NULL");
  if (same == GPR_CROSS && !dXb) return set_err(ctx, GPR_E_ARG, "dXb is NULL for a cross kernel");
  if (!dV) return set_err(ctx, GPR_E_ARG, "dV is NULL");
  if (!dOut) return set_err(ctx, GPR_E_ARG, "dOut is NULL");
  if (na < 1) return set_err(ctx, GPR_E_ARG, "na=%d < 1", na);
  if (nb < 1) return set_err(ctx, GPR_E_ARG, "nb=%d < 1", nb);
  if (nv < 1) return set_err(ctx, GPR_E_ARG, "nv=%d < 1", nv);
  if (same != GPR_CROSS && na != nb)
    return set_err(ctx, GPR_E_ARG, "na=%d != nb=%d for a same-object form", na, nb);
  if (ldv < nb) return set_err(ctx, GPR_E_ARG, "ldv=%d < nb=%d", ldv, nb);
  if (ldo < na) return set_err(ctx, GPR_E_ARG, "ldo=%d < na=%d", ldo, na);
  KmmOps o;
  GPR_TRY(kmm_prepare(ctx, kp, dXa, na, dXb, nb, same, &o, true));
  return kmm_apply(ctx, o, dV, nv, ldv, dOut, ldo);
}

}  // extern "C"
