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
// Not done here: K(x, x) is evaluated in full (one tile serving both triangles needs the tile in
// the transposed layout as well).
#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "gram_tile.hpp"
#include "kexp.hpp"

namespace {

constexpr int KMM_VS = KT + 2;   // LDS stride (doubles) between the staged V block's columns
constexpr int KMM_MAXS = 64;     // most slabs of one launch
typedef double kv2 __attribute__((ext_vector_type(2)));

// this thread's share of rows [j0, j0 + 64) x columns [0, 16 NVB) of V: row pair 2 (t & 31) of
// columns (t >> 5) + 8 k.  Zero past nb or nvc, and nothing past them is read.
template <int NVB>
__device__ __forceinline__ void kmm_fetch_v(const double* __restrict__ V, size_t ldv, int nb,
                                            int nvc, int j0, bool vec, kv2 (&r)[2 * NVB]) {
  const int j = j0 + 2 * (int)(threadIdx.x & 31), cg = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 2 * NVB; ++k) {
    const int c = cg + 8 * k;
    kv2 e = {0.0, 0.0};
    if (c < nvc && j < nb) {
      const double* src = V + (size_t)c * ldv + j;
      if (j + 1 < nb) {
        if (vec) {
          e = *reinterpret_cast<const kv2*>(src);
        } else {
          e[0] = src[0];
          e[1] = src[1];
        }
      } else {
        e[0] = src[0];
      }
    }
    r[k] = e;
  }
}

template <int NVB>
__device__ __forceinline__ void kmm_stage_v(const kv2 (&r)[2 * NVB], double* Vs) {
  const int pr = threadIdx.x & 31, cg = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 2 * NVB; ++k)
    *reinterpret_cast<kv2*>(Vs + (cg + 8 * k) * KMM_VS + 2 * pr) = r[k];
}

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
  const int nta = (o.na + KT - 1) / KT, nbb = (o.nb + KT - 1) / KT;
  const int ncu = ctx->ncu > 0 ? ctx->ncu : 256;
  int slabs = ctx->kmm_slabs > 0 ? ctx->kmm_slabs : (2 * ncu + nta - 1) / nta;
  slabs = std::max(1, std::min(slabs, std::min(nbb, KMM_MAXS)));
  const int slab_blocks = (nbb + slabs - 1) / slabs;
  slabs = (nbb + slab_blocks - 1) / slab_blocks;  // (no empty slab)
  double* dst = Out;
  size_t ldd = (size_t)ldo, stride = 0;
  if (slabs > 1) {
    GPR_TRY(ensure_buf(ctx, ctx->dkmm, (size_t)slabs * o.na * nvc));
    dst = ctx->dkmm;
    ldd = (size_t)o.na;
    stride = (size_t)o.na * nvc;
  }
  const int vec = ((uintptr_t)V & 15) == 0 && (ldv & 1) == 0;
  const size_t opB = (size_t)p0 * o.nbB * S * 64, opA = (size_t)p0 * o.nbA * S * 64;
  const size_t nB = (size_t)p0 * o.nbB * 16, nA = (size_t)p0 * o.nbA * 16;
  const dim3 grid((unsigned)nta, (unsigned)slabs);
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
                                          slab_blocks, V, (size_t)ldv, nvc, vec, dst, ldd, stride,
                                          slabs > 1 ? 0 : accum);
  });
  GPR_TRY(rc);
  LAUNCH_CHECK(ctx);
  if (slabs > 1) {
    const int blocks = (int)std::min<size_t>(((size_t)o.na * nvc + 255) / 256, 4096);
    kmm_reduce_kernel<<<blocks, 256, 0, ctx->stream>>>(ctx->dkmm, slabs, o.na, nvc, Out,
                                                       (size_t)ldo, accum);
    LAUNCH_CHECK(ctx);
  }
  return 0;
}

template <int SC>
int kmm_launch_nv(gpr_ctx* ctx, const KmmOps& o, const KParams& g, int p0, const double* V,
                  int ldv, int nvc, double* Out, int ldo, int accum) {
  return nvc <= 16 ? kmm_launch<SC, 1>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum)
                   : kmm_launch<SC, 4>(ctx, o, g, p0, V, ldv, nvc, Out, ldo, accum);
}

}  // namespace

int kmm_prepare(gpr_ctx* ctx, const KParams& kpx, const double* dXa, int na, const double* dXb,
                int nb, int same, KmmOps* o) {
  KParams kp = kparams_features(kpx);
  if (same == GPR_SAME_OBJECT) kp.has_noise = 0;  // eps per term, no noise (gpr_kernel's rule)
  GPR_TRY(launch_scaled_points(ctx, kpx, dXa, na, ctx->dxs));
  if (!same) GPR_TRY(launch_scaled_points(ctx, kpx, dXb, nb, ctx->dxps));
  const int S = (kp.d + 3) / 4;
  GramOps g;
  GPR_TRY(gram_prepare(ctx, kp, S, ctx->dxs, na, same ? nullptr : ctx->dxps.p, nb, same != 0, &g));
  *o = KmmOps{kp, na, nb, same, S, ctx->dxs, same ? ctx->dxs.p : ctx->dxps.p,
              g.A, g.nrmA, g.B, g.nrmB, g.nbA, g.nbB};
  return 0;
}

int kmm_apply(gpr_ctx* ctx, const KmmOps& o, const double* dV, int nv, int ldv, double* dOut,
              int ldo) {
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
  GPR_TRY(kmm_prepare(ctx, kp, dXa, na, dXb, nb, same, &o));
  return kmm_apply(ctx, o, dV, nv, ldv, dOut, ldo);
}

}  // extern "C"
