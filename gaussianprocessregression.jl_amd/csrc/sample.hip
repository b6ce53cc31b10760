// GP sampling (src/distributions.jl): standard normals on the device, the reference's
// all-elements shift of NormalDistribution(mu, Sigma) = cholesky(Sigma .+ 1e-7) (:20-23), and
// the triangular product s = L z + mu of sample(N) (:25-30) taken straight from a factor
// buffer: S = mu 1^T + U^T Z on the FP64 MFMA GEMM (gemm.hip, tri_p).
#include "common.hpp"
#include "randn.hpp"

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));

// Z[i] = element (offset + i) of the stream of `seed`, i < count.  One work-item per pair of
// the stream: a 16-B store where both members are wanted and the address allows, else the one
// or two 8-B stores (an odd offset or count takes the single member it needs at the ends).
__global__ __launch_bounds__(256) void randn_kernel(uint64_t seed, uint64_t offset,
                                                    double* __restrict__ Z, uint64_t count,
                                                    uint64_t npairs) {
  const uint64_t p0 = offset >> 1;
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < npairs;
       t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t p = p0 + t;
    double e, o;
    randn_pair(seed, p, e, o);
    const uint64_t g0 = 2 * p;              // (offset + count does not wrap: checked on the host)
    const bool in0 = g0 >= offset;          // false only for the first pair of an odd offset
    const uint64_t i1 = g0 + 1 - offset;    // index of the odd member (g0 + 1 >= offset always)
    const bool in1 = i1 < count;
    if (in0 && in1 && ((uintptr_t)(Z + (i1 - 1)) & 15) == 0) {
      *reinterpret_cast<d2*>(Z + (i1 - 1)) = d2{e, o};
    } else {
      if (in0) Z[i1 - 1] = e;
      if (in1) Z[i1] = o;
    }
  }
}

// A[i, j] += s over mode 0: the upper triangle with its diagonal (what dpotrf 'U' reads);
// 1: that and the whole 128 x 128 diagonal blocks (what the upper-only K assembly wrote: the
// tile-DAG mirrors the rest from it); 2: every element
__global__ __launch_bounds__(256) void add_scalar_kernel(double* __restrict__ A, size_t lda, int n,
                                                         double s, int mode) {
  for (int j = blockIdx.y; j < n; j += gridDim.y) {
    const int rows = mode == 0 ? j + 1 : mode == 1 ? min(n, (j / 128 + 1) * 128) : n;
    double* col = A + (size_t)j * lda;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += gridDim.x * blockDim.x)
      col[i] += s;
  }
}

int launch_add_scalar(gpr_ctx* ctx, double* A, int n, int lda, double s, int mode) {
  if (n <= 0 || s == 0.0) return 0;
  const int gx = std::max(1, std::min(16, (n + 255) / 256));
  TimerScope ts(ctx, TC_OTHER, 0.0);
  add_scalar_kernel<<<dim3(gx, std::min(n, 65535)), 256, 0, ctx->stream>>>(A, (size_t)lda, n, s, mode);
  LAUNCH_CHECK(ctx);
  return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// S = mu 1^T + U^T Z from the factor buffer dU (arguments checked by the callers)
int mvn_sample_core(gpr_ctx* ctx, const double* dU, int n, int ldu, const double* dmu,
                    const double* dZ, int ns, int ldz, double* dS, int lds) {
  GemmArgs g{};
  g.P = dU; g.ldp = ldu;
  g.Q = dZ; g.ldq = ldz;
  g.C = dS; g.ldc = lds;
  g.M = n; g.N = ns; g.K = n;
  g.alpha = 1.0; g.beta = 0.0;
  g.kend_from_m = 1;
  TimerScope ts(ctx, TC_OTHER, (double)n * n * ns);
  // Where the LDS-DMA pipelined kernel takes the operands, the rows above each diagonal tile
  // (k < m0: nothing to mask) go through it, and only the diagonal tiles' own 128 k-values
  // through the masked register-staged kernel, accumulating onto the first launch's result.
  const bool split = n > 256 && (n & 15) == 0 && aligned16(dU) && aligned16(dZ) &&
                     (ldu & 1) == 0 && (ldz & 1) == 0;
  if (split) {
    GemmArgs a = g;
    a.kend_from_m = 2;
    GPR_TRY(launch_gemm_tn(ctx, a, TC_OTHER));
    g.beta = 1.0;
    g.kfrom_m = 1;
  }
  g.tri_p = 1;
  g.mu = dmu;
  return launch_gemm_tn(ctx, g, TC_OTHER);
}

// [p, p + rows + (cols - 1) ld) of two column-major buffers intersect
bool overlap(const double* a, int rows_a, int cols_a, int lda, const double* b, int rows_b,
             int cols_b, int ldb) {
  const uintptr_t a0 = (uintptr_t)a, a1 = (uintptr_t)(a + ((size_t)(cols_a - 1) * lda + rows_a));
  const uintptr_t b0 = (uintptr_t)b, b1 = (uintptr_t)(b + ((size_t)(cols_b - 1) * ldb + rows_b));
  return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" {

int gpr_randn(gpr_ctx_t ctx, uint64_t seed, uint64_t offset, double* dZ, size_t count) {
  if (!ctx) return GPR_E_ARG;
  if (count == 0) return 0;
  if (!dZ) return set_err(ctx, GPR_E_ARG, "gpr_randn: dZ is NULL");
  if (offset + (uint64_t)count < offset)
    return set_err(ctx, GPR_E_ARG, "gpr_randn: offset + count exceeds 2^64");
  if (((uintptr_t)dZ & 7) != 0) return set_err(ctx, GPR_E_ARG, "gpr_randn: dZ is not 8-B aligned");
  const uint64_t npairs = ((offset + count - 1) >> 1) - (offset >> 1) + 1;
  const uint64_t want = (npairs + 255) / 256;
  const unsigned blocks = (unsigned)std::min<uint64_t>(want, 16384);  // grid-stride beyond that
  TimerScope ts(ctx, TC_OTHER, 0.0);
  randn_kernel<<<blocks, 256, 0, ctx->stream>>>(seed, offset, dZ, (uint64_t)count, npairs);
  LAUNCH_CHECK(ctx);
  return 0;
}

int gpr_mvn_sample(gpr_ctx_t ctx, const double* dU, int n, int ldu, const double* dmu,
                   const double* dZ, int ns, int ldz, double* dS, int lds) {
  if (!ctx) return GPR_E_ARG;
  if (n < 1 || ns < 1 || ldu < n || ldz < n || lds < n)
    return set_err(ctx, GPR_E_ARG, "gpr_mvn_sample: bad sizes (n=%d ns=%d ldu=%d ldz=%d lds=%d)", n,
                   ns, ldu, ldz, lds);
  if (!dU || !dZ || !dS) return set_err(ctx, GPR_E_ARG, "gpr_mvn_sample: NULL device pointer");
  if (overlap(dS, n, ns, lds, dZ, n, ns, ldz))
    return set_err(ctx, GPR_E_ARG, "gpr_mvn_sample: dS overlaps dZ");
  if (overlap(dS, n, ns, lds, dU, n, n, ldu) || (dmu && overlap(dS, n, ns, lds, dmu, n, 1, n)))
    return set_err(ctx, GPR_E_ARG, "gpr_mvn_sample: dS overlaps an input");
  return mvn_sample_core(ctx, dU, n, ldu, dmu, dZ, ns, ldz, dS, lds);
}

int gpr_mvn_factor(gpr_ctx_t ctx, double* dA, int n, int lda, double shift, int* info) {
  if (!ctx) return GPR_E_ARG;
  if (n < 1 || lda < n || !dA) return set_err(ctx, GPR_E_ARG, "gpr_mvn_factor: bad n/lda/dA");
  GPR_TRY(launch_add_scalar(ctx, dA, n, lda, shift, 0));
  int hinfo = 0;
  GPR_TRY(potrf_core(ctx, dA, n, lda, &hinfo));
  if (info) *info = hinfo;
  return hinfo;
}

int gpr_sample_prior(gpr_ctx_t ctx, const int* kinds, int nk, const double* hp, int d,
                     const double* dX, int n, const double* dmu, double shift, double eps,
                     const double* dZ, int ns, int ldz, double* dK, int ldk, double* dS, int lds,
                     int* info) {
  if (!ctx) return GPR_E_ARG;
  KParams kp;
  GPR_TRY(make_kparams(ctx, kinds, nk, hp, d, eps, &kp, nullptr));
  if (n < 1 || ns < 1 || ldk < n || ldz < n || lds < n || !dX || !dZ || !dK || !dS)
    return set_err(ctx, GPR_E_ARG, "gpr_sample_prior: bad args");
  if (overlap(dS, n, ns, lds, dZ, n, ns, ldz) || overlap(dS, n, ns, lds, dK, n, n, ldk) ||
      overlap(dK, n, n, ldk, dZ, n, ns, ldz))
    return set_err(ctx, GPR_E_ARG, "gpr_sample_prior: dS, dZ and dK overlap");
  GPR_TRY(launch_kernel_matrix_for_factor(ctx, kp, dX, n, dK, ldk));
  // Sigma .+ shift on every element (src/distributions.jl:21).  After an upper-only assembly
  // the tile-DAG mirrors the shifted tiles; after a full one every element is shifted here:
  // either way the strict lower triangle ends as that of the matrix that was factored.
  GPR_TRY(launch_add_scalar(ctx, dK, n, ldk, shift, ctx->fc.kup_pending(dK) ? 1 : 2));
  int hinfo = 0;
  GPR_TRY(potrf_core(ctx, dK, n, ldk, &hinfo));
  if (info) *info = hinfo;
  if (hinfo != 0) return hinfo;
  return mvn_sample_core(ctx, dK, n, ldk, dmu, dZ, ns, ldz, dS, lds);
}

// bench_sample.py's comparator (not part of the ABI): the same product by the UNMASKED
// kend_from_m GEMM, which assumes dP is zero below its diagonal
int gpr_debug_gemm_upper_p(gpr_ctx_t ctx, const double* dP, int n, int ldp, const double* dZ, int ns,
                           int ldz, double* dS, int lds) {
  if (!ctx || n < 1 || ns < 1 || ldp < n || ldz < n || lds < n || !dP || !dZ || !dS)
    return GPR_E_ARG;
  GemmArgs g{};
  g.P = dP; g.ldp = ldp;
  g.Q = dZ; g.ldq = ldz;
  g.C = dS; g.ldc = lds;
  g.M = n; g.N = ns; g.K = n;
  g.alpha = 1.0;
  g.kend_from_m = 1;
  return launch_gemm_tn(ctx, g, TC_OTHER);
}

}  // extern "C"
