// K-assembly above d = 20 through the C ABI, timed with device events: the Gram form on MFMA
// with a run-time number of k-steps (GPR_KBUILD_GRAM_MAXD unlimited) against the difference-form
// kernels every d > 20 took before (GPR_KBUILD_GRAM_MAXD = 20), alternated in one process.
// Symmetric N x N (SE and SE+SE+WN) and cross N x N/2 (SE+SE+WN); then the fused MLL gradient
// pass at d = 32 (register variant) and d = 64 (two-phase wide variant).
// Build: make -C gaussianprocessregression.jl_amd/csrc hdbench
// Run:   tools/highd_kbuild_bench [N = 16384] [reps = 7] [Ngrad = 8192]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../include/gpr_hip.h"

#define CK(x)                                                          \
  do {                                                                 \
    if ((x) != 0) {                                                    \
      fprintf(stderr, "%s failed (line %d): %s\n", #x, __LINE__, ctx ? gpr_last_error(ctx) : ""); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static gpr_ctx_t ctx = nullptr;

struct Stat {
  double mn, med, mx;
};
static Stat stat(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return {v.front(), v[v.size() / 2], v.back()};
}

int main(int argc, char** argv) {
  const int N = argc > 1 ? atoi(argv[1]) : 16384;
  const int reps = argc > 2 ? atoi(argv[2]) : 7;
  const int Ng = argc > 3 ? atoi(argv[3]) : 8192;
  const int M = N / 2, DMAX = 256;
  // the gradient pass reads the N x N buffer as its Ngrad x Ngrad K^{-1} and the first Ngrad
  // points: both must fit
  if (N < 64 || (N & 1) || reps < 1 || Ng < 1 || Ng > N) {
    fprintf(stderr, "usage: highd_kbuild_bench [N even >= 64] [reps >= 1] [Ngrad in 1..N]\n");
    return 2;
  }
  CK(gpr_ctx_create(0, nullptr, &ctx));
  hipStream_t st = (hipStream_t)gpr_ctx_stream(ctx);
  std::mt19937_64 rng(1);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::vector<double> hx((size_t)DMAX * N);
  for (auto& v : hx) v = U(rng);
  double *dX, *dXp, *dK;
  CK(gpr_malloc(ctx, hx.size() * 8, (void**)&dX));
  CK(gpr_malloc(ctx, hx.size() * 8, (void**)&dXp));
  CK(gpr_malloc(ctx, (size_t)N * N * 8, (void**)&dK));
  CK(gpr_upload(ctx, dX, hx.data(), hx.size() * 8));
  for (auto& v : hx) v = U(rng);
  CK(gpr_upload(ctx, dXp, hx.data(), hx.size() * 8));
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);

  struct Cfg {
    const char* name;
    int kinds[3];
    int nk;
    int cross;
  };
  const Cfg cfgs[] = {{"sym SE", {GPR_SE}, 1, 0},
                      {"sym SE+SE+WN", {GPR_SE, GPR_SE, GPR_WN}, 3, 0},
                      {"cross SE+SE+WN", {GPR_SE, GPR_SE, GPR_WN}, 3, 1}};
  const int ds[] = {24, 32, 48, 64, 100, 256};
  const double maxd[2] = {20.0, 1073741824.0};
  printf("# N = %d (cross %d x %d), %d alternated repetitions per setting after 2 warm-ups each\n", N,
         N, M, reps);
  printf("# ms: min / median / max; diff = GPR_KBUILD_GRAM_MAXD=20 (difference form), gram = "
         "unlimited; store = bytes written / 8 TB/s over the gram median\n");
  printf("%-16s %4s  %-26s  %-26s  %7s  %6s\n", "build", "d", "diff ms", "gram ms", "speedup", "store");
  for (int d : ds) {
    for (const Cfg& c : cfgs) {
      std::vector<double> hp;
      for (int k = 0; k < c.nk; ++k) {
        hp.push_back(0.3 + 1.7 * U(rng));
        if (c.kinds[k] == GPR_SE)
          for (int i = 0; i < d; ++i) hp.push_back((0.3 + 1.7 * U(rng)) * std::sqrt(8.0 / d));
      }
      std::vector<double> t[2];
      for (int r = -2; r < reps; ++r)
        for (int s = 0; s < 2; ++s) {
          CK(gpr_set_knob(ctx, "GPR_KBUILD_GRAM_MAXD", maxd[s]));
          hipEventRecord(e0, st);
          CK(gpr_kernel(ctx, c.kinds, c.nk, hp.data(), d, dX, N, c.cross ? dXp : nullptr,
                        c.cross ? M : N, c.cross ? GPR_CROSS : GPR_SELF, 1e-8, dK, N));
          hipEventRecord(e1, st);
          hipEventSynchronize(e1);
          float ms = 0;
          hipEventElapsedTime(&ms, e0, e1);
          if (r >= 0) t[s].push_back(ms);
        }
      const Stat a = stat(t[0]), b = stat(t[1]);
      const double bytes = 8.0 * N * (c.cross ? M : N);
      char sa[64], sb[64];
      snprintf(sa, sizeof sa, "%.3f / %.3f / %.3f", a.mn, a.med, a.mx);
      snprintf(sb, sizeof sb, "%.3f / %.3f / %.3f", b.mn, b.med, b.mx);
      printf("%-16s %4d  %-26s  %-26s  %6.2fx  %6.2f\n", c.name, d, sa, sb, a.med / b.med,
             bytes / 8e12 / (b.med * 1e-3));
      fflush(stdout);
    }
  }

  // the fused MLL gradient pass: any matrix serves as K^{-1} for timing
  {
    const int kinds[2] = {GPR_SE, GPR_WN};
    double* dal;
    CK(gpr_malloc(ctx, (size_t)Ng * 8, (void**)&dal));
    CK(gpr_upload(ctx, dal, hx.data(), (size_t)Ng * 8));
    printf("# gpr_mll_grad, SE+WN, N = %d (events around the call: pass + reduction + read-back)\n", Ng);
    for (int d : {32, 64}) {
      std::vector<double> hp(d + 2, 0.5), g(d + 2);
      std::vector<double> t;
      for (int r = -2; r < reps; ++r) {
        hipEventRecord(e0, st);
        CK(gpr_mll_grad(ctx, kinds, 2, hp.data(), d, dX, Ng, dK, Ng, dal, 1e-8, 0, g.data()));
        hipEventRecord(e1, st);
        hipEventSynchronize(e1);
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        if (r >= 0) t.push_back(ms);
      }
      const Stat a = stat(t);
      printf("mll_grad d = %2d: %.3f / %.3f / %.3f ms\n", d, a.mn, a.med, a.mx);
    }
    gpr_free(ctx, dal);
  }
  gpr_free(ctx, dX);
  gpr_free(ctx, dXp);
  gpr_free(ctx, dK);
  gpr_ctx_destroy(ctx);
  return 0;
}
