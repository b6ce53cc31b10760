// Watchdog harness for the tile-DAG factorisation (dag.hip built with -DDAG_TRACE): runs
// gpr_potrf_upper on a diagonally dominant SPD matrix in a thread and prints the
// per-workgroup progress words while it runs; exits (code 3) if it has not finished in 10 s.
// usage: dag_probe N [np [rgroup [rskew [rgroup_min]]]]   (np > 0: the C3-style job; np < 0: the
// C4-style gpr_fit_kinv, SE+WN, d = 16 -- factorisation, Z = U^-T and K^-1 = Z^T Z in the one
// launch; np = 0: the factorisation alone)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../../include/gpr_hip.h"
extern "C" void gpr_debug_dag_trace(int* out, void* stream);
extern "C" void gpr_debug_diag_phases(unsigned long long* out, int reset);

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 256;
  setenv("GPR_DAG", "1", 1);
  gpr_ctx_t ctx;
  if (gpr_ctx_create(0, nullptr, &ctx)) return 1;
  // the ticket order's knobs: from the environment like every knob, or argv[3..5] = row group,
  // skew, first grouped row (the phase profile per setting in one script)
  const char* order_knobs[3] = {"GPR_DAG_RGROUP", "GPR_DAG_RSKEW", "GPR_DAG_RGROUP_MIN"};
  for (int k = 0; k < 3; ++k) {
    if (argc > 3 + k) gpr_set_knob(ctx, order_knobs[k], atof(argv[3 + k]));
    double v = 0;
    gpr_get_knob(ctx, order_knobs[k], &v);
    printf("%s=%d%s", order_knobs[k], (int)v, k < 2 ? " " : "\n");
  }
  std::vector<double> h((size_t)n * n);
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) h[(size_t)j * n + i] = (i == j) ? n + 1.0 : 1.0 / (1 + i + j);
  double* A;
  hipMalloc(&A, h.size() * 8);
  hipMemcpy(A, h.data(), h.size() * 8, hipMemcpyHostToDevice);
  std::atomic<int> done{0};
  int info = -7, rc = -7;
  // argv[2] = np > 0: the C3-style job instead (gpr_fit_predict, SE+SE+WN, d = 8): the DAG
  // launch then also solves the np + 1 right-hand sides [K(x, xp) | y]
  const int npred = argc > 2 ? atoi(argv[2]) : 0;
  const int d = npred < 0 ? 16 : 8;
  double* dkinv = nullptr;
  double *dx = nullptr, *dy = nullptr, *dxp = nullptr, *dal = nullptr, *dmu = nullptr, *dvar = nullptr;
  if (npred != 0) {
    std::vector<double> hx((size_t)d * n), hy(n), hxp((size_t)d * std::max(npred, 1));
    unsigned long long st = 88172645463325252ull;
    auto rnd = [&] { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (st >> 11) * (1.0 / 9007199254740992.0); };
    for (auto& v : hx) v = rnd();
    for (auto& v : hxp) v = rnd();
    for (int i = 0; i < n; ++i) {
      double s = 0;
      for (int k = 0; k < d; ++k) s += hx[(size_t)i * d + k];
      hy[i] = std::sin(s) * std::sin(s);
    }
    hipMalloc(&dx, hx.size() * 8); hipMemcpy(dx, hx.data(), hx.size() * 8, hipMemcpyHostToDevice);
    hipMalloc(&dy, hy.size() * 8); hipMemcpy(dy, hy.data(), hy.size() * 8, hipMemcpyHostToDevice);
    hipMalloc(&dxp, hxp.size() * 8); hipMemcpy(dxp, hxp.data(), hxp.size() * 8, hipMemcpyHostToDevice);
    hipMalloc(&dal, (size_t)n * 8); hipMalloc(&dmu, (size_t)std::max(npred, 1) * 8);
    hipMalloc(&dvar, (size_t)std::max(npred, 1) * 8);
    if (npred < 0) hipMalloc(&dkinv, (size_t)n * n * 8);
  }
  std::thread th([&] {
    for (int rep = 0; rep < 2; ++rep) {
      if (npred < 0) {
        const int kinds[2] = {GPR_SE, GPR_WN};
        std::vector<double> hp{1.0};
        for (int k = 0; k < d; ++k) hp.push_back(3.0 * std::sqrt(8.0 / d));
        hp.push_back(0.1);
        rc = gpr_fit_kinv(ctx, kinds, 2, hp.data(), d, dx, n, dy, 1, n, 1e-8, A, n, dal, dkinv, n,
                          &info);
      } else if (npred > 0) {
        const int kinds[3] = {GPR_SE, GPR_SE, GPR_WN};
        std::vector<double> hp;
        for (int p = 0; p < 2; ++p) {
          hp.push_back(1.0);
          for (int k = 0; k < d; ++k) hp.push_back(3.0);
        }
        hp.push_back(0.1);
        rc = gpr_fit_predict(ctx, kinds, 3, hp.data(), d, dx, n, dy, 1, n, 1e-8, A, n, dal, dxp,
                             npred, GPR_PREDICT_DIAG, dmu, dvar, npred, nullptr, &info);
      } else {
        hipMemcpy(A, h.data(), h.size() * 8, hipMemcpyHostToDevice);
        rc = gpr_potrf_upper(ctx, A, n, n, &info);
      }
    }
    done = 1;
  });
  hipStream_t s;
  hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  std::vector<int> tr(4096);
  for (int it = 0; it < 300 && !done; ++it) {
    std::this_thread::sleep_for(std::chrono::milliseconds(100));
    if (it % 10 == 9) {
      gpr_debug_dag_trace(tr.data(), s);
      printf("t=%.1fs:", (it + 1) * 0.1);
      for (int b = 0; b < 3; ++b) printf(" wg%d[task %d phase %d waves %d %d %d %d]", b, tr[b * 8], tr[b * 8 + 1], tr[b*8+4], tr[b*8+5], tr[b*8+6], tr[b*8+7]);
      printf("\n");
      fflush(stdout);
    }
  }
  if (!done) {
    gpr_debug_dag_trace(tr.data(), s);
    printf("HUNG: ");
    for (int b = 0; b < 32; ++b) printf(" wg%d[%d,%d,it%d,sync%d]", b, tr[b * 8], tr[b * 8 + 1], tr[b * 8 + 3], tr[b * 8 + 2]);
    printf("\n");
    fflush(stdout);
    _exit(3);
  }
  th.join();
  printf("n=%d rc=%d info=%d %s\n", n, rc, info, gpr_last_error(ctx));
  // phase profile of the last launch: per-workgroup sums (10-ns ticks) in slots 2..7
  gpr_debug_dag_trace(tr.data(), s);
  double w = 0, ac = 0, fa = 0, tri = 0, all = 0, nt = 0, mx = 0;
  int nwg = 0;
  for (int b = 0; b < 512; ++b) {
    if (tr[b * 8 + 7] <= 0) continue;
    ++nwg;
    w += tr[b * 8 + 2]; ac += tr[b * 8 + 3]; fa += tr[b * 8 + 4]; tri += tr[b * 8 + 5];
    all += tr[b * 8 + 6]; nt += tr[b * 8 + 7];
    mx = std::max(mx, (double)tr[b * 8 + 6]);
  }
  if (nwg)
    printf("profile: %d workgroups, %.0f tasks; mean per workgroup (ms): total %.3f (max %.3f) "
           "wait %.3f accum %.3f factor %.3f trsm %.3f other %.3f\n", nwg, nt, all / nwg * 1e-5,
           mx * 1e-5, w / nwg * 1e-5, ac / nwg * 1e-5, fa / nwg * 1e-5, tri / nwg * 1e-5,
           (all - w - ac - fa - tri) / nwg * 1e-5);
  // the diagonal factor's phases, mean per diagonal task over every launch of the run (us)
  unsigned long long ph[16];
  gpr_debug_diag_phases(ph, 0);
  if (ph[8])
    printf("diag factor (%llu tasks), mean us: band elim %.2f %.2f %.2f %.2f  trailing %.2f %.2f %.2f"
           "  inverse %.2f  total %.2f\n", ph[8], ph[0] * 1e-2 / ph[8], ph[2] * 1e-2 / ph[8],
           ph[4] * 1e-2 / ph[8], ph[6] * 1e-2 / ph[8], ph[1] * 1e-2 / ph[8], ph[3] * 1e-2 / ph[8],
           ph[5] * 1e-2 / ph[8], ph[7] * 1e-2 / ph[8],
           (ph[0] + ph[1] + ph[2] + ph[3] + ph[4] + ph[5] + ph[6] + ph[7]) * 1e-2 / ph[8]);
  if (ph[8])
    printf("  wave 0 inside the bands (sum of 4 bands), mean us: loads+selects %.2f  elimination %.2f"
           "  stores %.2f\n", ph[9] * 1e-2 / ph[8], ph[10] * 1e-2 / ph[8], ph[11] * 1e-2 / ph[8]);
  return 0;
}
