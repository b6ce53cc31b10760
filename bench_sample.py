"""Sampling benchmark: the device normal generator, the triangular product from a factor buffer
and the fused prior sample (src/distributions.jl) on one MI355X.

  python bench_sample.py [--steps K --warmup W]

One JSON line with three measurements (HIP events on the context stream, median of --steps
after --warmup, min and max beside every median):
  randn       gpr_randn, 2^28 elements (2 GiB written), GB/s -- reported beside the pure-store
              ceilings of bench.py's `kbuild_store_ceiling` probe, taken in this same process
  mvn_sample  gpr_mvn_sample, S = mu 1^T + U^T Z at n = 32768, ns = 1024 from the factor buffer
              the fused call left (K below the diagonal), TF/s counting n^2 ns flops; and, run
              alternately in the same loop, the UNMASKED kend_from_m GEMM on a copy of U whose
              strict lower triangle is zeroed (what the product cost before a factor buffer
              could be multiplied in place)
  prior       gpr_sample_prior at the C3 kernel (SE+SE+WN, n = 32768, d = 8, ns = 1024): K
              assembly, K .+= 1e-7, dpotrf 'U' and the product in one call, ms
Synthetic data as bench.py: x ~ U[0,1)^(d x n) seed 0, hp sigma = 1, l = 3 sqrt(8/d),
sigma_n = 0.1; mu = sum(x); Z from gpr_randn(seed 1).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "gaussianprocessregression.jl_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (store_ceiling, default_hp, kinds_of: the headline bench's own helpers)

HBM_PEAK_GBS = 8000.0
FP64_PEAK_TF = 78.6


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--ns", type=int, default=1024)
    ap.add_argument("--kernel", default="SE+SE+WN")
    ap.add_argument("--randn-log2", type=int, default=28)
    return ap.parse_args()


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "runs": len(ms)}


def main():
    a = parse()
    import gpr_amd as G
    from gpr_amd import _lib

    lib = _lib.lib
    lib.gpr_debug_gemm_upper_p.restype = ctypes.c_int
    lib.gpr_debug_gemm_upper_p.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_int]
    ctx = G.Context(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    n, d, ns = a.n, a.d, a.ns

    def timed(f):
        """[ms] of --steps calls of f after --warmup, each between two events on the stream."""
        out = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            f()
            e1.record(ctx.stream)
            ctx.sync()
            if i >= a.warmup:
                out.append(e0.elapsed_time(e1))
        return out

    with torch.cuda.stream(ctx.stream):
        # ---- 1. gpr_randn ---------------------------------------------------------------
        cnt = 1 << a.randn_log2
        Zbig = ctx.empty(cnt)
        t_rn = stats(timed(lambda: ctx.check(lib.gpr_randn(ctx.h, 1, 0, P(Zbig), cnt), "randn")))
        head = Zbig[:1 << 20].cpu().numpy()
        del Zbig

        # ---- 3. fused prior sample at the C3 kernel (leaves the factor buffer for 2.) ----
        kinds = bench.kinds_of(a.kernel)
        hp = bench.default_hp(kinds, d)
        karr = (ctypes.c_int * len(kinds))(*kinds)
        hpp = hp.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        x = np.random.default_rng(0).random((d, n))
        dx, dmu = ctx.colmajor(x), ctx.colmajor(x.sum(0))
        K, Z, S = ctx.empty(n, n), ctx.empty(ns, n), ctx.empty(ns, n)
        ctx.check(lib.gpr_randn(ctx.h, 1, 0, P(Z), n * ns), "randn")
        info = ctypes.c_int(0)

        def prior():
            ctx.check(lib.gpr_sample_prior(ctx.h, karr, len(kinds), hpp, d, P(dx), n, P(dmu), 1e-7,
                                           1e-8, P(Z), ns, n, P(K), n, P(S), n, ctypes.byref(info)),
                      "sample_prior")
            if info.value != 0:
                raise RuntimeError(f"not PD: info={info.value}")

        t_prior = stats(timed(prior))
        s_fused = S.clone()
        ceiling = bench.store_ceiling(lib, ctx, ctx.empty(n, n), n)

        # ---- 2. masked product from the factor buffer vs the unmasked GEMM on triu(U) ----
        Uz = torch.tril(K)  # column-major upper triangle = torch's row-major lower one
        S2 = ctx.empty(ns, n)
        masked = lambda: ctx.check(lib.gpr_mvn_sample(ctx.h, P(K), n, n, P(dmu), P(Z), ns, n,  # noqa: E731
                                                      P(S), n), "mvn_sample")
        unmasked = lambda: ctx.check(lib.gpr_debug_gemm_upper_p(ctx.h, P(Uz), n, n, P(Z), ns, n,  # noqa: E731
                                                                P(S2), n), "gemm")
        tm, tu = [], []
        for i in range(a.warmup + a.steps):  # alternating, same process
            for f, acc in ((masked, tm), (unmasked, tu)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ctx.stream)
                f()
                e1.record(ctx.stream)
                ctx.sync()
                if i >= a.warmup:
                    acc.append(e0.elapsed_time(e1))
        t_m, t_u = stats(tm), stats(tu)
        same_as_fused = bool(torch.equal(S, s_fused))
        diff = float((S - (S2 + dmu[None, :])).abs().max() / S.abs().max())
        finite = bool(torch.isfinite(S).all())
        ctx.sync()

    flops = float(n) * n * ns
    tf = lambda st: flops / (st["median_ms"] * 1e-3) / 1e12  # noqa: E731
    rn_gbs = 8.0 * cnt / (t_rn["median_ms"] * 1e-3) / 1e9
    print(json.dumps({
        "metric": "GP sampling on one MI355X (randn, triangular product, fused prior sample)",
        "steps": a.steps, "warmup": a.warmup, "dtype": "f64",
        "randn": {"elements": cnt, **t_rn, "GBps": rn_gbs, "hbm_frac": rn_gbs / HBM_PEAK_GBS,
                  "mean": float(head.mean()), "var": float(head.var()),
                  "kbuild_store_ceiling": ceiling},
        "mvn_sample": {"n": n, "ns": ns, "flops_n2_ns": flops,
                       "masked_factor_buffer": {**t_m, "TFLOPs": tf(t_m)},
                       "unmasked_kend_from_m_on_triu_copy": {**t_u, "TFLOPs": tf(t_u)},
                       "masked_over_unmasked_median": t_m["median_ms"] / t_u["median_ms"],
                       "fp64_peak_frac_masked": tf(t_m) / FP64_PEAK_TF,
                       "max_rel_diff_masked_vs_unmasked": diff, "finite": finite,
                       "bitwise_equal_to_fused_call": same_as_fused},
        "prior": {"kernel": a.kernel, "n": n, "d": d, "ns": ns, **t_prior,
                  "samples_per_s": ns / (t_prior["median_ms"] * 1e-3)},
    }), flush=True)


if __name__ == "__main__":
    main()
