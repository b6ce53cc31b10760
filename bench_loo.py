"""Leave-one-out training benchmark at the C4 shape (SE+WN, N = 16384, d = 16).

  python bench_loo.py [--reps R --warmup W --n N --d D]

One JSON line with, all in one process on the same device buffers and alternating the two sides
of every comparison:

  loss_grad     log_loss_grad_(LeaveOneOut(), ...) against log_loss_grad_(MarginalLikelihood(), ...)
                on one MllGradCache: per side the median, minimum and maximum over --reps calls
                (host clock around calls that end in a device synchronise), and the ratio of the
                medians.  By flop count: about 2 n^3 (fit n^3 / 3, Z n^3 / 3, Z^T Z n^3 / 3, the
                SYRK n^3) against n^3.
  split         the LOO evaluation's parts: gpr_fit_kinv (device events), and from the library's
                own per-class event timers inside gpr_loo_grad the small kernels (class 15: terms,
                b = P f_alpha, S = diag(s) P, pre-fill, mirror), the SYRK (class 16, with its
                flops n^2 (n + 1) -> TF/s) and the fused gradient pass (class 4)
  loss_only     gpr_fit_loo + gpr_loo against gpr_fit + gpr_mll (what a zeroth-order method pays)
  vs_cv_loo     gpr_fit_loo + gpr_loo against cv_loo (gpr_cv_kfold with n one-point folds) on the
                same points

The four criteria differ in the per-point terms only; --crit picks the one that is timed.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "gaussianprocessregression.jl_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FP64_PEAK = 78.6  # TF/s, MFMA


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--crit", default="LogPredictive",
                    choices=["LogPredictive", "MSE", "ChiSq", "Mahalanobis"])
    return ap.parse_args()


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()),
            "reps": int(ts.size)}


def main():
    a = parse()
    import gpr_amd as G
    from gpr_amd import _lib

    lib = _lib.lib
    ctx = G.Context(0)
    N, d = a.n, a.d
    hp = np.r_[1.0, [3.0 * math.sqrt(8.0 / d)] * d, 0.1]
    x = np.random.default_rng(0).random((d, N))
    y = np.sin(x.sum(0)) ** 2
    cov = G.SquaredExp() + G.WhiteNoise()
    md = G.GPRModel(cov, hp, x, y, ctx=ctx)
    loo, mll = G.LeaveOneOut(getattr(G, a.crit)()), G.MarginalLikelihood()
    crit = G.core._loo_crit(loo)
    tc = G.MllGradCache(md)
    tl, tm = G.LooLossCache(md), G.MllLossCache(md)
    log_hp = np.log(hp)
    D = len(hp)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def timed(f):
        ctx.sync()
        t0 = time.perf_counter()
        f()
        ctx.sync()
        return time.perf_counter() - t0

    def alternate(fa, fb):
        """--warmup calls of each side, then --reps timed calls of each, alternating."""
        for _ in range(a.warmup):
            fa()
            fb()
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(timed(fa))
            tb.append(timed(fb))
        return stats(ta), stats(tb)

    out = {}
    with torch.cuda.stream(ctx.stream):
        # ---- loss + gradient ------------------------------------------------------------------
        g_loo, g_mll = np.zeros(D), np.zeros(D)
        vals = {}

        def lg_loo():
            vals["loo"] = G.log_loss_grad_(loo, True, g_loo, log_hp, md, tc)

        def lg_mll():
            vals["mll"] = G.log_loss_grad_(mll, True, g_mll, log_hp, md, tc)

        s_loo, s_mll = alternate(lg_loo, lg_mll)
        out["loss_grad"] = {"loo": s_loo, "mll": s_mll,
                            "ratio_of_medians": s_loo["median_ms"] / s_mll["median_ms"],
                            "loo_value": vals["loo"], "mll_value": vals["mll"],
                            "finite": bool(np.isfinite(g_loo).all() and np.isfinite(g_mll).all())}

        # ---- the LOO evaluation's parts ---------------------------------------------------------
        kinds, nk = G.core._kinds_arr(cov)
        _, hpp = G.core._hp_arr(hp)
        info = ctypes.c_int(0)
        gp = g_loo.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        val = ctypes.c_double(0.0)

        def fit_kinv():
            ctx.check(lib.gpr_fit_kinv(ctx.h, kinds, nk, hpp, d, P(md.dx()), N, P(md.dsample()), 1, N,
                                       1e-8, P(tc.kchol_base), tc.ld, P(tc.alpha), P(tc.Kinv), N,
                                       ctypes.byref(info)), "gpr_fit_kinv")

        def loo_grad():
            ctx.check(lib.gpr_loo_grad(ctx.h, kinds, nk, hpp, d, P(md.dx()), N, P(tc.Kinv), N,
                                       P(tc.alpha), 1e-8, crit, 1, ctypes.byref(val), gp),
                      "gpr_loo_grad")

        fit_ms, cls_ms = [], {4: [], 15: [], 16: []}
        syrk_flops = 0.0
        for _ in range(a.reps):
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record(ctx.stream)
            fit_kinv()
            e1.record(ctx.stream)
            ctx.sync()
            fit_ms.append(e0.elapsed_time(e1))
            ctx.check(lib.gpr_timing_enable(ctx.h, 1))
            ctx.check(lib.gpr_timing_reset(ctx.h))
            loo_grad()
            for c in cls_ms:
                ms, nl, fl = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
                ctx.check(lib.gpr_timing_get(ctx.h, c, ctypes.byref(ms), ctypes.byref(nl),
                                             ctypes.byref(fl)))
                cls_ms[c].append(ms.value)
                if c == 16:
                    syrk_flops = fl.value
            ctx.check(lib.gpr_timing_enable(ctx.h, 0))
        syrk_ms = float(np.median(cls_ms[16]))
        out["split"] = {"fit_kinv_ms": float(np.median(fit_ms)),
                        "small_kernels_ms": float(np.median(cls_ms[15])),
                        "syrk_ms": syrk_ms, "syrk_ms_min_max": [min(cls_ms[16]), max(cls_ms[16])],
                        "grad_pass_ms": float(np.median(cls_ms[4])),
                        "syrk_flops": syrk_flops,
                        "syrk_TFLOPs": syrk_flops / (syrk_ms * 1e-3) / 1e12,
                        "syrk_frac_of_fp64_mfma_peak": syrk_flops / (syrk_ms * 1e-3) / 1e12 / FP64_PEAK}

        # ---- loss only ----------------------------------------------------------------------------
        s_a, s_b = alternate(lambda: G.loss(loo, hp, md, tl), lambda: G.loss(mll, hp, md, tm))
        out["loss_only"] = {"fit_loo+loo": s_a, "fit+mll": s_b,
                            "ratio_of_medians": s_a["median_ms"] / s_b["median_ms"]}

        # ---- against cv_loo on the same points ----------------------------------------------------
        s_a, s_b = alternate(lambda: G.loss(loo, hp, md, tl), lambda: G.cv_loo(md, x, y))
        out["vs_cv_loo"] = {"fit_loo+loo": s_a, "cv_loo": s_b,
                            "ratio_of_medians": s_a["median_ms"] / s_b["median_ms"]}

    print(json.dumps({
        "metric": "LOO loss + gradient evaluations/s (C4 shape)",
        "value": 1e3 / out["loss_grad"]["loo"]["median_ms"],
        "unit": "log_loss_grad! evaluations/s (N=%d, d=%d, D=%d)" % (N, d, D),
        "higher_is_better": True, "dtype": "f64", "crit": a.crit,
        "data": "synthetic (x ~ U[0,1)^(d x N) seeded, y = sin(sum x)^2)",
        "config": {"workload": f"LOO loss+grad SE+WN N={N} d={d}", "reps": a.reps,
                   "warmup": a.warmup},
        **out,
    }), flush=True)


if __name__ == "__main__":
    main()
