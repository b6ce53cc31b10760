"""Periodic benchmark: what the 2d-wide embedded features of a Periodic part add to the K assembly,
to the fit + posterior job and to the MLL + gradient evaluation, on one MI355X.

  python bench_periodic.py [--steps K --warmup W]

One JSON line with four measurements (HIP events on the context stream, median of --steps after
--warmup, min and max beside every median; descriptions run alternately in one loop so that
drift hits every description alike):
  kbuild        the full symmetric K (gpr_kernel, GPR_SELF) at N = 32768, d = 8 for SE+SE+WN,
                SE+PER+WN and PER+WN, as 8 N^2 bytes / time against the 8 TB/s HBM peak (feature
                width 8, S = 2 k-steps, against 16, S = 4)
  kbuild_fit    the K assembly inside gpr_fit for the same descriptions (timing class 0: the
                upper-only build where the description takes it), with the bytes it wrote
  job           the C3-shaped gpr_fit_predict (np = 8192, diagonal variance), SE+PER+WN against
                SE+SE+WN
  mll_grad      the C4-shaped evaluation (N = 16384, d = 16: gpr_fit_kinv, gpr_mll, gpr_mll_grad
                with the log-scale chain rule) for SE+WN and PER+WN, ms per evaluation, and the
                gradient pass alone
Synthetic data as bench.py: x ~ U[0,1)^(d x n) seed 0, y = sin(sum x)^2, test points seed 1; hp
sigma = 1, sigma_n = 0.1, SquaredExp l = 3 sqrt(8/d); Periodic l = 0.75 sqrt(8/d), p_k = 0.5 +
0.1 k (the run time of every kernel here is independent of the hp values).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "gaussianprocessregression.jl_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0
KIND = {"SE": 1, "WN": 2, "PER": 5}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--np", type=int, default=8192, dest="npred")
    ap.add_argument("--mll-n", type=int, default=16384)
    ap.add_argument("--mll-d", type=int, default=16)
    ap.add_argument("--mll-steps", type=int, default=3)
    return ap.parse_args()


def kinds_of(name):
    return [KIND[k] for k in name.split("+")]


def default_hp(kinds, d, noise=0.1):
    hp = []
    for k in kinds:
        if k == KIND["WN"]:
            hp += [noise]
        elif k == KIND["PER"]:
            hp += [1.0] + [0.75 * math.sqrt(8.0 / d)] * d + [0.5 + 0.1 * i for i in range(d)]
        else:
            hp += [1.0] + [3.0 * math.sqrt(8.0 / d)] * d
    return np.array(hp, dtype=np.float64)


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "runs": len(ms)}


def main():
    a = parse()
    import gpr_amd as G
    from gpr_amd import _lib

    lib = _lib.lib
    ctx = G.Context(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dpp = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731

    def timed_call(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.stream)
        f()
        e1.record(ctx.stream)
        ctx.sync()
        return e0.elapsed_time(e1)

    def kbuild_class():
        ms, ln, fl = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
        lib.gpr_timing_get(ctx.h, 0, ctypes.byref(ms), ctypes.byref(ln), ctypes.byref(fl))
        return ms.value, fl.value

    out = {"metric": "Periodic against SquaredExp on one MI355X (K assembly, fit + posterior job, "
                     "MLL + gradient)",
           "steps": a.steps, "warmup": a.warmup, "dtype": "f64"}
    with torch.cuda.stream(ctx.stream):
        n, d, npred = a.n, a.d, a.npred
        x = np.random.default_rng(0).random((d, n))
        y = np.sin(x.sum(0)) ** 2
        xp = np.random.default_rng(1).random((d, npred))
        dx, dy, dxp = ctx.colmajor(x), ctx.colmajor(y), ctx.colmajor(xp)
        K, alpha = ctx.empty(n, n), ctx.empty(n)
        mu, var, work = ctx.empty(npred), ctx.empty(npred), ctx.empty(npred + 1, n)
        info = ctypes.c_int(0)
        names = ["SE+SE+WN", "SE+PER+WN", "PER+WN"]
        desc = {}
        for nm in names:
            kinds = kinds_of(nm)
            desc[nm] = ((ctypes.c_int * len(kinds))(*kinds), len(kinds), default_hp(kinds, d))

        def kernel(nm):
            karr, nk, hp = desc[nm]
            ctx.check(lib.gpr_kernel(ctx.h, karr, nk, dpp(hp), d, P(dx), n, None, n, 1, 1e-8, P(K), n),
                      "gpr_kernel")

        def fit(nm):
            karr, nk, hp = desc[nm]
            ctx.check(lib.gpr_fit(ctx.h, karr, nk, dpp(hp), d, P(dx), n, P(dy), 1, n, 1e-8, P(K), n,
                                  P(alpha), ctypes.byref(info)), "gpr_fit")
            if info.value != 0:
                raise RuntimeError(f"{nm}: K not positive definite, info={info.value}")

        def job(nm):
            karr, nk, hp = desc[nm]
            ctx.check(lib.gpr_fit_predict(ctx.h, karr, nk, dpp(hp), d, P(dx), n, P(dy), 1, n, 1e-8,
                                          P(K), n, P(alpha), P(dxp), npred, 1, P(mu), P(var), npred,
                                          P(work), ctypes.byref(info)), "gpr_fit_predict")
            if info.value != 0:
                raise RuntimeError(f"{nm}: K not positive definite, info={info.value}")

        # ---- 1. the full symmetric K ---------------------------------------------------------
        t = {nm: [] for nm in names}
        finite = {}
        for i in range(a.warmup + a.steps):
            for nm in names:
                ms = timed_call(lambda: kernel(nm))
                if i >= a.warmup:
                    t[nm].append(ms)
                if i == 0:
                    finite[nm] = bool(torch.isfinite(K[:64]).all())
        kb = {}
        for nm in names:
            st = stats(t[nm])
            gbs = 8.0 * n * n / (st["median_ms"] * 1e-3) / 1e9
            kb[nm] = {**st, "GBps": gbs, "hbm_frac": gbs / HBM_PEAK_GBS, "finite": finite[nm]}
        ref = kb["SE+SE+WN"]["median_ms"]
        out["kbuild"] = {"n": n, "d": d, "bytes": 8.0 * n * n, **kb,
                         "ratio_SE+PER_over_SE+SE": kb["SE+PER+WN"]["median_ms"] / ref,
                         "ratio_PER_over_SE+SE": kb["PER+WN"]["median_ms"] / ref}

        # ---- 2. the K assembly inside gpr_fit (timing class 0) -------------------------------
        t = {nm: [] for nm in names}
        nbytes = {}
        for i in range(a.warmup + a.steps):
            for nm in names:
                lib.gpr_timing_reset(ctx.h)
                lib.gpr_timing_enable(ctx.h, 1)
                fit(nm)
                ctx.sync()
                lib.gpr_timing_enable(ctx.h, 0)
                ms, nbytes[nm] = kbuild_class()
                if i >= a.warmup:
                    t[nm].append(ms)
        kf = {}
        for nm in names:
            st = stats(t[nm])
            gbs = nbytes[nm] / (st["median_ms"] * 1e-3) / 1e9
            kf[nm] = {**st, "bytes": nbytes[nm], "upper_only": nbytes[nm] < 6.0 * n * n,
                      "GBps": gbs, "hbm_frac": gbs / HBM_PEAK_GBS}
        ref = kf["SE+SE+WN"]["median_ms"]
        out["kbuild_fit"] = {"n": n, "d": d, **kf,
                             "ratio_SE+PER_over_SE+SE": kf["SE+PER+WN"]["median_ms"] / ref,
                             "ratio_PER_over_SE+SE": kf["PER+WN"]["median_ms"] / ref}

        # ---- 3. the C3-shaped job ------------------------------------------------------------
        jn = ["SE+SE+WN", "SE+PER+WN"]
        t = {nm: [] for nm in jn}
        for i in range(a.warmup + a.steps):
            for nm in jn:
                ms = timed_call(lambda: job(nm))
                if i >= a.warmup:
                    t[nm].append(ms)
        jb = {nm: {**stats(t[nm])} for nm in jn}
        jb["SE+PER+WN"]["mu_var_finite"] = bool(torch.isfinite(mu).all() and torch.isfinite(var).all())
        out["job"] = {"n": n, "d": d, "np": npred, **jb,
                      "ratio_SE+PER_over_SE+SE":
                          jb["SE+PER+WN"]["median_ms"] / jb["SE+SE+WN"]["median_ms"]}
        del K, work

        # ---- 4. the C4-shaped MLL + gradient evaluation --------------------------------------
        N, d2 = a.mll_n, a.mll_d
        x = np.random.default_rng(0).random((d2, N))
        y = np.sin(x.sum(0)) ** 2
        dx, dy = ctx.colmajor(x), ctx.colmajor(y)
        K, Kinv, alpha = ctx.empty(N, N), ctx.empty(N, N), ctx.empty(N)
        mllv = ctypes.c_double(0.0)
        mn = ["SE+WN", "PER+WN"]
        ev, gr, res = {}, {}, {}
        for nm in mn:
            kinds = kinds_of(nm)
            hp = default_hp(kinds, d2)
            karr = (ctypes.c_int * 2)(*kinds)
            g = np.zeros(len(hp))
            res[nm] = g

            def fitk(karr=karr, hp=hp):
                ctx.check(lib.gpr_fit_kinv(ctx.h, karr, 2, dpp(hp), d2, P(dx), N, P(dy), 1, N, 1e-8,
                                           P(K), N, P(alpha), P(Kinv), N, ctypes.byref(info)),
                          "fit_kinv")
                if info.value != 0:
                    raise RuntimeError(f"not PD: info={info.value}")
                ctx.check(lib.gpr_mll(ctx.h, P(K), N, N, P(dy), P(alpha), ctypes.byref(mllv)), "mll")

            def grad(karr=karr, hp=hp, g=g):
                ctx.check(lib.gpr_mll_grad(ctx.h, karr, 2, dpp(hp), d2, P(dx), N, P(Kinv), N, P(alpha),
                                           1e-8, 1, dpp(g)), "mll_grad")

            ev[nm], gr[nm] = (lambda f=fitk, g_=grad: (f(), g_())), grad
        te, tg, mv = {nm: [] for nm in mn}, {nm: [] for nm in mn}, {}
        for i in range(a.warmup + a.mll_steps):
            for nm in mn:  # (the gradient pass follows its own fit: Kinv and alpha are its)
                ms_e = timed_call(ev[nm])
                mv[nm] = mllv.value
                ms_g = timed_call(gr[nm])
                if i >= a.warmup:
                    te[nm].append(ms_e)
                    tg[nm].append(ms_g)
        mg = {nm: {"evaluation": stats(te[nm]), "grad_pass": stats(tg[nm]), "mll": mv[nm],
                   "grad_finite": bool(np.isfinite(res[nm]).all())} for nm in mn}
        out["mll_grad"] = {
            "n": N, "d": d2, **mg,
            "ratio_PER_over_SE_evaluation":
                mg["PER+WN"]["evaluation"]["median_ms"] / mg["SE+WN"]["evaluation"]["median_ms"],
            "ratio_PER_over_SE_grad_pass":
                mg["PER+WN"]["grad_pass"]["median_ms"] / mg["SE+WN"]["grad_pass"]["median_ms"],
        }
        ctx.sync()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
