"""Product-kernel benchmark: SE*PER+WN against SE+PER+WN on one MI355X -- the same two stationary
parts, hence the same distances and exponentials per element; only what is done with the two
values differs (multiplied into one term, or added as two).

  python bench_product.py [--steps K --warmup W]

One JSON line (HIP events on the context stream, median of --steps after --warmup, min and max
beside every median; the two descriptions alternate in one loop in one process, so that drift hits
both alike), every measurement with its ratio product / sum:
  kbuild        the full symmetric K (gpr_kernel, GPR_SELF) at N = 32768, d = 8
  kbuild_fit    the K assembly inside gpr_fit (timing class 0: the upper-only build), with the
                bytes it wrote
  job           the C3-shaped gpr_fit_predict (np = 8192, diagonal variance)
  mll_grad      at the C4 shape (N = 16384, d = 16): gpr_fit_kinv + gpr_mll + gpr_mll_grad (log
                scale), ms per evaluation, and the gradient pass alone -- the sum takes the wide
                kernel's Periodic form, the product its PROD form (every factor of the term
                evaluated per factor)
  predict_grad  at the C3 shape: the mean pass (gpr_predict_grad, want_var = 0) and the variance
                pass alone (timing class 9 inside a want_var = 1 call)
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
SE, WN, PER, MUL = 1, 2, 5, 6
DESC = {"SE+PER+WN": [SE, PER, WN], "SE*PER+WN": [SE, MUL, PER, WN]}
SUM, PROD = "SE+PER+WN", "SE*PER+WN"


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
    ap.add_argument("--call-steps", type=int, default=3)
    return ap.parse_args()


def default_hp(kinds, d, noise=0.1):
    hp = []
    for k in kinds:
        if k == WN:
            hp += [noise]
        elif k == PER:
            hp += [1.0] + [0.75 * math.sqrt(8.0 / d)] * d + [0.5 + 0.1 * i for i in range(d)]
        elif k == SE:
            hp += [1.0] + [3.0 * math.sqrt(8.0 / d)] * d
    return np.array(hp, dtype=np.float64)


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "runs": len(ms)}


def pair(t, extra=None):
    """{sum, product, ratio} of two lists of times"""
    r = {nm: {**stats(t[nm]), **((extra or {}).get(nm, {}))} for nm in (SUM, PROD)}
    r["ratio_product_over_sum"] = r[PROD]["median_ms"] / r[SUM]["median_ms"]
    return r


def main():
    a = parse()
    import gpr_amd as G
    from gpr_amd import _lib

    lib = _lib.lib
    ctx = G.Context(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    dpp = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731

    def timed_call(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.stream)
        f()
        e1.record(ctx.stream)
        ctx.sync()
        return e0.elapsed_time(e1)

    def timing_class(c):
        ms, ln, fl = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
        lib.gpr_timing_get(ctx.h, c, ctypes.byref(ms), ctypes.byref(ln), ctypes.byref(fl))
        return ms.value, fl.value

    def describe(d):
        return {nm: ((ctypes.c_int * len(k))(*k), len(k), default_hp(k, d)) for nm, k in DESC.items()}

    out = {"metric": "SE*PER+WN against SE+PER+WN on one MI355X (K assembly, fit + posterior job, "
                     "MLL + gradient, posterior gradients)",
           "steps": a.steps, "warmup": a.warmup, "dtype": "f64"}
    names = [SUM, PROD]
    with torch.cuda.stream(ctx.stream):
        n, d, npred = a.n, a.d, a.npred
        x = np.random.default_rng(0).random((d, n))
        y = np.sin(x.sum(0)) ** 2
        xp = np.random.default_rng(1).random((d, npred))
        dx, dy, dxp = ctx.colmajor(x), ctx.colmajor(y), ctx.colmajor(xp)
        K, alpha = ctx.empty(n, n), ctx.empty(n)
        mu, var, work = ctx.empty(npred), ctx.empty(npred), ctx.empty(npred + 1, n)
        info = ctypes.c_int(0)
        desc = describe(d)

        def kernel(nm):
            karr, nk, hp = desc[nm]
            ctx.check(lib.gpr_kernel(ctx.h, karr, nk, dpp(hp), d, P(dx), n, None, n, 1, 1e-8, P(K), n),
                      "gpr_kernel")

        def fit(nm, dst, al):
            karr, nk, hp = desc[nm]
            ctx.check(lib.gpr_fit(ctx.h, karr, nk, dpp(hp), d, P(dx), n, P(dy), 1, n, 1e-8, P(dst), n,
                                  P(al), ctypes.byref(info)), "gpr_fit")
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
        ex = {nm: {} for nm in names}
        for i in range(a.warmup + a.steps):
            for nm in names:
                ms = timed_call(lambda: kernel(nm))
                if i >= a.warmup:
                    t[nm].append(ms)
                if i == 0:
                    ex[nm]["finite"] = bool(torch.isfinite(K[:64]).all())
        for nm in names:
            gbs = 8.0 * n * n / (stats(t[nm])["median_ms"] * 1e-3) / 1e9
            ex[nm].update(GBps=gbs, hbm_frac=gbs / HBM_PEAK_GBS)
        out["kbuild"] = {"n": n, "d": d, "bytes": 8.0 * n * n, **pair(t, ex)}

        # ---- 2. the K assembly inside gpr_fit (timing class 0) -------------------------------
        t = {nm: [] for nm in names}
        ex = {nm: {} for nm in names}
        for i in range(a.warmup + a.steps):
            for nm in names:
                lib.gpr_timing_reset(ctx.h)
                lib.gpr_timing_enable(ctx.h, 1)
                fit(nm, K, alpha)
                ctx.sync()
                lib.gpr_timing_enable(ctx.h, 0)
                ms, nbytes = timing_class(0)
                ex[nm] = {"bytes": nbytes, "upper_only": nbytes < 6.0 * n * n}
                if i >= a.warmup:
                    t[nm].append(ms)
        out["kbuild_fit"] = {"n": n, "d": d, **pair(t, ex)}

        # ---- 3. the C3-shaped job ------------------------------------------------------------
        t = {nm: [] for nm in names}
        ex = {nm: {} for nm in names}
        for i in range(a.warmup + a.steps):
            for nm in names:
                ms = timed_call(lambda: job(nm))
                ex[nm]["mu_var_finite"] = bool(torch.isfinite(mu).all() and torch.isfinite(var).all())
                if i >= a.warmup:
                    t[nm].append(ms)
        out["job"] = {"n": n, "d": d, "np": npred, **pair(t, ex)}
        del work

        # ---- 4. posterior gradients at the C3 shape ------------------------------------------
        U = {SUM: K, PROD: ctx.empty(n, n)}
        al = {nm: ctx.empty(n) for nm in names}
        for nm in names:
            fit(nm, U[nm], al[nm])
        Q = ctx.empty(npred, n)
        gm, gv = ctx.empty(npred, d), ctx.empty(npred, d)

        def pgrad(nm, want_var):
            karr, nk, hp = desc[nm]
            ctx.check(lib.gpr_predict_grad(ctx.h, karr, nk, dpp(hp), d, P(dx), n, P(U[nm]), n,
                                           P(al[nm]), 1, P(dxp), npred, want_var, 1e-8, P(gm),
                                           P(gv) if want_var else None, P(Q) if want_var else None),
                      "gpr_predict_grad")

        tm = {nm: [] for nm in names}
        for i in range(a.warmup + a.steps):
            for nm in names:
                ms = timed_call(lambda: pgrad(nm, 0))
                if i >= a.warmup:
                    tm[nm].append(ms)
        tv = {nm: [] for nm in names}
        ex = {nm: {} for nm in names}
        for i in range(1 + a.call_steps):
            for nm in names:
                lib.gpr_timing_reset(ctx.h)
                lib.gpr_timing_enable(ctx.h, 1)
                pgrad(nm, 1)
                ctx.sync()
                lib.gpr_timing_enable(ctx.h, 0)
                ex[nm]["finite"] = bool(torch.isfinite(gm).all() and torch.isfinite(gv).all())
                if i >= 1:
                    tv[nm].append(timing_class(9)[0])
        out["predict_grad"] = {"n": n, "d": d, "np": npred, "slab": ctx.get_knob("GPR_PGRAD_SLAB"),
                               "mean_pass": pair(tm), "var_pass": pair(tv, ex)}
        del K, U, Q

        # ---- 5. the C4-shaped MLL + gradient evaluation --------------------------------------
        N, d2 = a.mll_n, a.mll_d
        x = np.random.default_rng(0).random((d2, N))
        y = np.sin(x.sum(0)) ** 2
        dx2, dy2 = ctx.colmajor(x), ctx.colmajor(y)
        K2, Kinv, alpha2 = ctx.empty(N, N), ctx.empty(N, N), ctx.empty(N)
        mllv = ctypes.c_double(0.0)
        desc2 = describe(d2)
        res = {nm: np.zeros(len(desc2[nm][2])) for nm in names}

        def fitk(nm):
            karr, nk, hp = desc2[nm]
            ctx.check(lib.gpr_fit_kinv(ctx.h, karr, nk, dpp(hp), d2, P(dx2), N, P(dy2), 1, N, 1e-8,
                                       P(K2), N, P(alpha2), P(Kinv), N, ctypes.byref(info)), "fit_kinv")
            if info.value != 0:
                raise RuntimeError(f"{nm}: not PD: info={info.value}")
            ctx.check(lib.gpr_mll(ctx.h, P(K2), N, N, P(dy2), P(alpha2), ctypes.byref(mllv)), "mll")

        def grad(nm):
            karr, nk, hp = desc2[nm]
            ctx.check(lib.gpr_mll_grad(ctx.h, karr, nk, dpp(hp), d2, P(dx2), N, P(Kinv), N, P(alpha2),
                                       1e-8, 1, dpp(res[nm])), "mll_grad")

        te, tg = {nm: [] for nm in names}, {nm: [] for nm in names}
        ex = {nm: {} for nm in names}
        for i in range(a.warmup + a.mll_steps):
            for nm in names:  # (the gradient pass follows its own fit: Kinv and alpha are its)
                ms_e = timed_call(lambda: (fitk(nm), grad(nm)))
                ex[nm]["mll"] = mllv.value
                ms_g = timed_call(lambda: grad(nm))
                ex[nm]["grad_finite"] = bool(np.isfinite(res[nm]).all())
                if i >= a.warmup:
                    te[nm].append(ms_e)
                    tg[nm].append(ms_g)
        out["mll_grad"] = {"n": N, "d": d2, "evaluation": pair(te, ex), "grad_pass": pair(tg)}
        ctx.sync()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
