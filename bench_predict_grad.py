"""Posterior-gradient benchmark: the two fused passes of gpr_predict_grad against the cross K build
of the same shape, on one MI355X.

  python bench_predict_grad.py [--steps K --warmup W]

One JSON line.  At the C3 shape (N = 32768, d = 8, np = 8192) and for SE+SE+WN, SE+M52+WN and
SE+PER+WN, in one process (descriptions and measurements alternate in one loop, so that drift hits
all alike; median of --steps after --warmup, min and max beside every median):
  cross       gpr_kernel(..., GPR_CROSS): K(x, xp), N x np -- the yardstick (HIP events)
  mean_pass   gpr_predict_grad(want_var = 0): d mu / d xp (HIP events around the call)
  call        gpr_predict_grad(want_var = 1) as a whole (HIP events; --call-steps after
              --call-warmup), and from the library's timing classes inside it:
  solve       the solve that makes Q = K^-1 K(x, xp) from the fitted factor (class 10; by
              Z = U^-T and two MFMA products at this shape, GPR_PGRAD_SOLVE),
  var_pass    the variance pass alone, without the cross build and the solve (class 9),
  mean_pass_in_call   the mean pass (class 8)
and once, after the loops, solve_by_sweeps: the same solve by gpr_potrs_upper's sweeps
(GPR_PGRAD_SOLVE=0; one call of one description, --no-sweeps skips it),
and every pass as a ratio to the cross build.  The mean pass evaluates the same exponentials as
the cross build, adds about 2 d FMAs per element and stores nothing; the variance pass reads the
8 N np bytes of Q that the cross build writes.
Synthetic data as bench.py: x ~ U[0,1)^(d x n) seed 0, y = sin(sum x)^2, test points seed 1; hp
sigma = 1, sigma_n = 0.1, SquaredExp / Matern l = 3 sqrt(8/d); Periodic l = 0.75 sqrt(8/d), p_k =
0.5 + 0.1 k (the run time of every kernel here is independent of the hp values).
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

KIND = {"SE": 1, "WN": 2, "M52": 4, "PER": 5}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--np", type=int, default=8192, dest="npred")
    ap.add_argument("--call-steps", type=int, default=5)
    ap.add_argument("--call-warmup", type=int, default=1)
    ap.add_argument("--no-sweeps", action="store_true")
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
        ctx.check(lib.gpr_timing_get(ctx.h, c, ctypes.byref(ms), ctypes.byref(ln), ctypes.byref(fl)))
        return ms.value

    n, d, m = a.n, a.d, a.npred
    out = {"metric": "posterior gradients w.r.t. the test inputs against the cross K build on one "
                     "MI355X", "n": n, "d": d, "np": m, "steps": a.steps, "warmup": a.warmup,
           "call_steps": a.call_steps, "call_warmup": a.call_warmup,
           "dtype": "f64", "slab": ctx.get_knob("GPR_PGRAD_SLAB"), "Q_bytes": 8.0 * n * m}
    names = ["SE+SE+WN", "SE+M52+WN", "SE+PER+WN"]
    with torch.cuda.stream(ctx.stream):
        x = np.random.default_rng(0).random((d, n))
        y = np.sin(x.sum(0)) ** 2
        xp = np.random.default_rng(1).random((d, m))
        dx, dy, dxp = ctx.colmajor(x), ctx.colmajor(y), ctx.colmajor(xp)
        U = {nm: ctx.empty(n, n) for nm in names}   # a fitted factor per description
        alpha = {nm: ctx.empty(n) for nm in names}
        Q = ctx.empty(m, n)
        gm, gv = ctx.empty(m, d), ctx.empty(m, d)
        info = ctypes.c_int(0)
        desc = {}
        for nm in names:
            kinds = kinds_of(nm)
            desc[nm] = ((ctypes.c_int * len(kinds))(*kinds), len(kinds), default_hp(kinds, d))
            karr, nk, hp = desc[nm]
            ctx.check(lib.gpr_fit(ctx.h, karr, nk, dpp(hp), d, P(dx), n, P(dy), 1, n, 1e-8, P(U[nm]), n,
                                  P(alpha[nm]), ctypes.byref(info)), "gpr_fit")
            if info.value != 0:
                raise RuntimeError(f"{nm}: K not positive definite, info={info.value}")

        def cross(nm):
            karr, nk, hp = desc[nm]
            ctx.check(lib.gpr_kernel(ctx.h, karr, nk, dpp(hp), d, P(dx), n, P(dxp), m, 0, 1e-8, P(Q), n),
                      "gpr_kernel")

        def pgrad(nm, want_var):
            karr, nk, hp = desc[nm]
            ctx.check(lib.gpr_predict_grad(ctx.h, karr, nk, dpp(hp), d, P(dx), n, P(U[nm]), n,
                                           P(alpha[nm]), 1, P(dxp), m, want_var, 1e-8, P(gm),
                                           P(gv) if want_var else None, P(Q) if want_var else None),
                      "gpr_predict_grad")

        keys = ["cross", "mean_pass", "call", "solve", "mean_pass_in_call", "var_pass"]
        t = {nm: {k: [] for k in keys} for nm in names}
        finite = {}
        # the cheap pair, alternating
        for i in range(a.warmup + a.steps):
            for nm in names:
                r = {"cross": timed_call(lambda: cross(nm)), "mean_pass": timed_call(lambda: pgrad(nm, 0))}
                if i >= a.warmup:
                    for k, v in r.items():
                        t[nm][k].append(v)
        # the whole call (its solve is hundreds of ms: repeated less often)
        for i in range(a.call_warmup + a.call_steps):
            for nm in names:
                lib.gpr_timing_reset(ctx.h)
                lib.gpr_timing_enable(ctx.h, 1)
                r = {"call": timed_call(lambda: pgrad(nm, 1))}
                lib.gpr_timing_enable(ctx.h, 0)
                r["solve"] = timing_class(10)
                r["mean_pass_in_call"], r["var_pass"] = timing_class(8), timing_class(9)
                finite[nm] = bool(torch.isfinite(gm).all() and torch.isfinite(gv).all())
                if i >= a.call_warmup:
                    for k, v in r.items():
                        t[nm][k].append(v)
        for nm in names:
            res = {k: stats(t[nm][k]) for k in keys}
            ref = res["cross"]["median_ms"]
            res["finite"] = finite[nm]
            res["cross_GBps"] = 8.0 * n * m / (ref * 1e-3) / 1e9
            res["var_pass_Q_read_GBps"] = 8.0 * n * m / (res["var_pass"]["median_ms"] * 1e-3) / 1e9
            for k in ("solve", "mean_pass", "var_pass", "call"):
                res[f"ratio_{k}_over_cross"] = res[k]["median_ms"] / ref
            out[nm] = res
        if not a.no_sweeps:  # one call with the solve by sweeps (tens of seconds at the C3 shape)
            ctx.set_knob("GPR_PGRAD_SOLVE", 0)
            lib.gpr_timing_reset(ctx.h)
            lib.gpr_timing_enable(ctx.h, 1)
            ms = timed_call(lambda: pgrad(names[0], 1))
            lib.gpr_timing_enable(ctx.h, 0)
            out["solve_by_sweeps"] = {"description": names[0], "call_ms": ms, "solve_ms": timing_class(10),
                                      "runs": 1}
            ctx.set_knob("GPR_PGRAD_SOLVE", -1)
        ctx.sync()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
