"""Append benchmark: conditioning a fitted model on m new observations with gpr_fit_append against
the full refit a user had to do before, on one MI355X.

  python bench_append.py [--steps K --warmup W --out FILE]

One JSON line, also written to --out (default profiles/r15_bench_append.json).  At the C3
description (SE+SE+WN, d = 8) and N = 32768 points in all, for m in {1, 16, 128} new points (and 32,
48, 64, which place the threshold of GPR_APPEND_SWEEP's auto rule) on a factor of n0 = N - m, in one process and one loop per m (the measurements alternate, so that drift
hits all alike; median of --steps after --warmup, min and max beside every median):
  append_sweep   gpr_fit_append with GPR_APPEND_SWEEP = 1 (HIP events around the call), and from
                 the library's timing class 11 inside it:
  solve_sweep    the skinny forward solve V = U^-T K(x, x_new) by the single-launch sweep
  append_trsm    gpr_fit_append with GPR_APPEND_SWEEP = 0, and
  solve_trsm     its class 11: the same solve by the GEMM-based route
  trsm           gpr_trsm_upper_trans on the same factor with m columns (the existing public route)
  fit            gpr_fit on all N points: what a user does today
Before every timed append the context's factor cache is put back on the n0-point factor by an
untimed gpr_potrs_upper, as a chain of appends finds it.  Reported ratios: fit / append (either
route), trsm / solve_sweep, and the sweep against the one-pass floor: the bytes of U's upper
triangle, 4 n0 (n0 + 1), at 8 TB/s.
Synthetic data as bench.py: x ~ U[0,1)^(d x n) seed 0, y = sin(sum x)^2; hp sigma = 1,
sigma_n = 0.1, l = 3 sqrt(8/d).
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

HBM_BYTES_PER_S = 8.0e12


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--m", type=int, nargs="+", default=[1, 16, 32, 48, 64, 128])
    ap.add_argument("--fit-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_bench_append.json"))
    return ap.parse_args()


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

    N, d = a.n, a.d
    kinds = [_lib.GPR_SE, _lib.GPR_SE, _lib.GPR_WN]
    karr, nk = (ctypes.c_int * 3)(*kinds), 3
    hp = np.array(([1.0] + [3.0 * math.sqrt(8.0 / d)] * d) * 2 + [0.1], dtype=np.float64)
    out = {"metric": "gpr_fit_append against the full refit and the skinny solve against the "
                     "existing route on one MI355X", "description": "SE+SE+WN", "n": N, "d": d,
           "steps": a.steps, "warmup": a.warmup, "fit_steps": a.fit_steps, "dtype": "f64",
           "auto_knob": ctx.get_knob("GPR_APPEND_SWEEP")}
    with torch.cuda.stream(ctx.stream):
        x = np.random.default_rng(0).random((d, N))
        y = np.sin(x.sum(0)) ** 2
        dx, dy = ctx.colmajor(x), ctx.colmajor(y)
        dK, dKfull = ctx.empty(N, N), ctx.empty(N, N)
        alpha_full = ctx.empty(N)
        info = ctypes.c_int(0)

        def fit(buf, n, alpha):
            ctx.check(lib.gpr_fit(ctx.h, karr, nk, dpp(hp), d, P(dx), n, P(dy), 1, N, 1e-8, P(buf), N,
                                  P(alpha), ctypes.byref(info)), "gpr_fit")
            if info.value != 0:
                raise RuntimeError(f"K not positive definite, info={info.value}")

        fit_ms = []
        for i in range(1 + a.fit_steps):
            t = timed_call(lambda: fit(dKfull, N, alpha_full))
            if i >= 1:
                fit_ms.append(t)
        out["fit"] = stats(fit_ms)
        a_full = alpha_full.cpu().numpy()
        for m in a.m:
            n0 = N - m
            alpha0, alpha1, scratch = ctx.empty(n0), ctx.empty(N), ctx.empty(n0)
            B = ctx.empty(m, n0)
            fit(dK, n0, alpha0)

            def recache():
                scratch.copy_(alpha0)
                ctx.check(lib.gpr_potrs_upper(ctx.h, P(dK), n0, N, P(scratch), 1, n0), "gpr_potrs_upper")

            def append(route):
                ctx.set_knob("GPR_APPEND_SWEEP", route)
                rc = lib.gpr_fit_append(ctx.h, karr, nk, dpp(hp), d, P(dx), n0, m, P(dy), 1, N, 1e-8,
                                        P(dK), N, P(alpha0), P(alpha1), ctypes.byref(info))
                ctx.check(rc, "gpr_fit_append")
                if info.value != 0:
                    raise RuntimeError(f"append not positive definite, info={info.value}")

            def trsm():
                ctx.check(lib.gpr_trsm_upper_trans(ctx.h, P(dK), n0, N, P(B), m, n0),
                          "gpr_trsm_upper_trans")

            keys = ["append_sweep", "solve_sweep", "append_trsm", "solve_trsm", "trsm"]
            t = {k: [] for k in keys}
            err = {}
            for i in range(a.warmup + a.steps):
                r = {}
                for route, name in ((1, "sweep"), (0, "trsm")):
                    recache()
                    ctx.sync()
                    lib.gpr_timing_reset(ctx.h)
                    lib.gpr_timing_enable(ctx.h, 1)
                    r[f"append_{name}"] = timed_call(lambda: append(route))
                    lib.gpr_timing_enable(ctx.h, 0)
                    r[f"solve_{name}"] = timing_class(11)
                    got = alpha1.cpu().numpy()
                    err[name] = float(np.abs(got - a_full).max() / np.abs(a_full).max())
                recache()
                B.copy_(dK[n0:, :n0])  # (the V the append left: any right-hand side serves)
                ctx.sync()
                r["trsm"] = timed_call(trsm)
                if i >= a.warmup:
                    for k, v in r.items():
                        t[k].append(v)
            ctx.set_knob("GPR_APPEND_SWEEP", out["auto_knob"])
            res = {k: stats(t[k]) for k in keys}
            tri_bytes = 4.0 * n0 * (n0 + 1)
            floor_ms = tri_bytes / HBM_BYTES_PER_S * 1e3
            res["n0"] = n0
            res["alpha_err_vs_full_fit"] = err
            res["upper_triangle_bytes"] = tri_bytes
            res["one_pass_floor_ms"] = floor_ms
            res["solve_sweep_fraction_of_floor"] = floor_ms / res["solve_sweep"]["median_ms"]
            res["solve_sweep_GBps"] = tri_bytes / (res["solve_sweep"]["median_ms"] * 1e-3) / 1e9
            res["ratio_fit_over_append_sweep"] = out["fit"]["median_ms"] / res["append_sweep"]["median_ms"]
            res["ratio_fit_over_append_trsm"] = out["fit"]["median_ms"] / res["append_trsm"]["median_ms"]
            res["ratio_trsm_over_solve_sweep"] = res["trsm"]["median_ms"] / res["solve_sweep"]["median_ms"]
            res["ratio_solve_trsm_over_solve_sweep"] = (res["solve_trsm"]["median_ms"] /
                                                        res["solve_sweep"]["median_ms"])
            out[f"m={m}"] = res
            del alpha0, alpha1, scratch, B
        ctx.sync()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
