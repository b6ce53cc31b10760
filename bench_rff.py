"""Pathwise posterior sampling: gpr_rff_matmul and sample_paths on one MI355X.

  python bench_rff.py [--steps K --warmup W]

One JSON line.  In one process, measurements alternating in one loop (drift hits all alike; median
of --steps after --warmup, min and max beside every median; HIP events around each call):
  rff         Out = Phi(X) W at n = 2^20, d = 8, SE+SE+WN, nfreq = 4096 for ns = 1, 16 and 64
              (n nfreq nse = 8.6e9 sincos pairs), against
  kmm         gpr_kernel_matmul with as many profile evaluations: the C3 shape's nb = 32768 and
              na = n nfreq / nb output points, the same numbers of columns.
The rates are derived from the timing alone: sincos pairs (exponentials) per second and the second
MFMA's flop/s (4 n nfreq nse ns: a cos and a sin row per frequency).
  paths       on a C3 fit (n = 32768, d = 8, SE+SE+WN), wall clock with a synchronisation, --reps
              runs each: sample_paths (n_samples 16, n_features 1024) by the factor and by the CG
              solve, its evaluation at m = 8192 and m = 2^20, and sample_posterior at m = 8192 (the
              only size of the two it can run: its covariance at 2^20 points is 8.8 TB).
Synthetic data as bench.py: x ~ U[0,1)^(d x n) seed 0, y = sin(sum x)^2, test points seed 1; hp
sigma = 1, sigma_n = 0.1, l = 3 sqrt(8/d).
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


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--nfreq", type=int, default=4096)
    ap.add_argument("--fit-n", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cg-maxit", type=int, default=1000)
    return ap.parse_args()


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "runs": len(ms)}


def main():
    a = parse()
    import gpr_amd as G
    from gpr_amd import _lib

    lib = _lib.lib
    ctx = G.default_context()
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dpp = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731

    def timed_call(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.stream)
        f()
        e1.record(ctx.stream)
        ctx.sync()
        return e0.elapsed_time(e1)

    n, d, F, nb = a.n, a.d, a.nfreq, 32768
    nse, nvs = 2, [1, 16, 64]
    na = n * F // nb
    cov = G.SquaredExp() + G.SquaredExp() + G.WhiteNoise()
    hp = np.array(([1.0] + [3.0 * math.sqrt(8.0 / d)] * d) * 2 + [0.1])
    karr, nk = (ctypes.c_int * 3)(1, 1, 2), 3
    out = {"metric": "random-feature products and pathwise posterior sampling on one MI355X",
           "n": n, "d": d, "nfreq": F, "kmm_na": na, "kmm_nb": nb, "steps": a.steps,
           "warmup": a.warmup, "dtype": "f64"}
    with torch.cuda.stream(ctx.stream):
        dx = ctx.colmajor(np.random.default_rng(0).random((d, n)))
        om = ctx.empty(nse * F * d)
        ctx.check(lib.gpr_rff_draw(ctx.h, karr, nk, d, F, 1, P(om)), "gpr_rff_draw")
        W = ctx.colmajor(np.random.default_rng(2).standard_normal((2 * nse * F, 64)))
        V = ctx.colmajor(np.random.default_rng(3).standard_normal((nb, 64)))
        O = ctx.empty(64, n)

        def rff(ns):
            ctx.check(lib.gpr_rff_matmul(ctx.h, karr, nk, dpp(hp), d, P(dx), n, P(om), F, P(W), ns,
                                         2 * nse * F, P(O), n), "gpr_rff_matmul")

        def kmm(nv):  # the first na points against the first nb
            ctx.check(lib.gpr_kernel_matmul(ctx.h, karr, nk, dpp(hp), d, P(dx), na, P(dx), nb, 0,
                                            1e-8, P(V), nv, nb, P(O), na), "gpr_kernel_matmul")

        t = {f"{k}_ns{ns}": [] for k in ("rff", "kmm") for ns in nvs}
        for i in range(a.warmup + a.steps):
            for ns in nvs:
                r = {f"rff_ns{ns}": timed_call(lambda: rff(ns)),
                     f"kmm_ns{ns}": timed_call(lambda: kmm(ns))}
                if i >= a.warmup:
                    for k, v in r.items():
                        t[k].append(v)
        for k, v in t.items():
            out[k] = stats(v)
        for ns in nvs:
            ms, ref = out[f"rff_ns{ns}"]["median_ms"], out[f"kmm_ns{ns}"]["median_ms"]
            out[f"rff_ns{ns}"].update(
                sincos_pairs_per_s=float(n) * F * nse / (ms * 1e-3),
                product_mfma_flops=4.0 * n * F * nse * ns / (ms * 1e-3), ratio_over_kmm=ms / ref)
            out[f"kmm_ns{ns}"]["exponentials_per_s"] = float(na) * nb * nse / (ref * 1e-3)
        del dx, O, W, V, om
        torch.cuda.empty_cache()

    # a draw as a function against a draw at fixed points, on a C3 fit
    nf, ns = a.fit_n, 16
    x = np.random.default_rng(0).random((d, nf))
    y = np.sin(x.sum(0)) ** 2
    md = G.GPRModel(cov, hp, x, y)
    xp = {m: np.random.default_rng(1).random((d, m)) for m in (8192, 1 << 20)}
    dxp = {m: ctx.colmajor(v) for m, v in xp.items()}
    dout = {m: ctx.empty(ns, m) for m in xp}

    def wall(f):
        ctx.sync()
        t0 = time.perf_counter()
        r = f()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, r

    res = {"n": nf, "n_samples": ns, "n_features": 1024, "reps": a.reps}
    tt = {k: [] for k in ("sample_paths_factor", "eval_8192", "eval_1048576", "sample_posterior_8192")}
    for _ in range(a.reps + 1):  # (the first run grows the workspaces: dropped)
        ms, paths = wall(lambda: G.sample_paths(md, n_samples=ns, solver="factor"))
        tt["sample_paths_factor"].append(ms)
        for m in xp:
            tt[f"eval_{m}"].append(wall(lambda: paths.evaluate_(dxp[m], dout[m]))[0])
        tt["sample_posterior_8192"].append(wall(lambda: G.sample_posterior(md, xp[8192], n_samples=ns))[0])
    for k, v in tt.items():
        res[k] = stats(v[1:])
    ms, pcg = wall(lambda: G.sample_paths(md, n_samples=ns, solver="cg", tol=1e-6, maxit=a.cg_maxit))
    res["sample_paths_cg"] = {"ms": ms, "runs": 1, "tol": 1e-6, "maxit": a.cg_maxit,
                              "iters": pcg.iters, "relres_max": float(pcg.relres.max())}
    res["paths_8192_over_sample_posterior"] = (
        (res["sample_paths_factor"]["median_ms"] + res["eval_8192"]["median_ms"])
        / res["sample_posterior_8192"]["median_ms"])
    out["paths"] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
