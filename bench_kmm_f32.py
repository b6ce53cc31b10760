"""The matrix-free product with FP32 kernel evaluation (GPR_KMM_PREC = 1) against the FP64 route
(0) on one MI355X: K(x, x) V under GPR_SELF, the C3-shaped posterior mean, one CG solve and one
free MLL gradient by both settings.

  python bench_kmm_f32.py [--steps K --warmup W]

One JSON line.  One process, the two settings alternating in one loop (drift hits both alike;
median of --steps after --warmup with min and max beside it; HIP events around each call):
  product   n = 32 768 and 65 536, d = 8 and 16, SE+WN and SE+SE+WN, nv = 1, 16, 64;
  mean      K(xp, x) alpha at the C3 shape (np = 8192, n = 32 768, d = 8, SE+SE+WN);
  cg        one gpr_solve_cg at n = 65 536, sigma_n = 0.3, tol 1e-6 per setting: iterations (every
            product of either precision), the refined solve's outer steps and FP64 products, time;
  grad      gpr_mll_grad_free at n = 16 384, d = 16, 15 probes, tol 1e-6 per setting.
Synthetic data as bench.py: x ~ U[0,1)^(d x n) seed 0, y = sin(sum x)^2; hp sigma = 1,
sigma_n = 0.1 (0.3 for cg and grad), l = 3 sqrt(8/d).
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

from bench_kmatmul import description, stats  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ns", type=int, nargs="+", default=[32768, 65536])
    ap.add_argument("--ds", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--np", type=int, default=8192, dest="npred")
    ap.add_argument("--cg-n", type=int, default=65536)
    ap.add_argument("--cg-maxit", type=int, default=400)
    ap.add_argument("--grad-n", type=int, default=16384)
    ap.add_argument("--grad-d", type=int, default=16)
    return ap.parse_args()


def main():
    a = parse()
    import gpr_amd as G
    from gpr_amd import _lib

    lib = _lib.lib
    ctx = G.Context(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    dpp = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731

    def timed_call(f, prec):
        ctx.set_knob("GPR_KMM_PREC", prec)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.stream)
        f()
        e1.record(ctx.stream)
        ctx.sync()
        ctx.set_knob("GPR_KMM_PREC", 0)
        return e0.elapsed_time(e1)

    def alternate(f):
        """(fp64 stats, fp32 stats) of f by the two settings, alternating"""
        t = {0: [], 1: []}
        for i in range(a.warmup + a.steps):
            for s in (0, 1):
                ms = timed_call(f, s)
                if i >= a.warmup:
                    t[s].append(ms)
        return stats(t[0]), stats(t[1])

    out = {"metric": "FP32 vs FP64 kernel evaluation in the matrix-free K V on one MI355X",
           "steps": a.steps, "warmup": a.warmup, "product": []}
    with torch.cuda.stream(ctx.stream):
        for d in a.ds:
            for n in a.ns:
                dx = ctx.colmajor(np.random.default_rng(0).random((d, n)))
                V = ctx.colmajor(np.random.default_rng(2).standard_normal((n, 64)))
                O = ctx.empty(64, n)
                for name in ("SE+WN", "SE+SE+WN"):
                    karr, nk, hp = description(name, d)
                    for nv in (1, 16, 64):
                        f64, f32 = alternate(lambda: ctx.check(lib.gpr_kernel_matmul(
                            ctx.h, karr, nk, dpp(hp), d, P(dx), n, None, n, 1, 1e-8, P(V), nv, n,
                            P(O), n), "gpr_kernel_matmul"))
                        out["product"].append({
                            "n": n, "d": d, "description": name, "nv": nv, "fp64": f64, "fp32": f32,
                            "fp64_over_fp32": f64["median_ms"] / f32["median_ms"]})
                del dx, V, O
                torch.cuda.empty_cache()

        # the C3-shaped mean: K(xp, x) alpha, np x n
        d, n, m = 8, 32768, a.npred
        dx = ctx.colmajor(np.random.default_rng(0).random((d, n)))
        dxp = ctx.colmajor(np.random.default_rng(1).random((d, m)))
        al = ctx.colmajor(np.random.default_rng(2).standard_normal(n))
        mu = ctx.empty(m)
        karr, nk, hp = description("SE+SE+WN", d)
        f64, f32 = alternate(lambda: ctx.check(lib.gpr_kernel_matmul(
            ctx.h, karr, nk, dpp(hp), d, P(dxp), m, P(dx), n, 0, 1e-8, P(al), 1, n, P(mu), m),
            "gpr_kernel_matmul"))
        out["mean"] = {"np": m, "n": n, "d": d, "description": "SE+SE+WN", "fp64": f64, "fp32": f32,
                       "fp64_over_fp32": f64["median_ms"] / f32["median_ms"]}
        del dx, dxp, al, mu
        torch.cuda.empty_cache()

        # one CG solve per setting
        d, nc = 8, a.cg_n
        xc = np.random.default_rng(0).random((d, nc))
        dxc, dyc = ctx.colmajor(xc), ctx.colmajor(np.sin(xc.sum(0)) ** 2)
        kc, nkc, hpc = description("SE+WN", d, noise=0.3)
        X = ctx.empty(nc)
        iters, relres = ctypes.c_int(0), (ctypes.c_double * 1)()

        def cg(maxit):
            ctx.check(lib.gpr_solve_cg(ctx.h, kc, nkc, dpp(hpc), d, P(dxc), nc, P(dyc), 1, nc, 1e-8,
                                       1e-6, maxit, P(X), nc, ctypes.byref(iters), relres),
                      "gpr_solve_cg")

        out["cg"] = {"n": nc, "d": d, "sigma_n": 0.3, "tol": 1e-6, "maxit": a.cg_maxit, "runs": 1}
        for s, key in ((0, "fp64"), (1, "mixed")):
            timed_call(lambda: cg(2), s)
            ms = timed_call(lambda: cg(a.cg_maxit), s)
            out["cg"][key] = {"iters": iters.value, "relres": relres[0], "ms": ms}
            if s:
                out["cg"][key].update(outer_steps=int(ctx.get_knob("GPR_CG_STAT_OUTER")),
                                      fp64_products=int(ctx.get_knob("GPR_CG_STAT_F64")))
        out["cg"]["fp64_over_mixed"] = out["cg"]["fp64"]["ms"] / out["cg"]["mixed"]["ms"]
        del dxc, dyc, X
        torch.cuda.empty_cache()

        # the free gradient per setting
        ng, dg, m = a.grad_n, a.grad_d, 15
        xg = np.random.default_rng(0).random((dg, ng))
        dxg, dyg = ctx.colmajor(xg), ctx.colmajor(np.sin(xg.sum(0)) ** 2)
        kg, nkg, hpg = description("SE+WN", dg, noise=0.3)
        g = np.empty(len(hpg))
        rel = (ctypes.c_double * (m + 1))()
        gs = {}

        def grad():
            ctx.check(lib.gpr_mll_grad_free(ctx.h, kg, nkg, dpp(hpg), dg, P(dxg), ng, P(dyg), 1e-8,
                                            m, 0, None, 1e-6, ng, 0, dpp(g), ctypes.byref(iters),
                                            rel), "gpr_mll_grad_free")
            gs[int(ctx.get_knob("GPR_KMM_PREC"))] = (g.copy(), iters.value)

        f64, f32 = alternate(grad)
        out["grad"] = {"n": ng, "d": dg, "probes": m, "tol": 1e-6, "sigma_n": 0.3,
                       "fp64": dict(f64, iters=gs[0][1]), "mixed": dict(f32, iters=gs[1][1]),
                       "fp64_over_mixed": f64["median_ms"] / f32["median_ms"],
                       "max_rel_difference": float(np.max(np.abs(gs[0][0] - gs[1][0]) /
                                                          np.abs(gs[0][0])))}
        ctx.sync()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
