"""The symmetric matrix-free product (GPR_KMM_SYM = 1) against the full evaluation (0) on one
MI355X: K(x, x) V under GPR_SELF, one CG solve and one free MLL gradient by both routes.

  python bench_kmm_sym.py [--steps K --warmup W]

One JSON line.  One process, the two routes alternating in one loop (drift hits both alike; median
of --steps after --warmup with min and max beside it; HIP events around each call):
  product   n = 32 768 and 65 536, d = 8, SE+WN and SE+SE+WN, nv = 1 and 16; with each shape the
            bytes of partial products the symmetric route writes and reads again (from the launch
            geometry: every band's Out[J] partial below its first row, plus the Out[I] partials);
  cg        one gpr_solve_cg at n = 65 536, sigma_n = 0.3, tol 1e-6 per route: iterations, total
            time, time per product (the call ends with one more product for the true residual);
  grad      gpr_mll_grad_free at n = 16 384, d = 16, 15 probes, tol 1e-6 per route.
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
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--cg-n", type=int, default=65536)
    ap.add_argument("--cg-maxit", type=int, default=300)
    ap.add_argument("--grad-n", type=int, default=16384)
    ap.add_argument("--grad-d", type=int, default=16)
    return ap.parse_args()


def partial_bytes(n, nv, G, ncu=256, P=64):
    """bytes the symmetric route writes as partials (and reads again) for one pass"""
    nblk = -(-n // 64)
    nband = -(-nblk // G)
    total = 0
    for b0 in range(0, nband, P):
        nb = min(P, nband - b0)
        slabs = max(1, min(-(-2 * ncu // nb), nblk - b0 * G, 64))
        total += sum(n - (b0 + p) * G * 64 for p in range(nb)) * nv + nb * slabs * G * 64 * nv
    return 8 * total


def main():
    a = parse()
    import gpr_amd as G
    from gpr_amd import _lib

    lib = _lib.lib
    ctx = G.Context(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    dpp = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731

    def timed_call(f, sym):
        ctx.set_knob("GPR_KMM_SYM", sym)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.stream)
        f()
        e1.record(ctx.stream)
        ctx.sync()
        ctx.set_knob("GPR_KMM_SYM", 0)
        return e0.elapsed_time(e1)

    d = a.d
    out = {"metric": "symmetric vs full matrix-free K(x, x) V on one MI355X", "d": d,
           "steps": a.steps, "warmup": a.warmup, "dtype": "f64", "product": [], }
    with torch.cuda.stream(ctx.stream):
        for n in a.ns:
            dx = ctx.colmajor(np.random.default_rng(0).random((d, n)))
            V = ctx.colmajor(np.random.default_rng(2).standard_normal((n, 16)))
            O = ctx.empty(16, n)
            cases = [(name, nv) for name in ("SE+WN", "SE+SE+WN") for nv in (1, 16)]
            t = {(c, s): [] for c in cases for s in (0, 1)}
            for i in range(a.warmup + a.steps):
                for name, nv in cases:
                    karr, nk, hp = description(name, d)
                    for s in (0, 1):
                        ms = timed_call(lambda: ctx.check(lib.gpr_kernel_matmul(
                            ctx.h, karr, nk, dpp(hp), d, P(dx), n, None, n, 1, 1e-8, P(V), nv, n,
                            P(O), n), "gpr_kernel_matmul"), s)
                        if i >= a.warmup:
                            t[((name, nv), s)].append(ms)
            for name, nv in cases:
                full, sym = stats(t[((name, nv), 0)]), stats(t[((name, nv), 1)])
                out["product"].append({
                    "n": n, "description": name, "nv": nv, "full": full, "symmetric": sym,
                    "full_over_symmetric": full["median_ms"] / sym["median_ms"],
                    "partial_bytes_each_way": partial_bytes(n, nv, 4)})
            del dx, V, O
            torch.cuda.empty_cache()

        # one CG solve per route
        nc = a.cg_n
        xc = np.random.default_rng(0).random((d, nc))
        dxc, dyc = ctx.colmajor(xc), ctx.colmajor(np.sin(xc.sum(0)) ** 2)
        kc, nkc, hpc = description("SE+WN", d, noise=0.3)
        X = ctx.empty(nc)
        iters, relres = ctypes.c_int(0), (ctypes.c_double * 1)()

        def cg(maxit):
            ctx.check(lib.gpr_solve_cg(ctx.h, kc, nkc, dpp(hpc), d, P(dxc), nc, P(dyc), 1, nc, 1e-8,
                                       1e-6, maxit, P(X), nc, ctypes.byref(iters), relres),
                      "gpr_solve_cg")

        out["cg"] = {"n": nc, "sigma_n": 0.3, "tol": 1e-6, "maxit": a.cg_maxit, "runs": 1}
        for s, key in ((0, "full"), (1, "symmetric")):
            timed_call(lambda: cg(2), s)
            ms = timed_call(lambda: cg(a.cg_maxit), s)
            out["cg"][key] = {"iters": iters.value, "relres": relres[0], "ms": ms,
                              "ms_per_product": ms / (iters.value + 1)}
        del dxc, dyc, X
        torch.cuda.empty_cache()

        # the free gradient per route
        ng, dg, m = a.grad_n, a.grad_d, 15
        xg = np.random.default_rng(0).random((dg, ng))
        dxg, dyg = ctx.colmajor(xg), ctx.colmajor(np.sin(xg.sum(0)) ** 2)
        kg, nkg, hpg = description("SE+WN", dg, noise=0.3)
        g = np.empty(len(hpg))
        rel = (ctypes.c_double * (m + 1))()

        def grad():
            ctx.check(lib.gpr_mll_grad_free(ctx.h, kg, nkg, dpp(hpg), dg, P(dxg), ng, P(dyg), 1e-8,
                                            m, 0, None, 1e-6, ng, 0, dpp(g), ctypes.byref(iters),
                                            rel), "gpr_mll_grad_free")

        t = {0: [], 1: []}
        gs = {}
        for i in range(a.warmup + a.steps):
            for s in (0, 1):
                ms = timed_call(grad, s)
                gs[s] = (g.copy(), iters.value)
                if i >= a.warmup:
                    t[s].append(ms)
        out["grad"] = {"n": ng, "d": dg, "probes": m, "tol": 1e-6, "sigma_n": 0.3,
                       "full": dict(stats(t[0]), iters=gs[0][1]),
                       "symmetric": dict(stats(t[1]), iters=gs[1][1]),
                       "max_rel_difference": float(np.max(np.abs(gs[0][0] - gs[1][0]) /
                                                          np.abs(gs[0][0])))}
        out["grad"]["full_over_symmetric"] = (out["grad"]["full"]["median_ms"] /
                                              out["grad"]["symmetric"]["median_ms"])
        ctx.sync()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
