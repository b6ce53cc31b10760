"""Matrix-free kernel products: gpr_kernel_matmul, the matrix-free posterior mean and gpr_solve_cg
on one MI355X.

  python bench_kmatmul.py [--steps K --warmup W]

One JSON line.  In one process, measurements alternating in one loop (drift hits all alike; median
of --steps after --warmup, min and max beside every median; HIP events around each call):
  product     Out = K(xa, xb) V at the C3 shape (na = 8192, nb = 32768, d = 8, SE+SE+WN) for nv = 1,
              16 and 64, against
  cross       gpr_kernel(..., GPR_CROSS) of the same shape -- the floor: the same profile
              evaluations with the stores removed and one MFMA stream added -- and
  dense       gpr_kernel plus the GEMM K V (torch.matmul on the context's stream);
  mean        gpr_predict(GPR_PREDICT_MEAN) at m = 8192 by both routes (GPR_MEAN_FREE 0 / 1);
  mean_1m     one matrix-free mean at m = 1 048 576 for SE+M52+WN, with the peak device memory of
              the call (a shape the dense route cannot run: K(x, xp) alone is 275 GB);
  cg          one gpr_solve_cg at n = 65 536, sigma_n = 0.3, tol 1e-6, at most --cg-maxit
              iterations: iterations, ms per iteration, final true relres.
The product's FP64 rates are derived from the timing alone: profile evaluations per second, and
the second MFMA's 2 na nb nv flop/s.
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

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "gaussianprocessregression.jl_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

KIND = {"SE": 1, "WN": 2, "M52": 4}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--np", type=int, default=8192, dest="npred")
    ap.add_argument("--big-np", type=int, default=1 << 20)
    ap.add_argument("--cg-n", type=int, default=65536)
    ap.add_argument("--cg-maxit", type=int, default=300)
    return ap.parse_args()


def description(name, d, noise=0.1):
    kinds = [KIND[k] for k in name.split("+")]
    hp = []
    for k in kinds:
        hp += [noise] if k == KIND["WN"] else [1.0] + [3.0 * math.sqrt(8.0 / d)] * d
    return (ctypes.c_int * len(kinds))(*kinds), len(kinds), np.array(hp, dtype=np.float64)


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

    n, d, m = a.n, a.d, a.npred
    out = {"metric": "matrix-free kernel products on one MI355X", "n": n, "d": d, "np": m,
           "steps": a.steps, "warmup": a.warmup, "dtype": "f64"}
    with torch.cuda.stream(ctx.stream):
        x = np.random.default_rng(0).random((d, n))
        y = np.sin(x.sum(0)) ** 2
        xp = np.random.default_rng(1).random((d, m))
        dx, dy, dxp = ctx.colmajor(x), ctx.colmajor(y), ctx.colmajor(xp)
        karr, nk, hp = description("SE+SE+WN", d)
        nvs = [1, 16, 64]
        V = ctx.colmajor(np.random.default_rng(2).standard_normal((n, 64)))  # (64, n)
        O = ctx.empty(64, m)
        Kx = ctx.empty(n, m)  # K(xp, x): m x n column-major
        U, alpha, mu = ctx.empty(n, n), ctx.empty(n), ctx.empty(m)
        info = ctypes.c_int(0)
        ctx.check(lib.gpr_fit(ctx.h, karr, nk, dpp(hp), d, P(dx), n, P(dy), 1, n, 1e-8, P(U), n,
                              P(alpha), ctypes.byref(info)), "gpr_fit")

        def cross():
            ctx.check(lib.gpr_kernel(ctx.h, karr, nk, dpp(hp), d, P(dxp), m, P(dx), n, 0, 1e-8,
                                     P(Kx), m), "gpr_kernel")

        def product(nv):
            ctx.check(lib.gpr_kernel_matmul(ctx.h, karr, nk, dpp(hp), d, P(dxp), m, P(dx), n, 0,
                                            1e-8, P(V), nv, n, P(O), m), "gpr_kernel_matmul")

        def dense(nv):
            cross()
            torch.matmul(V[:nv], Kx, out=O[:nv])  # (nv, n) (n, m): Out^T = V^T K^T

        def mean(route):
            ctx.set_knob("GPR_MEAN_FREE", route)
            ctx.check(lib.gpr_predict(ctx.h, karr, nk, dpp(hp), d, P(dx), n, P(U), n, P(alpha), 1,
                                      P(dxp), m, 0, 1e-8, P(mu), None, m,
                                      None if route else P(Kx)), "gpr_predict")

        t = {"cross": [], "mean_dense": [], "mean_free": []}
        for nv in nvs:
            t[f"product_nv{nv}"], t[f"dense_nv{nv}"] = [], []
        for i in range(a.warmup + a.steps):
            r = {"cross": timed_call(cross), "mean_dense": timed_call(lambda: mean(0)),
                 "mean_free": timed_call(lambda: mean(1))}
            for nv in nvs:
                r[f"product_nv{nv}"] = timed_call(lambda: product(nv))
                r[f"dense_nv{nv}"] = timed_call(lambda: dense(nv))
            if i >= a.warmup:
                for k, v in r.items():
                    t[k].append(v)
        ctx.set_knob("GPR_MEAN_FREE", -1)
        for k, v in t.items():
            out[k] = stats(v)
        ref = out["cross"]["median_ms"]
        for nv in nvs:
            ms = out[f"product_nv{nv}"]["median_ms"]
            out[f"product_nv{nv}"].update(
                ratio_over_cross=ms / ref, ratio_over_dense=ms / out[f"dense_nv{nv}"]["median_ms"],
                profile_evals_per_s=2.0 * n * m / (ms * 1e-3),
                product_mfma_flops=2.0 * n * m * nv / (ms * 1e-3))
        out["mean_free_over_dense"] = out["mean_free"]["median_ms"] / out["mean_dense"]["median_ms"]
        del Kx, O, V
        torch.cuda.empty_cache()

        # a million scattered test points with a Matern part
        M = a.big_np
        k2, nk2, hp2 = description("SE+M52+WN", d)
        ctx.check(lib.gpr_fit(ctx.h, k2, nk2, dpp(hp2), d, P(dx), n, P(dy), 1, n, 1e-8, P(U), n,
                              P(alpha), ctypes.byref(info)), "gpr_fit")
        dxb = ctx.colmajor(np.random.default_rng(3).random((d, M)))
        mub = ctx.empty(M)
        ctx.sync()
        free0, total = torch.cuda.mem_get_info()

        def big():
            ctx.check(lib.gpr_predict(ctx.h, k2, nk2, dpp(hp2), d, P(dx), n, P(U), n, P(alpha), 1,
                                      P(dxb), M, 0, 1e-8, P(mub), None, M, None), "gpr_predict")

        big()  # (grows the workspaces)
        ms = timed_call(big)
        free1, _ = torch.cuda.mem_get_info()
        out["mean_1m"] = {"description": "SE+M52+WN", "np": M, "ms": ms, "runs": 1,
                          "finite": bool(torch.isfinite(mub).all()),
                          "workspace_bytes_grown": free0 - free1,
                          "device_bytes_in_use": total - free1,
                          "dense_scratch_bytes_avoided": 8.0 * n * M}
        del dxb, mub, U
        torch.cuda.empty_cache()

        # conjugate gradients beyond the comfortable factor size
        nc = a.cg_n
        xc = np.random.default_rng(0).random((d, nc))
        dxc = ctx.colmajor(xc)
        dyc = ctx.colmajor(np.sin(xc.sum(0)) ** 2)
        kc, nkc, hpc = description("SE+WN", d, noise=0.3)
        X = ctx.empty(nc)
        iters, relres = ctypes.c_int(0), (ctypes.c_double * 1)()

        def cg(maxit):
            ctx.check(lib.gpr_solve_cg(ctx.h, kc, nkc, dpp(hpc), d, P(dxc), nc, P(dyc), 1, nc, 1e-8,
                                       1e-6, maxit, P(X), nc, ctypes.byref(iters), relres),
                      "gpr_solve_cg")

        cg(2)
        ms = timed_call(lambda: cg(a.cg_maxit))
        # (the call ends with one more product for the true residual)
        out["cg"] = {"n": nc, "sigma_n": 0.3, "tol": 1e-6, "maxit": a.cg_maxit,
                     "iters": iters.value, "relres": relres[0], "ms": ms,
                     "ms_per_product": ms / (iters.value + 1), "runs": 1}
        ctx.sync()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
