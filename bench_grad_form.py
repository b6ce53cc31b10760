"""The matrix-free gradient form and the matrix-free MLL gradient on one MI355X.

  python bench_grad_form.py [--steps K --warmup W]

One JSON line.  In one process, the measurements of a shape alternating in one loop (drift hits
all alike; median of --steps after --warmup, min and max beside it; HIP events around each call):
  form        gpr_kernel_grad_form at r = 16 (SE+WN, n = 16384, d = 16), against
  product     gpr_kernel_matmul on the same points (GPR_SELF) with nv = 2d, and
  dense_pass  gpr_mll_grad's fused pass over a stored n x n weight;
  free        gpr_mll_grad_free end to end (m = 15 probes, tol 1e-6) with its CG iterations, against
  dense       gpr_fit_kinv + gpr_mll + gpr_mll_grad;
  free_big    form and free alone at every n of --big (no n x n buffer is allocated there);
  spread      the standard deviation over --seeds seeds of each component of free's gradient at the
              first shape, relative to the dense gradient's magnitude (a single run).
Synthetic data as bench.py: x ~ U[0,1)^(d x n) seed 0, y = sin(sum x)^2; hp sigma = 1,
l = 3 sqrt(8/d); sigma_n = 0.3 (CG's iteration count grows as 1 / sigma_n).
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


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--big", type=int, nargs="*", default=[65536, 131072])
    ap.add_argument("--probes", type=int, default=15)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--maxit", type=int, default=400)
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
    d, m, r = a.d, a.probes, 16
    karr = (ctypes.c_int * 2)(1, 2)
    hp = np.array([1.0] + [3.0 * math.sqrt(8.0 / d)] * d + [0.3])
    g, gd = np.zeros(len(hp)), np.zeros(len(hp))
    iters, relres = ctypes.c_int(0), (ctypes.c_double * (1 + m))()

    def timed_call(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.stream)
        f()
        e1.record(ctx.stream)
        ctx.sync()
        return e0.elapsed_time(e1)

    def shape(n, dense):
        x = np.random.default_rng(0).random((d, n))
        dx, dy = ctx.colmajor(x), ctx.colmajor(np.sin(x.sum(0)) ** 2)
        A = ctx.colmajor(np.random.default_rng(2).standard_normal((n, 2 * d)))  # (2d, n)
        O = ctx.empty(2 * d, n)
        f = {
            "form": lambda: ctx.check(lib.gpr_kernel_grad_form(
                ctx.h, karr, 2, dpp(hp), d, P(dx), n, P(A), n, P(A), n, r, 1e-8, 1, dpp(g)), "form"),
            "free": lambda seed=0: ctx.check(lib.gpr_mll_grad_free(
                ctx.h, karr, 2, dpp(hp), d, P(dx), n, P(dy), 1e-8, m, seed, None, 1e-6, a.maxit, 1,
                dpp(g), ctypes.byref(iters), relres), "free"),
        }
        if dense:
            K, Kinv, alpha = ctx.empty(n, n), ctx.empty(n, n), ctx.empty(n)
            mllv, info = ctypes.c_double(0.0), ctypes.c_int(0)
            f["product"] = lambda: ctx.check(lib.gpr_kernel_matmul(
                ctx.h, karr, 2, dpp(hp), d, P(dx), n, None, n, 1, 1e-8, P(A), 2 * d, n, P(O), n), "kmm")
            f["dense_pass"] = lambda: ctx.check(lib.gpr_mll_grad(
                ctx.h, karr, 2, dpp(hp), d, P(dx), n, P(Kinv), n, P(alpha), 1e-8, 1, dpp(gd)), "grad")

            def dense_eval():
                ctx.check(lib.gpr_fit_kinv(ctx.h, karr, 2, dpp(hp), d, P(dx), n, P(dy), 1, n, 1e-8,
                                           P(K), n, P(alpha), P(Kinv), n, ctypes.byref(info)), "fit")
                ctx.check(lib.gpr_mll(ctx.h, P(K), n, n, P(dy), P(alpha), ctypes.byref(mllv)), "mll")
                f["dense_pass"]()

            f["dense"] = dense_eval
            order = ["dense", "dense_pass", "form", "product", "free"]  # (dense first: it fills Kinv)
        else:
            order = ["form", "free"]
        ms = {k: [] for k in order}
        for i in range(a.warmup + a.steps):
            for k in order:
                t = timed_call(f[k])
                if i >= a.warmup:
                    ms[k].append(t)
        res = {k: stats(v) for k, v in ms.items()}
        res["free"].update(cg_iters=iters.value, max_relres=max(relres[:]))
        if dense:
            gs = []
            for s in range(a.seeds):
                f["free"](s)
                gs.append(g.copy())
            res["spread"] = {"seeds": a.seeds, "probes": m, "dense_grad": gd.tolist(),
                             "free_mean": np.mean(gs, 0).tolist(),
                             "free_std_over_abs_dense": (np.std(gs, 0) / np.abs(gd)).tolist()}
        return res

    out = {"metric": "matrix-free gradient form and MLL gradient on one MI355X", "d": d, "r": r,
           "probes": m, "steps": a.steps, "warmup": a.warmup, "dtype": "f64"}
    with torch.cuda.stream(ctx.stream):
        out[f"n{a.n}"] = shape(a.n, True)
        for n in a.big:
            out[f"n{n}"] = shape(n, False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
