"""Matern benchmark: what the FP64 square root and the polynomial of the Matern-3/2 / Matern-5/2
profiles add to the K assembly and to the MLL + gradient evaluation, on one MI355X.

  python bench_matern.py [--steps K --warmup W]

One JSON line with two measurements (HIP events on the context stream, median of --steps after
--warmup, min and max beside every median):
  kbuild    the full symmetric K (gpr_kernel, GPR_SELF) at N = 32768, d = 8 for SE+WN, M52+WN,
            M32+WN and SE+M52+WN, all through the same mirrored-tile Gram kernels
            (GPR_KBUILD_TILES=1 keeps the single SquaredExp part off its column build), as
            8 N^2 bytes / time against the 8 TB/s HBM peak, with the ratios M52/SE and M32/SE;
            run alternately in one loop so that drift hits every description alike
  mll_grad  the C4-shaped evaluation (N = 16384, d = 16: gpr_fit_kinv, gpr_mll, gpr_mll_grad
            with the log-scale chain rule) for SE+WN and M52+WN, ms per evaluation, and the
            gradient pass alone
Synthetic data as bench.py: x ~ U[0,1)^(d x n) seed 0, y = sin(sum x)^2, hp sigma = 1,
l = 3 sqrt(8/d), sigma_n = 0.1.
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
KIND = {"SE": 1, "WN": 2, "M32": 3, "M52": 4}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--mll-n", type=int, default=16384)
    ap.add_argument("--mll-d", type=int, default=16)
    ap.add_argument("--mll-steps", type=int, default=3)
    return ap.parse_args()


def kinds_of(name):
    return [KIND[k] for k in name.split("+")]


def default_hp(kinds, d, noise=0.1):
    hp = []
    for k in kinds:
        hp += [noise] if k == KIND["WN"] else [1.0] + [3.0 * math.sqrt(8.0 / d)] * d
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

    out = {"metric": "Matern-3/2 and Matern-5/2 against SquaredExp on one MI355X "
                     "(K assembly, MLL + gradient)",
           "steps": a.steps, "warmup": a.warmup, "dtype": "f64"}
    with torch.cuda.stream(ctx.stream):
        # ---- 1. the symmetric K build, every description through the mirrored Gram tiles ----
        n, d = a.n, a.d
        x = np.random.default_rng(0).random((d, n))
        dx = ctx.colmajor(x)
        K = ctx.empty(n, n)
        ctx.set_knob("GPR_KBUILD_TILES", 1)
        names = ["SE+WN", "M52+WN", "M32+WN", "SE+M52+WN"]
        calls, t = {}, {nm: [] for nm in names}
        for nm in names:
            kinds = kinds_of(nm)
            hp = default_hp(kinds, d)
            karr = (ctypes.c_int * len(kinds))(*kinds)
            calls[nm] = (lambda karr=karr, nk=len(kinds), hp=hp: ctx.check(
                lib.gpr_kernel(ctx.h, karr, nk, dpp(hp), d, P(dx), n, None, n, 1, 1e-8, P(K), n),
                "gpr_kernel"))
        finite = {}
        for i in range(a.warmup + a.steps):  # alternating, same process
            for nm in names:
                ms = timed_call(calls[nm])
                if i >= a.warmup:
                    t[nm].append(ms)
                if i == 0:
                    finite[nm] = bool(torch.isfinite(K[:64]).all())
        ctx.set_knob("GPR_KBUILD_TILES", 0)
        t_col = stats([timed_call(calls["SE+WN"]) for _ in range(a.warmup + a.steps)][a.warmup:])
        kb = {}
        for nm in names:
            st = stats(t[nm])
            gbs = 8.0 * n * n / (st["median_ms"] * 1e-3) / 1e9
            kb[nm] = {**st, "GBps": gbs, "hbm_frac": gbs / HBM_PEAK_GBS, "finite": finite[nm]}
        se = kb["SE+WN"]["median_ms"]
        out["kbuild"] = {
            "n": n, "d": d, "bytes": 8.0 * n * n, "path": "mirrored 64x64 Gram tiles (GPR_KBUILD_TILES=1)",
            **kb,
            "ratio_M52_over_SE": kb["M52+WN"]["median_ms"] / se,
            "ratio_M32_over_SE": kb["M32+WN"]["median_ms"] / se,
            "ratio_SE+M52_over_SE": kb["SE+M52+WN"]["median_ms"] / se,
            "SE+WN_column_build_default": t_col,
        }
        del K

        # ---- 2. the C4-shaped MLL + gradient evaluation ------------------------------------
        N, d2 = a.mll_n, a.mll_d
        x = np.random.default_rng(0).random((d2, N))
        y = np.sin(x.sum(0)) ** 2
        dx, dy = ctx.colmajor(x), ctx.colmajor(y)
        K, Kinv, alpha = ctx.empty(N, N), ctx.empty(N, N), ctx.empty(N)
        mllv, info = ctypes.c_double(0.0), ctypes.c_int(0)
        mg = {}
        for nm in ("SE+WN", "M52+WN"):
            kinds = kinds_of(nm)
            hp = default_hp(kinds, d2)
            karr = (ctypes.c_int * 2)(*kinds)
            g = np.zeros(len(hp))

            def fit():
                ctx.check(lib.gpr_fit_kinv(ctx.h, karr, 2, dpp(hp), d2, P(dx), N, P(dy), 1, N, 1e-8,
                                           P(K), N, P(alpha), P(Kinv), N, ctypes.byref(info)),
                          "fit_kinv")
                if info.value != 0:
                    raise RuntimeError(f"not PD: info={info.value}")
                ctx.check(lib.gpr_mll(ctx.h, P(K), N, N, P(dy), P(alpha), ctypes.byref(mllv)), "mll")

            def grad():
                ctx.check(lib.gpr_mll_grad(ctx.h, karr, 2, dpp(hp), d2, P(dx), N, P(Kinv), N, P(alpha),
                                           1e-8, 1, dpp(g)), "mll_grad")

            def step():
                fit()
                grad()

            ts = [timed_call(step) for _ in range(a.warmup + a.mll_steps)][a.warmup:]
            tg = [timed_call(grad) for _ in range(a.warmup + a.mll_steps)][a.warmup:]
            mg[nm] = {"evaluation": stats(ts), "grad_pass": stats(tg), "mll": mllv.value,
                      "grad_finite": bool(np.isfinite(g).all())}
        out["mll_grad"] = {
            "n": N, "d": d2, **mg,
            "ratio_M52_over_SE_evaluation":
                mg["M52+WN"]["evaluation"]["median_ms"] / mg["SE+WN"]["evaluation"]["median_ms"],
            "ratio_M52_over_SE_grad_pass":
                mg["M52+WN"]["grad_pass"]["median_ms"] / mg["SE+WN"]["grad_pass"]["median_ms"],
        }
        ctx.sync()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
