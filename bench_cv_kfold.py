"""k-fold / leave-one-out benchmark: gpr_cv_kfold (every complementary fold from ONE factorisation
of all points) against gpr_cv_batch (one factorisation per fold) on the same folds, on one MI355X.

  python bench_cv_kfold.py [--steps K --warmup W --out FILE]

One JSON line, also written to --out (default profiles/r19_bench_cv_kfold.json).  Kernel SE+WN,
d = 8, cost Mahalanobis; folds from kfoldcv(n, k, rng = default_rng(5)); shapes n = 8192 with
k in {1, 8, 64, 128, 819} and n = 16384 with k = 64.  Per shape (median of --steps after --warmup,
min and max beside every median; the calls synchronise themselves, host clock around them):
  kfold_gram     gpr_cv_kfold with GPR_CV_KFOLD_GRAM = 1 (fold Grams of Z = U^-T), and from the
                 library's timing classes in a run of their own:
    gram           class 13: the fold-Gram kernel (k <= 128), or panel copy + SYRK per fold
    solve          class 14: the per-fold factor / solve / loss kernel (k <= 128)
    fit_z          kfold_gram - gram - solve: K, the factorisation with Z, alpha, up/downloads
                   (k > 128: the per-fold factorisations and solves are in here too)
    gram_floor     the bytes of Z below the folds' first rows (rounded down to the kernel's 32
                   rows), sum_f k (n - first_f) 8, at 8 TB/s; gram / gram_floor beside it
  kfold_kinv     gpr_cv_kfold with GPR_CV_KFOLD_GRAM = 0 (P_FF gathered from the full K^-1)
  cv_batch       gpr_cv_batch on the same folds with trn = the complements (an odd number of runs,
                 --steps / 2 | 1; one run where a run takes more than 4 s).  Where that takes
                 minutes (k = 1 and k = 8: n / k factorisations of n - k points) it is timed on
                 the first 8 folds and multiplied by nfold / 8: "extrapolated_from_folds": 8
  speedup        cv_batch / kfold of the faster route; rel_routes, rel_batch: the largest relative
                 difference of the losses between the two routes and against cv_batch's folds
"crossover" (n = 8192, k = 64): gpr_cv_kfold and gpr_cv_batch on the first m folds, m = 1, 2, 3, 4,
6, 8, and the smallest m from which gpr_cv_kfold is the faster call.
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
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "gaussianprocessregression.jl_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
ROWS = 32  # the fold-Gram kernel's row granularity
TC_CV_GRAM, TC_CV_SOLVE = 13, 14
SHAPES = [(8192, 1), (8192, 8), (8192, 64), (8192, 128), (8192, 819), (16384, 64)]
EXTRAPOLATE_FOLDS = 8


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_bench_cv_kfold.json"))
    return ap.parse_args()


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "runs": len(ms)}


def timed(fn, steps, warmup):
    out = None
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms), out


def main():
    a = parse()
    import gpr_amd as G
    from gpr_amd._lib import lib

    d = a.d
    ctx = G.default_context()
    hp = np.array([1.0] + [3.0 * math.sqrt(8.0 / d)] * d + [0.1])
    cost = G.Mahalanobis()

    def tclass(c):
        ms, ln, fl = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
        ctx.check(lib.gpr_timing_get(ctx.h, c, ctypes.byref(ms), ctypes.byref(ln), ctypes.byref(fl)))
        return ms.value

    res = {"bench": "cv_kfold", "kernel": "SE+WN", "d": d, "cost": "Mahalanobis",
           "steps": a.steps, "warmup": a.warmup,
           "auto_knob": ctx.get_knob("GPR_CV_KFOLD_GRAM"), "shapes": []}
    models = {}

    def model(n):  # (one size at a time: the previous model's device arrays go)
        if n not in models:
            models.clear()
            rng = np.random.default_rng(0)
            x = rng.random((d, n))
            y = np.sin(x.sum(axis=0)) ** 2
            models[n] = (G.GPRModel(G.SquaredExp() + G.WhiteNoise(), hp, x, y), x, y)
        return models[n]

    def kfold(n, tst, route, steps=a.steps, warmup=a.warmup):
        md, x, y = model(n)
        ctx.set_knob("GPR_CV_KFOLD_GRAM", route)
        return timed(lambda: G.cv_kfold(md, cost, x, y, tst), steps, warmup)

    for n, k in SHAPES:
        md, x, y = model(n)
        _, tst = G.kfoldcv(n, k, rng=np.random.default_rng(5))
        nfold = len(tst)
        row = {"n": n, "k": k, "nfold": nfold}
        t1, l1 = kfold(n, tst, 1)
        t0, l0 = kfold(n, tst, 0)
        row["kfold_gram"], row["kfold_kinv"] = t1, t0
        row["rel_routes"] = float(np.max(np.abs(l1 - l0) / np.abs(l0)))
        # the library's own choice (GPR_CV_KFOLD_GRAM = -1: Grams up to k = 128, the gather above)
        ta, _ = kfold(n, tst, res["auto_knob"])
        row["kfold_auto"] = ta
        # the split of the Gram route, from the timing classes (a run of its own)
        ctx.set_knob("GPR_CV_KFOLD_GRAM", 1)
        ctx.check(lib.gpr_timing_enable(ctx.h, 1))
        ctx.check(lib.gpr_timing_reset(ctx.h))
        reps = max(1, a.steps)
        t_on, _ = timed(lambda: G.cv_kfold(md, cost, x, y, tst), reps, 0)
        gram, solve = tclass(TC_CV_GRAM) / reps, tclass(TC_CV_SOLVE) / reps
        ctx.check(lib.gpr_timing_enable(ctx.h, 0))
        first = np.array([int(np.min(f)) // ROWS * ROWS for f in tst])
        floor_ms = float(np.sum(k * (n - first)) * 8.0 / HBM_BYTES_PER_S * 1e3)
        row["split_gram_route"] = {
            "gram_ms": gram, "solve_ms": solve,
            "fit_z_ms": t_on["median_ms"] - gram - solve, "total_timed_ms": t_on["median_ms"],
            "gram_floor_ms": floor_ms, "gram_over_floor": gram / floor_ms if k <= 128 else None,
            "lds_kernels": k <= 128}
        # gpr_cv_batch on the same folds
        trn = G.complement_folds(n, tst)
        per_fold_model = {8192: 12.1, 16384: 48.6}[n]  # DESIGN 6.2, ms per fold
        # an odd number of runs, so that the median is a run and one slow call (the batched path
        # allocates and frees gigabytes of workspace per call) cannot set it
        batch_steps = max(1, a.steps // 2) | 1
        if nfold * per_fold_model > 4000.0 and nfold > EXTRAPOLATE_FOLDS and k < 64:
            m = EXTRAPOLATE_FOLDS
            tb, lb = timed(lambda: G.cv_batch(md, cost, x, y, (trn[:m], tst[:m])), batch_steps, 1)
            scale = nfold / m
            row["cv_batch"] = {kk: (v * scale if kk.endswith("_ms") else v) for kk, v in tb.items()}
            row["cv_batch"]["extrapolated_from_folds"] = m
            row["cv_batch"]["measured_ms_for_those"] = tb["median_ms"]
            row["rel_batch"] = float(np.max(np.abs(l1[:m] - lb) / np.abs(lb)))
        else:
            slow = nfold * per_fold_model > 4000.0
            tb, lb = timed(lambda: G.cv_batch(md, cost, x, y, (trn, tst)),
                           1 if slow else batch_steps, 0 if slow else 1)
            row["cv_batch"] = dict(tb, extrapolated_from_folds=None)
            row["rel_batch"] = float(np.max(np.abs(l1 - lb) / np.abs(lb)))
        best = min(t1["median_ms"], t0["median_ms"])
        row["speedup_vs_cv_batch"] = row["cv_batch"]["median_ms"] / best
        row["gram_route_over_kinv_route"] = t1["median_ms"] / t0["median_ms"]
        res["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        if (n, k) == (8192, 64):
            cross = []
            for m in (1, 2, 3, 4, 6, 8):
                tk, _ = kfold(n, tst[:m], 1, steps=3, warmup=1)
                tb, _ = timed(lambda: G.cv_batch(md, cost, x, y, (trn[:m], tst[:m])), 3, 1)
                cross.append({"folds": m, "kfold_ms": tk["median_ms"], "cv_batch_ms": tb["median_ms"]})
            first_win = None  # the smallest m from which every measured m has kfold ahead
            for c in reversed(cross):
                if c["kfold_ms"] >= c["cv_batch_ms"]:
                    break
                first_win = c["folds"]
            res["crossover"] = {"n": n, "k": k, "points": cross,
                                "kfold_faster_from_folds": first_win}
            print(json.dumps(res["crossover"]), file=sys.stderr, flush=True)
    ctx.set_knob("GPR_CV_KFOLD_GRAM", res["auto_knob"])
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
