"""Remove benchmark: taking r observations out of a fitted model with gpr_fit_remove against the
full refit of the kept points a user had to do before, on one MI355X.

  python bench_remove.py [--steps K --warmup W --out FILE]

One JSON line, also written to --out (default profiles/r17_bench_remove.json).  At the C3
description (SE+SE+WN, d = 8) and a fit of n0 = 32768 points: r = 1 at the oldest point (index 0: the
whole triangle is rewritten), in the middle and at the newest (a copy), and r in {R, 2R, 128} spread
evenly (R = 8, the update's group).  Per case, in one process and one loop (the routes alternate, so
that drift hits both alike; median of --steps after --warmup, min and max beside every median):
  remove_sweep   gpr_fit_remove with GPR_REMOVE_SWEEP = 1 (HIP events around the call), and from the
                 library's timing class 12 inside it:
  update_sweep   the rank-r update of the factor, one persistent launch per group
  remove_chain   gpr_fit_remove with GPR_REMOVE_SWEEP = 0, and
  update_chain   its class 12: one diagonal and one panel launch per 128-row block
  sweeps         gpr_potrs_upper on the result with one column: the two alpha sweeps the call ends with
  rest_*         remove - update - sweeps: the gather (and the index upload)
  fit            gpr_fit on the kept points: what a user does today
Reported beside them: fit / remove, the byte floor at 8 TB/s (the upper triangle from the first
touched row block on, read and written once per group, plus the compacting copy read and written
once), the sweep's hops (column blocks from the first touched one on, summed over the groups) and its
time per hop, and whether the two routes' outputs are equal bit for bit.
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
GROUP, NB = 8, 128


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--fit-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_bench_remove.json"))
    return ap.parse_args()


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "runs": len(ms)}


def floor_and_hops(n0, idx):
    """(bytes, hops): what the update and the copy must move, and the sweep's block hops"""
    n = n0 - len(idx)
    nblk = -(-n // NB)
    tri = lambda m: 8.0 * m * (m + 1) / 2  # noqa: E731
    rowlim = min(nblk, idx[0] // NB) * NB
    copy_elems = n * (n - 1) / 2 + (tri(n) - tri(max(n - rowlim, 0))) / 8.0
    nbytes, hops = 2 * 8.0 * copy_elems, 0
    for s0 in range(0, len(idx), GROUP):
        a0 = (idx[s0] - s0) // NB
        if a0 >= nblk:
            break
        nbytes += 2 * tri(n - a0 * NB)
        hops += nblk - a0
    return nbytes, hops


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
    out = {"metric": "gpr_fit_remove against the full refit of the kept points on one MI355X",
           "description": "SE+SE+WN", "n0": N, "d": d, "steps": a.steps, "warmup": a.warmup,
           "fit_steps": a.fit_steps, "dtype": "f64", "group": GROUP,
           "auto_knob": ctx.get_knob("GPR_REMOVE_SWEEP")}
    spread = lambda r: [int(v) for v in np.linspace(0, N - 1, r + 2)[1:-1]]  # noqa: E731
    cases = [("r=1 oldest", [0]), ("r=1 middle", [N // 2]), ("r=1 newest", [N - 1]),
             (f"r={GROUP} spread", spread(GROUP)), (f"r={2 * GROUP} spread", spread(2 * GROUP)),
             ("r=128 spread", spread(128))]
    with torch.cuda.stream(ctx.stream):
        x = np.random.default_rng(0).random((d, N))
        y = np.sin(x.sum(0)) ** 2
        dx, dy = ctx.colmajor(x), ctx.colmajor(y)
        dK, dKfit = ctx.empty(N, N), ctx.empty(N, N)
        outs = [ctx.empty(N, N), ctx.empty(N, N)]
        alpha0 = ctx.empty(N)
        info = ctypes.c_int(0)

        def fit(buf, xs, ys, n, alpha):
            ctx.check(lib.gpr_fit(ctx.h, karr, nk, dpp(hp), d, P(xs), n, P(ys), 1, n, 1e-8, P(buf), N,
                                  P(alpha), ctypes.byref(info)), "gpr_fit")
            if info.value != 0:
                raise RuntimeError(f"K not positive definite, info={info.value}")

        fit(dK, dx, dy, N, alpha0)
        for name, idx in cases:
            r = len(idx)
            n = N - r
            keep = torch.as_tensor(np.setdiff1d(np.arange(N), idx), device=dx.device)
            dxk = dx.index_select(0, keep).contiguous()
            dyk = dy.index_select(0, keep).contiguous()
            cidx = (ctypes.c_int * r)(*idx)
            alphas = [ctx.empty(n), ctx.empty(n)]
            a_fit, scratch = ctx.empty(n), ctx.empty(n)
            fit_ms = []
            for i in range(1 + a.fit_steps):
                t = timed_call(lambda: fit(dKfit, dxk, dyk, n, a_fit))
                if i >= 1:
                    fit_ms.append(t)
            a_ref = a_fit.cpu().numpy()

            def remove(route):
                ctx.set_knob("GPR_REMOVE_SWEEP", route)
                ctx.check(lib.gpr_fit_remove(ctx.h, P(dK), N, N, cidx, r, P(dyk), 1, n, P(outs[route]),
                                             N, P(alphas[route])), "gpr_fit_remove")

            def sweeps():
                ctx.check(lib.gpr_potrs_upper(ctx.h, P(outs[1]), n, N, P(scratch), 1, n),
                          "gpr_potrs_upper")

            keys = ["remove_sweep", "update_sweep", "remove_chain", "update_chain", "sweeps"]
            t = {k: [] for k in keys}
            err = {}
            for i in range(a.warmup + a.steps):
                res_i = {}
                for route, rname in ((1, "sweep"), (0, "chain")):
                    ctx.sync()
                    lib.gpr_timing_reset(ctx.h)
                    lib.gpr_timing_enable(ctx.h, 1)
                    res_i[f"remove_{rname}"] = timed_call(lambda: remove(route))
                    lib.gpr_timing_enable(ctx.h, 0)
                    res_i[f"update_{rname}"] = timing_class(12)
                    got = alphas[route].cpu().numpy()
                    err[rname] = float(np.abs(got - a_ref).max() / np.abs(a_ref).max())
                scratch.copy_(dyk)
                remove(1)  # (the context's factor cache on outs[1], as the call leaves it)
                ctx.sync()
                res_i["sweeps"] = timed_call(sweeps)
                if i >= a.warmup:
                    for k, v in res_i.items():
                        t[k].append(v)
            ctx.set_knob("GPR_REMOVE_SWEEP", out["auto_knob"])
            res = {k: stats(t[k]) for k in keys}
            res["fit"] = stats(fit_ms)
            med = lambda k: res[k]["median_ms"]  # noqa: E731
            for rname in ("sweep", "chain"):
                res[f"rest_{rname}_ms"] = med(f"remove_{rname}") - med(f"update_{rname}") - med("sweeps")
                res[f"ratio_fit_over_remove_{rname}"] = med("fit") / med(f"remove_{rname}")
            nbytes, hops = floor_and_hops(N, idx)
            res.update({"r": r, "first_index": idx[0], "last_index": idx[-1], "n_kept": n,
                        "alpha_err_vs_fit": err, "floor_bytes": nbytes,
                        "byte_floor_ms": nbytes / HBM_BYTES_PER_S * 1e3, "sweep_hops": hops,
                        "sweep_us_per_hop": med("update_sweep") * 1e3 / hops if hops else None,
                        "routes_bit_equal": bool(torch.equal(outs[0][:n, :n], outs[1][:n, :n]) and
                                                 torch.equal(alphas[0], alphas[1]))})
            res["remove_sweep_fraction_of_floor"] = res["byte_floor_ms"] / med("remove_sweep")
            out[name] = res
            del dxk, dyk, alphas, a_fit, scratch, keep
        ctx.sync()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
