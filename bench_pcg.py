"""The pivoted-Cholesky preconditioner of the matrix-free CG solve (gpr_solve_pcg) on one MI355X.

  solve     SE+WN, d = 8, n = 65 536, tol 1e-6, 1 and 16 right-hand sides: sigma_n in {0.3, 0.03,
            0.01} x rank in {0, 32, 64, 128, 256}.  Per setting: iterations, total ms (median of 3,
            the settings alternating in one process after a warm-up), the factor's build ms
            (gpr_pchol alone), and the preconditioner's ms per iteration, derived as
            (total - build) / iters minus rank 0's ms per iteration at the same sigma_n.  A rank-0
            run that reaches --maxit is reported as capped: its ms per iteration still stands, its
            total is a lower bound.
  floors    one product's ms (rank 0's ms per iteration), and the byte floors at 8 TB/s: the build
            reads n k^2 / 2 doubles, an application 2 x 8 n k bytes.
  counts    device iterations against the NumPy restatement (tests/pchol_ref.py) on a dense K at
            --small-n points, same description.
  grad      gpr_mll_grad_free at n = 16 384, d = 16, sigma_n = 0.03, rank 0 and 128, against the
            dense gpr_fit_kinv + gpr_mll_grad.
Synthetic data as bench.py: x ~ U[0,1)^(d x n) seed 0, y = sin(sum x)^2; sigma = 1, l = --ell sqrt(8
/ d).  One JSON line; --out also writes it to a file.
"""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "gaussianprocessregression.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--ell", type=float, default=3.0)
    ap.add_argument("--maxit", type=int, default=250)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small-n", type=int, default=2048)
    ap.add_argument("--grad-n", type=int, default=16384)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def main():
    a = parse()
    import gpr_amd as G
    from gpr_amd import _lib

    lib, ctx = _lib.lib, G.Context(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    dpp = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    karr = (ctypes.c_int * 2)(1, 2)
    sigmas, ranks = [0.3, 0.03, 0.01], [0, 32, 64, 128, 256]

    def hp_of(d, sn):
        return np.array([1.0] + [a.ell * math.sqrt(8.0 / d)] * d + [sn])

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.stream)
        f()
        e1.record(ctx.stream)
        ctx.sync()
        return e0.elapsed_time(e1)

    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    out = {"metric": "pivoted-Cholesky preconditioned CG on one MI355X", "n": a.n, "d": a.d,
           "ell": a.ell, "tol": 1e-6, "maxit": a.maxit, "runs": a.runs, "solve": [], "counts": []}
    with torch.cuda.stream(ctx.stream):
        n, d = a.n, a.d
        x = np.random.default_rng(0).random((d, n))
        dx = ctx.colmajor(x)
        cols = [np.sin(x.sum(0)) ** 2] + [np.random.default_rng(c).standard_normal(n) for c in range(1, 16)]
        dB, X, Lbuf = ctx.colmajor(np.column_stack(cols)), ctx.empty(16, n), ctx.empty(256, n)
        iters, reached, relres = ctypes.c_int(0), ctypes.c_int(0), (ctypes.c_double * 16)()
        piv = (ctypes.c_int * 256)()

        def solve(hp, nrhs, rank, nn=n, dxx=dx, dBB=dB, maxit=a.maxit):
            ctx.check(lib.gpr_solve_pcg(ctx.h, karr, 2, dpp(hp), d, P(dxx), nn, P(dBB), nrhs, nn, 1e-8,
                                        1e-6, maxit, rank, 0.0, P(X), nn, ctypes.byref(iters), relres,
                                        ctypes.byref(reached)), "gpr_solve_pcg")

        solve(hp_of(d, 0.3), 16, 256, maxit=2)  # warm-up: every workspace at its largest
        for nrhs in (1, 16):
            for sn in sigmas:
                hp = hp_of(d, sn)
                ms = {r: [] for r in ranks}
                it, rr, build = {}, {}, {0: 0.0}
                for _ in range(a.runs):
                    for r in ranks:  # alternating
                        ms[r].append(timed(lambda: solve(hp, nrhs, r)))
                        it[r], rr[r] = iters.value, max(relres[:nrhs])
                for r in ranks[1:]:
                    build[r] = med([timed(lambda: ctx.check(lib.gpr_pchol(
                        ctx.h, karr, 2, dpp(hp), d, P(dx), n, 1e-8, r, 0.0, P(Lbuf), n, piv,
                        ctypes.byref(reached)), "gpr_pchol")) for _ in range(a.runs)])
                per0 = med(ms[0]) / (it[0] + 1)  # (+ the true residual's product)
                for r in ranks:
                    per = (med(ms[r]) - build[r]) / (it[r] + 1)
                    out["solve"].append({
                        "nrhs": nrhs, "sigma_n": sn, "rank": r, "iters": it[r], "capped": it[r] >= a.maxit,
                        "relres": rr[r], "ms": med(ms[r]), "build_ms": build[r], "ms_per_iter": per,
                        "apply_ms_per_iter": per - per0 if r else 0.0, "product_ms": per0,
                        "build_floor_ms": 8.0 * n * r * r / 2 / 8e12 * 1e3,
                        "apply_floor_ms": 2 * 8.0 * n * r / 8e12 * 1e3})
        # device counts against the NumPy restatement on a dense K
        import pchol_ref as PC
        ns = a.small_n
        xs, hp = x[:, :ns].copy(), hp_of(d, 0.03)
        l = hp[1:d + 1]
        D = sum((l[k] * (xs[k][:, None] - xs[k][None, :])) ** 2 for k in range(d))
        Kc = np.exp(-D)
        delta = 0.03 ** 2 + 1e-8
        dxs, dBs = ctx.colmajor(xs), ctx.colmajor(cols[0][:ns].copy())
        for r in (0, 64, 256):
            solve(hp, 1, r, nn=ns, dxx=dxs, dBB=dBs, maxit=ns)
            Lr = PC.pchol(Kc, r)[0] if r else np.zeros((ns, 0))
            ref = PC.pcg(Kc + delta * np.eye(ns), cols[0][:ns], Lr, delta, 1e-6, ns)[1]
            out["counts"].append({"n": ns, "sigma_n": 0.03, "rank": r, "iters": iters.value, "numpy": ref})
        # the matrix-free gradient
        del X, Lbuf, dB
        ng, dg = a.grad_n, 16
        xg = np.random.default_rng(0).random((dg, ng))
        hpg = hp_of(dg, 0.03)
        md = G.GPRModel(G.SquaredExp() + G.WhiteNoise(), hpg, xg, np.sin(xg.sum(0)) ** 2, ctx=ctx)
        K, Kinv, alpha = ctx.empty(ng, ng), ctx.empty(ng, ng), ctx.empty(ng)
        info, gd = ctypes.c_int(0), np.zeros(len(hpg))

        def dense():
            ctx.check(lib.gpr_fit_kinv(ctx.h, karr, 2, dpp(hpg), dg, P(md.dx()), ng, P(md.dsample()), 1,
                                       ng, 1e-8, P(K), ng, P(alpha), P(Kinv), ng, ctypes.byref(info)), "fit")
            ctx.check(lib.gpr_mll_grad(ctx.h, karr, 2, dpp(hpg), dg, P(md.dx()), ng, P(Kinv), ng,
                                       P(alpha), 1e-8, 1, dpp(gd)), "grad")

        res = {}
        f = {"dense": dense,
             "free_rank0": lambda: res.__setitem__(0, G.mll_grad_free(md, maxit=2000)[1]),
             "free_rank128": lambda: res.__setitem__(128, G.mll_grad_free(md, maxit=2000, precond_rank=128)[1])}
        for k in f:
            f[k]()
        ms = {k: [] for k in f}
        for _ in range(a.runs):
            for k in f:
                ms[k].append(timed(f[k]))
        out["grad"] = {"n": ng, "d": dg, "sigma_n": 0.03, "probes": 15, "tol": 1e-6,
                       "dense_ms": med(ms["dense"]), "free_rank0_ms": med(ms["free_rank0"]),
                       "free_rank0_iters": res[0], "free_rank128_ms": med(ms["free_rank128"]),
                       "free_rank128_iters": res[128]}
        ctx.sync()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
