"""GPU: gpr_pchol and gpr_solve_pcg against the NumPy restatement of tests/pchol_ref.py (problems a - e;
its pivot gaps are asserted on the CPU by tests/test_pchol_ref_cpu.py).  The factor's bar is 16 x
the largest max|L - L_longdouble| / sqrt(c) of the float64 restatement over the (problem, rank)
cases: the device's other exponential and fused sums are amplified as that is.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import cg_ref as C
import kernel_ref_ld as R
import pchol_ref as PC
import test_gpu_mll_grad_free as MG
import test_product_cpu as PR
from test_gpu_solve_cg_paths import GPR_E_ARG, SENT, _dp, _karr, _P

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

NAMES = sorted(PC.PROBLEMS)


def _bar():
    return 16.0 * max(PC.factor(nm, r)[3] for nm in NAMES for r in PC.RANKS)


def _model(name):
    desc, hp, x = PC.inputs(name)
    return G.GPRModel(PR.cov_of(desc), hp, x, np.zeros(x.shape[1]))


def _pcg(name, B, rank, rtol=0.0, tol=PC.TOL, maxit=5000, pad=(0, 0), x=None):
    """(X, iters, relres, rank reached); ldb = n + pad[0] (padding NaN), ldx = n + pad[1] (sentinel)"""
    desc, hp, x0 = PC.inputs(name)
    x = x0 if x is None else x
    ctx = G.default_context()
    d, n = x.shape
    B = np.asarray(B, dtype=np.float64).reshape(n, -1)
    nrhs = B.shape[1]
    dB = torch.full((nrhs, n + pad[0]), float("nan"), dtype=torch.float64, device=ctx.device)
    dB[:, :n] = torch.from_numpy(np.ascontiguousarray(B.T)).to(ctx.device)
    dX = torch.full((nrhs, n + pad[1]), SENT, dtype=torch.float64, device=ctx.device)
    dx, (ka, nk), hpa = ctx.colmajor(x), _karr(desc), np.array(hp)
    iters, reached, relres = ctypes.c_int(-7), ctypes.c_int(-7), np.full(nrhs, SENT)
    rc = G._lib.lib.gpr_solve_pcg(ctx.h, ka, nk, _dp(hpa), d, _P(dx), n, _P(dB), nrhs, n + pad[0],
                                  R.EPS, tol, maxit, rank, rtol, _P(dX), n + pad[1],
                                  ctypes.byref(iters), _dp(relres), ctypes.byref(reached))
    assert rc == 0, G._lib.lib.gpr_last_error(ctx.h)
    o = dX.cpu().numpy()
    assert np.all(o[:, n:] == SENT) and not np.any(o[:, :n] == SENT)
    return o[:, :n].T.copy(), iters.value, relres, reached.value


@functools.lru_cache(maxsize=None)
def _dense(name):
    """(B of 17 columns, K^-1 B, cond_2(K)), computed once"""
    K = PC.reference(name)[2]
    B = PC.rhs(name, 17)
    return B, np.linalg.solve(K, B), np.linalg.cond(K, 2)


@functools.lru_cache(maxsize=None)
def _ref_counts(name, rank):
    """the NumPy recurrence's iteration per column of the 17"""
    _, _, K, _, delta = PC.reference(name)
    return PC.pcg(K, _dense(name)[0], PC.factor(name, rank)[0], delta, PC.TOL, 5000)[2]


def _assert_solution(X, relres, B, Xs, cond):
    assert np.all(relres <= 10 * PC.TOL), relres
    err = np.linalg.norm(X - Xs, axis=0) / np.linalg.norm(Xs, axis=0)
    print(f"relres {relres.max():.3g}, err {err.max():.3g}, cond {cond:.3g}")
    assert np.all(err <= cond * relres)


@pytest.mark.parametrize("rank", PC.RANKS)
@pytest.mark.parametrize("name", NAMES)
def test_factor(name, rank):
    desc, hp, x = PC.inputs(name)
    Kc, _, _, c, _ = PC.reference(name)
    Lr, pivr, _, _ = PC.factor(name, rank)
    L, piv = G.pivoted_cholesky(PR.cov_of(desc), hp, x, rank)
    assert np.array_equal(piv, pivr)
    bar, err = _bar(), np.max(np.abs(L - Lr)) / math.sqrt(c)
    rows = np.max(np.abs(Kc[piv] - L[piv] @ L.T)) / c
    print(f"BAR {bar:.3g}: max|L - L_ref| / sqrt(c) = {err:.3g}, pivoted rows / c = {rows:.3g}")
    assert err <= bar and rows <= bar
    assert np.all(c - np.sum(L * L, axis=1) >= -bar * c)  # the residual diagonal


def test_full_rank_is_an_exact_solve():
    B, Xs, cond = _dense("a")
    X, iters, relres, reached = _pcg("a", B[:, :1], 130)
    print(f"rank reached {reached}, iters {iters}")
    assert iters <= 3
    _assert_solution(X, relres, B[:, :1], Xs[:, :1], cond)


@pytest.mark.parametrize("nrhs", [1, 3, 17])
@pytest.mark.parametrize("rank", [5, 17, 64])
@pytest.mark.parametrize("name", NAMES)
def test_solve(name, rank, nrhs):
    B, Xs, cond = _dense(name)
    X, iters, relres, reached = _pcg(name, B[:, :nrhs], rank, pad=(3, 5))
    ref = int(_ref_counts(name, rank)[:nrhs].max())
    print(f"iters {iters}, the NumPy recurrence {ref}")
    assert reached == rank
    _assert_solution(X, relres, B[:, :nrhs], Xs[:, :nrhs], cond)
    assert iters <= math.ceil(C.MARGIN * ref)
    if rank == 64 and name in "ab":
        plain = G.solve_cg(_model(name), B[:, :nrhs], tol=PC.TOL, maxit=5000, precond_rank=0)[1]
        assert iters < plain, (iters, plain)


def test_rank_zero_is_the_parent_and_calls_repeat():
    B = _dense("a")[0][:, :3]
    md = _model("a")
    X0, it0, rr0 = G.solve_cg(md, B, tol=PC.TOL)
    X1, it1, rr1 = G.solve_cg(md, B, tol=PC.TOL, precond_rank=0)
    X2, it2, rr2, _ = _pcg("a", B, 0, maxit=md.n)
    assert it0 == it1 == it2 and np.array_equal(X0, X1) and np.array_equal(X0, X2)
    assert np.array_equal(rr0, rr1) and np.array_equal(rr0, rr2)
    a, b = _pcg("b", _dense("b")[0][:, :3], 17), _pcg("b", _dense("b")[0][:, :3], 17)
    assert a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


def test_early_stop_on_duplicated_points():
    desc, hp, x0 = PC.inputs("a")
    x = np.concatenate([x0, x0[:, -10:]], axis=1)  # n = 140
    L, piv = G.pivoted_cholesky(PR.cov_of(desc), hp, x, 140, rtol=1e-12)
    assert len(piv) < 140 and L.shape == (140, len(piv)) and np.all(np.isfinite(L))
    K = R.kernel_ld(desc, hp, x).astype(np.float64)
    B = np.sin(np.sum(x, axis=0)) ** 2
    X, iters, relres, reached = _pcg("a", B, 140, rtol=1e-12, x=x)
    assert reached == len(piv)
    _assert_solution(X, relres, B[:, None], np.linalg.solve(K, B)[:, None], np.linalg.cond(K, 2))


def test_mll_grad_free_takes_the_rank():
    n = 96
    hp, x, y, md = MG._model([R.SE, R.WN], n, n + 2)
    Z = np.sqrt(n) * np.eye(n)
    g0, _, rr0 = G.mll_grad_free(md, Z=Z, tol=1e-12, maxit=20 * n)
    g1, it1, rr1 = G.mll_grad_free(md, Z=Z, tol=1e-12, maxit=20 * n, precond_rank=17)
    assert md.ctx.get_knob("GPR_CG_PRECOND") == 0
    # test_gpu_mll_grad_free's bound for exact probes, once for each of the two calls
    K = R.kernel_ld([R.SE, R.WN], hp, x).astype(np.float64)
    Kinv = np.linalg.inv(K).astype(R.LD)
    a = Kinv @ y.astype(R.LD)
    _, T, S = MG.GF.form_ref([R.SE, R.WN], hp, x, np.outer(a, a) - Kinv,
                             np.outer(np.abs(a), np.abs(a)) + np.abs(Kinv))
    kappa = np.linalg.cond(K, 2)
    bound = sum(4 * kappa * rr.max() * S + (1e-13 + (n + (n + 1) + 2 * MG.D + 16) * R.U) * T
                for rr in (rr0, rr1))
    assert np.all(np.abs(g1.astype(R.LD) - g0.astype(R.LD)) <= bound)


BAD = [(dict(rank=257), "rank"), (dict(rank=131), "rank"), (dict(ldl=129), "ldl"),
       (dict(rtol=-1.0), "rtol")]


@pytest.mark.parametrize("change,word", BAD, ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in BAD])
def test_argument_errors(change, word):
    desc, hp, x = PC.inputs("a")
    ctx = G.default_context()
    d, n = x.shape
    a = dict(rank=5, ldl=n, rtol=0.0)
    a.update(change)
    dL = torch.full((300, n), SENT, dtype=torch.float64, device=ctx.device)
    dx, (ka, nk), hpa = ctx.colmajor(x), _karr(desc), np.array(hp)
    piv, reached = (ctypes.c_int * 300)(*([-7] * 300)), ctypes.c_int(-7)
    rc = G._lib.lib.gpr_pchol(ctx.h, ka, nk, _dp(hpa), d, _P(dx), n, R.EPS, a["rank"], a["rtol"],
                              _P(dL), a["ldl"], piv, ctypes.byref(reached))
    msg = G._lib.lib.gpr_last_error(ctx.h).decode()
    assert rc == GPR_E_ARG and word in msg, (rc, msg)
    ctx.sync()
    assert torch.all(dL == SENT).item() and reached.value == -7 and all(p == -7 for p in piv)
