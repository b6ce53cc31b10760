"""GPU: the matrix-free gradient of the negative log marginal likelihood (gpr_mll_grad_free).

Exact probes.  With Z = sqrt(n) I and m = n, (1/m) Z Z' = I and Hutchinson's estimator is the
trace itself, so the call must reproduce the dense gradient -0.5 sum (alpha alpha' - K^-1) o dK_j up
to its solves and the form's rounding (this also takes r = n + 1 through the whole stack):
    |g_j - ref_j| <= 4 kappa max(relres) sum_ab (|alpha| |alpha|' + |K^-1|)_ab |dK_j,ab|
                     + the form's bound of test_gpu_grad_form.py, whose |M| is that same matrix,
kappa = cond_2(K): CG's normwise error kappa relres in each of [alpha | K^-1 Z], carried through the
form, which is bilinear in them.  The reference is the oracle's mll_grad where the oracle has the
kernel (SE + WN); with a Matern part it is the same formula on kernel_ref_ld's K and dK.

Random probes (the default path) are checked by value: the probes are regenerated with gpr_randn,
handed back in as Z, and the estimate of exactly those probes is formed in long double.
"""
import ctypes

import numpy as np
import pytest

import kernel_ref_ld as R
import test_gpu_grad_form as GF
import test_product_cpu as PR
from kernel_ref_ld import LD, M52, SE, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")
from oracle import gpr_oracle as O  # noqa: E402

D = 8


def _model(desc, n, seed):
    rng = np.random.default_rng(seed)
    hp = rng.uniform(0.3, 2.0, sum(R.width(k, D) for k in R.flat(desc)))
    hp[-1] = rng.uniform(0.3, 1.0)  # sigma_n >= 0.3: cond_2(K) stays in the thousands
    x = rng.random((D, n))
    y = np.sin(np.sum(x, axis=0)) ** 2
    return hp, x, y, G.GPRModel(PR.cov_of(desc), hp, x, y)


@pytest.mark.parametrize("n", [96, 130])
@pytest.mark.parametrize("desc", [[SE, WN], [SE, M52, WN]], ids=["SE+WN", "SE+M52+WN"])
def test_exact_probes_reproduce_the_dense_gradient(desc, n):
    hp, x, y, md = _model(desc, n, n + len(desc))
    g, iters, relres = G.mll_grad_free(md, Z=np.sqrt(n) * np.eye(n), tol=1e-12, maxit=20 * n)
    K = R.kernel_ld(desc, hp, x).astype(np.float64) if M52 in desc else O.kernel(desc, hp, x)
    Kinv = np.linalg.inv(K).astype(LD)
    a = Kinv @ y.astype(LD)
    ref, T, S = GF.form_ref(desc, hp, x, np.outer(a, a) - Kinv,
                            np.outer(np.abs(a), np.abs(a)) + np.abs(Kinv))
    ref = -0.5 * ref if M52 in desc else O.mll_grad(desc, hp, x, y)
    kappa = np.linalg.cond(K, 2)
    bound = 4 * kappa * relres.max() * S + (1e-13 + (n + (n + 1) + 2 * D + 16) * R.U) * T
    err = np.abs(g.astype(LD) - ref)
    print(f"iters {iters}, max relres {relres.max():.3g}, cond {kappa:.1f}, "
          f"max |err| / bound = {float(np.max(err / bound)):.3g}")
    assert relres.shape == (n + 1,)
    assert np.all(err <= bound)


def _device_randn(ctx, seed, count):
    Z = ctx.empty(count)
    L = G._lib.lib
    assert L.gpr_randn(ctx.h, seed, 0, ctypes.c_void_p(Z.data_ptr()), count) == 0, \
        L.gpr_last_error(ctx.h)
    return ctx.host(Z)


@pytest.mark.parametrize("m", [1, 15, 20])
@pytest.mark.parametrize("desc", [[SE, WN], [SE, M52, WN]], ids=["SE+WN", "SE+M52+WN"])
def test_random_probes_by_value(desc, m):
    """The default path: Z = gpr_randn(seed, 0, n m) as a column-major n x m matrix.  The call with
    the seed must equal the call with that Z handed in bit for bit (the same solves, the same
    form), and both the same-Z estimate in long double,
        g_j = -1/2 (alpha' dK_j alpha - (1/m) sum_c (K^-1 z_c)' dK_j z_c) = -1/2 sum M o dK_j,
        M = alpha alpha' - (1/m) U Z',  U = K^-1 Z,
    inside the exact-probe test's bound with |M| = |alpha| |alpha|' + (1/m) |U| |Z|' and r = m + 1
    factor columns.  m = 20 is r = 21, past the 16 columns the form keeps in registers."""
    n, seed = 130, 40 + m
    hp, x, y, md = _model(desc, n, n + len(desc) + m)
    Z = _device_randn(md.ctx, seed, n * m).reshape(m, n).T
    g, iters, relres = G.mll_grad_free(md, probes=m, seed=seed, tol=1e-12, maxit=20 * n)
    gz, iters_z, relres_z = G.mll_grad_free(md, Z=Z, tol=1e-12, maxit=20 * n)
    assert relres.shape == (m + 1,)
    assert np.array_equal(g, gz) and iters == iters_z and np.array_equal(relres, relres_z)
    K = R.kernel_ld(desc, hp, x).astype(np.float64)
    Kinv = np.linalg.inv(K).astype(LD)
    a, U, Zl = Kinv @ y.astype(LD), Kinv @ Z.astype(LD), Z.astype(LD)
    ref, T, S = GF.form_ref(desc, hp, x, np.outer(a, a) - (U @ Zl.T) / LD(m),
                            np.outer(np.abs(a), np.abs(a)) + (np.abs(U) @ np.abs(Zl).T) / LD(m))
    kappa = np.linalg.cond(K, 2)
    bound = 4 * kappa * relres.max() * S + (1e-13 + (n + (m + 1) + 2 * D + 16) * R.U) * T
    err = np.abs(g.astype(LD) - LD(-0.5) * ref)
    print(f"m {m}: iters {iters}, max relres {relres.max():.3g}, cond {kappa:.1f}, "
          f"max |err| / bound = {float(np.max(err / bound)):.3g}")
    assert np.all(err <= bound)


def test_log_scale_is_one_multiplication_by_hp():
    """with exact probes (nothing random): the log_scale gradient is the plain one times hp[i]"""
    n = 96
    hp, x, y, md = _model([SE, M52, WN], n, 7)
    Z = np.sqrt(n) * np.eye(n)
    g = G.mll_grad_free(md, Z=Z, tol=1e-12, maxit=20 * n)[0]
    gl = G.mll_grad_free(md, Z=Z, tol=1e-12, maxit=20 * n, log_scale=True)[0]
    assert np.all(np.isfinite(g)) and np.all(g != 0.0)
    assert np.array_equal(gl, g * hp)


# (what changes, the word the message must carry)
BAD_ARGS = [(dict(dX=None), "dX is"), (dict(dy=None), "dy is"), (dict(grad=None), "grad is"),
            (dict(n=0), "n="), (dict(m=0), "m="), (dict(seed=-1), "seed"),
            (dict(tol=0.0), "tol"), (dict(tol=-1.0), "tol"), (dict(maxit=-1), "maxit")]


@pytest.mark.parametrize("change,word", BAD_ARGS, ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in BAD_ARGS])
def test_argument_errors(change, word):
    """GPR_E_ARG naming the argument, before anything is written"""
    from gpr_amd import core
    hp, x, y, md = _model([SE, WN], 70, 5)
    ctx, L = md.ctx, G._lib.lib
    kinds, nk = core._kinds_arr(md.covar)
    g, relres, iters = np.full(len(hp), -7.5), np.full(4, -7.5), ctypes.c_int(-7)
    dp = ctypes.POINTER(ctypes.c_double)
    a = dict(dX=md.dx(), n=md.n, dy=md.dsample(), m=3, seed=0, tol=1e-6, maxit=10,
             grad=g.ctypes.data_as(dp))
    a.update(change)
    rc = L.gpr_mll_grad_free(ctx.h, kinds, nk, core._hp_arr(hp)[1], md.d, core._ptr(a["dX"]),
                             a["n"], core._ptr(a["dy"]), R.EPS, a["m"], a["seed"], None, a["tol"],
                             a["maxit"], 0, a["grad"], ctypes.byref(iters), relres.ctypes.data_as(dp))
    msg = L.gpr_last_error(ctx.h).decode()
    assert rc == -1, (rc, msg)  # GPR_E_ARG
    assert word in msg, msg
    assert np.all(g == -7.5) and np.all(relres == -7.5) and iters.value == -7


def test_seed_reproduces_and_matters():
    hp, x, y, md = _model([SE, WN], 130, 3)
    a = G.mll_grad_free(md, seed=11)[0]
    b = G.mll_grad_free(md, seed=11)[0]
    c = G.mll_grad_free(md, seed=12)[0]
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    assert not np.array_equal(a, c)
