"""The tile-DAG's accumulation loop (dag.hip dag_accum): a ring of five LDS stages, one barrier
per TWO 16-deep K stages.

The other tile-DAG tests only reach a one-stage ragged tail (n = 144, 400, 1040, ...).  The
two-stage period can go wrong on odd stage counts and at the single-stage half period that ends
them, so these cases give the last tile row every stage count 1..7 behind 1, 2, 3 and 8 full row
blocks, in every instance of the kernel: the plain factorisation, the right-hand sides inside the
launch, the gram tasks (gpr_fit_kinv) and a batched launch (cv_batch).  Tolerances are those of
the tests they extend (test_gpu_parity.py, test_crossval.py); helpers copied from there.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.linalg as sla

from oracle import gpr_oracle as O

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

SE, WN = O.SE, O.WN


def relnorm(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _spd(n, d=4, seed=0, noise=0.3):
    rng = np.random.default_rng(seed)
    x = rng.random((d, n))
    return O.kernel([SE, WN], np.r_[1.0, [1.5] * d, noise], x)


def _dev_potrf(ctx, A):
    dA = ctx.colmajor(A)
    n = A.shape[0]
    info = ctypes.c_int(-7)
    rc = G._lib.lib.gpr_potrf_upper(ctx.h, ctypes.c_void_p(dA.data_ptr()), n, n, ctypes.byref(info))
    assert rc >= 0, G._lib.lib.gpr_last_error(ctx.h)
    return dA, info.value


def _fit_predict_dev(ctx, kinds, hp, x, y, xp, mode):
    d, n = x.shape
    m = xp.shape[1]
    y2 = y if y.ndim == 2 else y[:, None]
    nrhs = y2.shape[1]
    dx, dy, dxp = ctx.colmajor(x), ctx.colmajor(y2), ctx.colmajor(xp)
    K = ctx.empty(n, n)
    alpha = ctx.empty(nrhs, n)
    mu = ctx.empty(nrhs, m)
    var = ctx.empty(m) if mode == G.GPR_PREDICT_DIAG else ctx.empty(m, m)
    karr = (ctypes.c_int * len(kinds))(*[1 if k == SE else 2 for k in kinds])
    hpa = np.asarray(hp, dtype=np.float64)
    info = ctypes.c_int(-1)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = G._lib.lib.gpr_fit_predict(ctx.h, karr, len(kinds),
                                    hpa.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), d, P(dx),
                                    n, P(dy), nrhs, n, 1e-8, P(K), n, P(alpha), P(dxp), m, mode,
                                    P(mu), P(var), m, None, ctypes.byref(info))
    assert rc == 0 and info.value == 0, G._lib.lib.gpr_last_error(ctx.h)
    return ctx.host(K), ctx.host(alpha), ctx.host(mu), ctx.host(var)


# n = 128 f + 16 t: f full row blocks (8 stages each), then a last tile row whose accumulations
# run f * 8 stages and whose W-product runs t stages -- t = 2..7 after one block, 3 after 2 and 3
@pytest.mark.parametrize("n", [160, 176, 192, 208, 224, 240, 304, 432])
def test_potrf_dag_ragged_stage_counts(n, monkeypatch):
    monkeypatch.setenv("GPR_DAG", "1")
    ctx = G.Context(0)
    A = _spd(n, seed=n + 7)
    dA, info = _dev_potrf(ctx, A)
    assert info == 0
    R = ctx.host(dA)
    U = sla.cholesky(A, lower=False)
    assert relnorm(np.triu(R), U) < 1e-12
    assert np.array_equal(np.tril(R, -1), np.tril(A, -1))
    B = np.random.default_rng(4).random((n, 2))
    dB = ctx.colmajor(B)
    assert G._lib.lib.gpr_potrs_upper(ctx.h, ctypes.c_void_p(dA.data_ptr()), n, n,
                                      ctypes.c_void_p(dB.data_ptr()), 2, n) == 0
    assert relnorm(ctx.host(dB), O.cho_solve_upper(U, B)) < 1e-11


_KINDS = [SE, WN]
_DIM = 3


@functools.lru_cache(maxsize=None)
def _problem(n, npred):
    """Inputs and the oracle's results, computed once per shape (callers do not write to them)."""
    x, y, xp = O.synthetic(_DIM, n, npred, seed_train=n, seed_test=npred)
    hp = O.default_hp(_KINDS, _DIM, noise=0.05)
    K = O.kernel(_KINDS, hp, x)
    U = sla.cholesky(K, lower=False)
    alpha = O.cho_solve_upper(U, y)
    mu, var = O.predict(_KINDS, hp, x, y, xp, diagonal_var=True)
    _, S = O.predict(_KINDS, hp, x, y, xp, diagonal_var=False)
    return x, y, xp, hp, K, U, alpha, mu, var, S


# np + 1 right-hand sides: 2, 131 (a last column tile of 3), 78, 141 (13); last tile rows of 3, 7,
# 3 and 3 stages after 1, 1, 2 and 8 full row blocks
@pytest.mark.parametrize("n,npred", [(176, 1), (240, 130), (304, 77), (1072, 140)])
def test_fit_predict_dag_ragged_stage_counts(n, npred, monkeypatch):
    monkeypatch.setenv("GPR_FUSED_RHS", "2")
    monkeypatch.setenv("GPR_DAG", "1")
    x, y, xp, hp, K, U, alpha_o, mu_o, var_o, S_o = _problem(n, npred)
    ctx = G.Context(0)
    Kd, alpha, mu, var = _fit_predict_dev(ctx, _KINDS, hp, x, y, xp, G.GPR_PREDICT_DIAG)
    np.testing.assert_allclose(np.tril(Kd, -1), np.tril(K, -1), rtol=1e-13, atol=1e-15)
    Kdev = np.tril(Kd) + np.tril(Kd, -1).T
    np.fill_diagonal(Kdev, np.diag(K))
    assert relnorm(np.triu(Kd), sla.cholesky(Kdev, lower=False)) < 1e-11
    np.testing.assert_allclose(alpha.ravel(), alpha_o, rtol=1e-8, atol=1e-10 * np.abs(alpha_o).max())
    vtol = 1e-8 * O.diag_prior(_KINDS, hp, _DIM)
    np.testing.assert_allclose(mu.ravel(), mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var, var_o, rtol=1e-8, atol=vtol)
    _, _, mu2, S = _fit_predict_dev(ctx, _KINDS, hp, x, y, xp, G.GPR_PREDICT_FULL)
    np.testing.assert_allclose(mu2.ravel(), mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(S, S_o, rtol=1e-8, atol=vtol)


def test_fit_predict_dag_deterministic(monkeypatch):
    """Two launches on the same inputs: the order in which workgroups claim tasks differs, the
    arithmetic of every tile does not."""
    monkeypatch.setenv("GPR_FUSED_RHS", "2")
    monkeypatch.setenv("GPR_DAG", "1")
    x, y, xp, hp = _problem(1072, 140)[:4]
    ctx = G.Context(0)
    a = _fit_predict_dev(ctx, _KINDS, hp, x, y, xp, G.GPR_PREDICT_DIAG)
    b = _fit_predict_dev(ctx, _KINDS, hp, x, y, xp, G.GPR_PREDICT_DIAG)
    for name, u, v in zip(("K", "alpha", "mu", "var"), a, b):
        assert np.array_equal(u, v), name


# the gram instance: K^{-1} = Z^T Z tile tasks, whose last row block is short (3 stages)
@pytest.mark.parametrize("n", [176, 304, 1072])
def test_fit_kinv_dag_ragged_stage_counts(n, monkeypatch):
    monkeypatch.setenv("GPR_FUSE_KINV", "2")
    monkeypatch.setenv("GPR_DAG", "1")
    monkeypatch.setenv("GPR_DAG_GRAM", "1")
    kinds = [SE, WN]
    dim = 4
    x, y, _ = O.synthetic(dim, n, 0, seed_train=n)
    hp = O.default_hp(kinds, dim, noise=0.1)
    ctx = G.Context(0)
    dx, dy = ctx.colmajor(x), ctx.colmajor(y)
    K, Kinv, alpha = ctx.empty(n, n), ctx.empty(n, n), ctx.empty(n)
    karr = (ctypes.c_int * 2)(1, 2)
    info = ctypes.c_int(-1)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = G._lib.lib.gpr_fit_kinv(ctx.h, karr, 2, hp.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                 dim, P(dx), n, P(dy), 1, n, 1e-8, P(K), n, P(alpha), P(Kinv), n,
                                 ctypes.byref(info))
    assert rc == 0 and info.value == 0
    Ko = O.kernel(kinds, hp, x)
    Uo = sla.cholesky(Ko, lower=False)
    Kd = ctx.host(K)
    assert relnorm(np.triu(Kd), Uo) < 1e-11
    np.testing.assert_allclose(ctx.host(alpha), O.cho_solve_upper(Uo, y), rtol=1e-9, atol=1e-12)
    Ki = ctx.host(Kinv)
    assert np.array_equal(Ki, Ki.T)
    assert relnorm(Ki, O.kinv_from_upper(Uo)) < 1e-10


def test_cv_batch_ragged_folds():
    """The batched instance: 7 folds of 1000 points, 130 test points each -- 870 training points
    per fold, padded to 880 = 6 x 128 + 7 x 16, and a 144-row test covariance (1 block + 1 stage)."""
    d, n, k = 3, 1000, 130
    rng = np.random.default_rng(11 + d)
    x = rng.random((d, n))
    y = np.sin(x.sum(axis=0)) ** 2
    kinds = ["SE", "WN"]
    hp = O.default_hp(kinds, d, length=2.0)
    md = G.GPRModel(G.SquaredExp() + G.WhiteNoise(), hp, x, y)
    cvset = G.kfoldcv(n, k, rng=np.random.default_rng(5))
    assert len(cvset[0]) == 7
    got = G.cv_batch(md, G.Mahalanobis(), x, y, cvset)
    want = O.cv_batch(kinds, hp, "Mahalanobis", x, y, cvset)
    np.testing.assert_allclose(got, want, rtol=1e-8, atol=0)
