"""The tile-DAG's accumulation loop (dag.hip dag_accum) with scalar-addressed LDS-DMA and a
five-fold unrolled ring.

The loop runs whole groups of five two-stage periods (two laps of the five LDS buffers, so the
ring position is a compile-time value) and then the 0..4 periods that are left, each behind a
check of its own, and an odd stage count ends with a single-stage half period.  An accumulation
over f row blocks runs 8 f stages = 4 f periods, so f = 1, 2, 3, 4, 5, 6, 11 leaves 4, 3, 2, 1,
0, 4, 4 periods behind 0, 1, 2, 3, 4, 4, 8 groups: every way out of the loop, and more than one
trip round it.  A last tile row of t = 0, 1, 3, 6 stages gives the row clamp of the DMA sources
(rows past the matrix re-read the last valid one) and the W-product's odd stage counts.  All of
it in the four instances of the kernel: the plain factorisation, the right-hand sides inside
gpr_fit_predict's launch, the gram tasks (gpr_fit_kinv) and a batched launch (cv_batch, whose
only outputs are the fold losses: they are checked against the oracle's, which come from SciPy
factorisations of the same folds).

The DMA source of a lane is a scalar base per 8-row piece plus a 32-bit lane offset that holds
(row in the piece) * ld * 8: the same matrix under three leading dimensions must give the same
bits, for A and for B.  The launch takes leading dimensions up to 2^25 doubles directly (56 ld +
128 < 2^31 bytes); the host predicate is checked at that bound without a GPU.

Tolerances are those of tests/test_gpu_dag_ring.py; helpers copied from there.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.linalg as sla

from oracle import gpr_oracle as O

G = pytest.importorskip("gpr_amd")

SE, WN = O.SE, O.WN

_F = [1, 2, 3, 4, 5, 6, 11]
_T = [0, 1, 3, 6]
_SIZES = [128 * f + 16 * t for f in _F for t in _T]

_LD_MAX = 1 << 25


def relnorm(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@functools.lru_cache(maxsize=None)
def _spd(n, d=4, noise=0.3):
    """A kernel matrix and its SciPy factor, computed once per size (callers do not write)."""
    rng = np.random.default_rng(n + 7)
    x = rng.random((d, n))
    A = O.kernel([SE, WN], np.r_[1.0, [1.5] * d, noise], x)
    return A, sla.cholesky(A, lower=False)


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _dev_potrf_ld(ctx, A, lda):
    """A into the first n rows of an lda x n column-major buffer (NaN beyond), factored there."""
    n = A.shape[0]
    buf = np.full((lda, n), np.nan)
    buf[:n] = A
    dA = ctx.colmajor(buf)
    info = ctypes.c_int(-7)
    rc = G._lib.lib.gpr_potrf_upper(ctx.h, _P(dA), n, lda, ctypes.byref(info))
    assert rc >= 0, G._lib.lib.gpr_last_error(ctx.h)
    assert info.value == 0
    return dA


@pytest.mark.gpu
@pytest.mark.parametrize("n", _SIZES)
def test_potrf_every_exit_of_the_ring(n, monkeypatch):
    monkeypatch.setenv("GPR_DAG", "1")
    ctx = G.Context(0)
    A, U = _spd(n)
    dA = _dev_potrf_ld(ctx, A, n)
    R = ctx.host(dA)
    assert relnorm(np.triu(R), U) < 1e-12
    assert np.array_equal(np.tril(R, -1), np.tril(A, -1))
    B = np.random.default_rng(4).random((n, 2))
    dB = ctx.colmajor(B)
    assert G._lib.lib.gpr_potrs_upper(ctx.h, _P(dA), n, n, _P(dB), 2, n) == 0
    assert relnorm(ctx.host(dB), O.cho_solve_upper(U, B)) < 1e-11


_KINDS = [SE, WN]
_DIM = 3
_NPRED = 5  # np + 1 = 6 right-hand sides: one ragged column tile


@functools.lru_cache(maxsize=None)
def _problem(n):
    x, y, xp = O.synthetic(_DIM, n, _NPRED, seed_train=n, seed_test=_NPRED)
    hp = O.default_hp(_KINDS, _DIM, noise=0.05)
    K = O.kernel(_KINDS, hp, x)
    U = sla.cholesky(K, lower=False)
    alpha = O.cho_solve_upper(U, y)
    mu, var = O.predict(_KINDS, hp, x, y, xp, diagonal_var=True)
    return x, y, xp, hp, K, alpha, mu, var


def _fit_predict_dev(ctx, hp, x, y, xp):
    d, n = x.shape
    m = xp.shape[1]
    dx, dy, dxp = ctx.colmajor(x), ctx.colmajor(y[:, None]), ctx.colmajor(xp)
    K, alpha, mu, var = ctx.empty(n, n), ctx.empty(1, n), ctx.empty(1, m), ctx.empty(m)
    karr = (ctypes.c_int * 2)(1, 2)
    hpa = np.asarray(hp, dtype=np.float64)
    info = ctypes.c_int(-1)
    rc = G._lib.lib.gpr_fit_predict(ctx.h, karr, 2, hpa.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                    d, _P(dx), n, _P(dy), 1, n, 1e-8, _P(K), n, _P(alpha), _P(dxp), m,
                                    G.GPR_PREDICT_DIAG, _P(mu), _P(var), m, None, ctypes.byref(info))
    assert rc == 0 and info.value == 0, G._lib.lib.gpr_last_error(ctx.h)
    return ctx.host(K), ctx.host(alpha), ctx.host(mu), ctx.host(var)


@pytest.mark.gpu
@pytest.mark.parametrize("n", _SIZES)
def test_fit_predict_every_exit_of_the_ring(n, monkeypatch):
    monkeypatch.setenv("GPR_FUSED_RHS", "2")
    monkeypatch.setenv("GPR_DAG", "1")
    x, y, xp, hp, K, alpha_o, mu_o, var_o = _problem(n)
    ctx = G.Context(0)
    Kd, alpha, mu, var = _fit_predict_dev(ctx, hp, x, y, xp)
    np.testing.assert_allclose(np.tril(Kd, -1), np.tril(K, -1), rtol=1e-13, atol=1e-15)
    Kdev = np.tril(Kd) + np.tril(Kd, -1).T
    np.fill_diagonal(Kdev, np.diag(K))
    assert relnorm(np.triu(Kd), sla.cholesky(Kdev, lower=False)) < 1e-11
    np.testing.assert_allclose(alpha.ravel(), alpha_o, rtol=1e-8, atol=1e-10 * np.abs(alpha_o).max())
    np.testing.assert_allclose(mu.ravel(), mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var, var_o, rtol=1e-8, atol=1e-8 * O.diag_prior(_KINDS, hp, _DIM))


@pytest.mark.gpu
@pytest.mark.parametrize("n", _SIZES)
def test_fit_kinv_every_exit_of_the_ring(n, monkeypatch):
    monkeypatch.setenv("GPR_FUSE_KINV", "2")
    monkeypatch.setenv("GPR_DAG", "1")
    monkeypatch.setenv("GPR_DAG_GRAM", "1")
    dim = 4
    x, y, _ = O.synthetic(dim, n, 0, seed_train=n)
    hp = O.default_hp(_KINDS, dim, noise=0.1)
    ctx = G.Context(0)
    dx, dy = ctx.colmajor(x), ctx.colmajor(y)
    K, Kinv, alpha = ctx.empty(n, n), ctx.empty(n, n), ctx.empty(n)
    karr = (ctypes.c_int * 2)(1, 2)
    info = ctypes.c_int(-1)
    rc = G._lib.lib.gpr_fit_kinv(ctx.h, karr, 2, hp.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                 dim, _P(dx), n, _P(dy), 1, n, 1e-8, _P(K), n, _P(alpha), _P(Kinv), n,
                                 ctypes.byref(info))
    assert rc == 0 and info.value == 0
    Ko = O.kernel(_KINDS, hp, x)
    Uo = sla.cholesky(Ko, lower=False)
    Kd = ctx.host(K)
    assert relnorm(np.triu(Kd), Uo) < 1e-11
    np.testing.assert_allclose(np.tril(Kd, -1), np.tril(Ko, -1), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(ctx.host(alpha), O.cho_solve_upper(Uo, y), rtol=1e-9, atol=1e-12)
    Ki = ctx.host(Kinv)
    assert np.array_equal(Ki, Ki.T)
    assert relnorm(Ki, O.kinv_from_upper(Uo)) < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("n", _SIZES)
def test_cv_batch_every_exit_of_the_ring(n):
    """Three folds of n training points each (40 test points: a 48-row test covariance)."""
    d, k = 3, 40
    rng = np.random.default_rng(11 + n)
    x = rng.random((d, n + k))
    y = np.sin(x.sum(axis=0)) ** 2
    kinds = ["SE", "WN"]
    hp = O.default_hp(kinds, d, length=2.0)
    md = G.GPRModel(G.SquaredExp() + G.WhiteNoise(), hp, x, y)
    cvset = G.kfoldcv(n + k, k, nb=3, rng=np.random.default_rng(5))
    assert len(cvset[0]) == 3 and len(cvset[0][0]) == n
    got = G.cv_batch(md, G.Mahalanobis(), x, y, cvset)
    want = O.cv_batch(kinds, hp, "Mahalanobis", x, y, cvset)
    np.testing.assert_allclose(got, want, rtol=1e-8, atol=0)


# 3 row blocks and a 3-stage last tile row: ragged, more than one workgroup's worth of tiles
@pytest.mark.gpu
def test_factor_bitwise_equal_across_lda(monkeypatch):
    monkeypatch.setenv("GPR_DAG", "1")
    n = 432
    A, U = _spd(n)
    ctx = G.Context(0)
    ref = ctx.host(_dev_potrf_ld(ctx, A, n))
    assert relnorm(np.triu(ref), U) < 1e-12
    for lda in (n + 16, n + 1040):
        R = ctx.host(_dev_potrf_ld(ctx, A, lda))
        assert np.array_equal(R[:n], ref), lda
        assert np.isnan(R[n:]).all(), lda  # nothing written below the matrix


@pytest.mark.gpu
def test_solve_bitwise_equal_across_ldb(monkeypatch):
    """The solve-only launch: B's tiles are the tasks, B's leading dimension the DMA's."""
    monkeypatch.setenv("GPR_DAG", "1")
    monkeypatch.setenv("GPR_DAG_SOLVE", "1")
    n, nrhs = 432, 144
    A, U = _spd(n)
    B = np.random.default_rng(9).random((n, nrhs))
    ctx = G.Context(0)
    dA = _dev_potrf_ld(ctx, A, n)
    out = []
    for ldb in (n, n + 16, n + 1040):
        buf = np.full((ldb, nrhs), np.nan)
        buf[:n] = B
        dB = ctx.colmajor(buf)
        assert G._lib.lib.gpr_potrs_upper(ctx.h, _P(dA), n, n, _P(dB), nrhs, ldb) == 0
        X = ctx.host(dB)
        assert np.isnan(X[n:]).all(), ldb
        out.append(X[:n])
    assert relnorm(out[0], O.cho_solve_upper(U, B)) < 1e-11
    assert np.array_equal(out[1], out[0])
    assert np.array_equal(out[2], out[0])


@pytest.mark.gpu
def test_factor_and_solve_repeatable(monkeypatch):
    monkeypatch.setenv("GPR_FUSED_RHS", "2")
    monkeypatch.setenv("GPR_DAG", "1")
    x, y, xp, hp = _problem(1504)[:4]
    ctx = G.Context(0)
    a = _fit_predict_dev(ctx, hp, x, y, xp)
    b = _fit_predict_dev(ctx, hp, x, y, xp)
    for name, u, v in zip(("K", "alpha", "mu", "var"), a, b):
        assert np.array_equal(u, v), name


def test_shape_predicate_at_the_ld_bound():
    """Host only: the launch takes ld <= 2^25 directly; anything larger goes to the padded copy."""
    ok = G._lib.lib.gpr_debug_dag_shape_ok
    ok.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong]
    ok.restype = ctypes.c_int
    base = 1 << 20
    assert ok(256, 256, base) == 1
    assert ok(256, _LD_MAX, base) == 1
    assert ok(256, _LD_MAX + 16, base) == 0
    assert ok(256, (1 << 31) - 16, base) == 0
    # the largest lane offset at the bound (row 7 of a piece, last chunk) fits 31 bits
    assert 7 * 8 * _LD_MAX + 128 < 1 << 31
    # the other conditions are unchanged
    assert ok(250, 256, base) == 0 and ok(256, 264, base) == 0 and ok(256, 256, base + 64) == 0
