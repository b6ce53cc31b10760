"""GPU: the Periodic kind through every layer -- the embedding (operand preparation), K assembly
by feature width (compile-time-S Gram tiles, the run-time-S tile, the difference forms, groups of
four parts, the upper-only build for a fit), dK/dtheta, the fused MLL gradient, fit / posterior,
cross-validation, training, sampling, and the refusals.

Expected values: the NumPy restatement of tests/test_periodic_cpu.py (difference form, feature
by feature), which that file pins to oracle/gpr_oracle.py.

Tolerances are the SquaredExp ones of tests/test_gpu_parity.py: kernel matrices rtol 1e-13 / atol
1e-15, dK/dtheta rtol 1e-12 / atol 1e-14, MLL rel 1e-10, gradient and posterior rtol 1e-8.
Kernel-matrix cases use l_k ~ 0.75 sqrt(8/d) (D <= 4 sum l^2 ~ 18..30): there the embedded forms
in float64 stay within 2e-14 relative of a long-double evaluation of the difference form; at the
suite's usual l = 3 sqrt(8/d) D reaches 288 and the float64 difference form itself is 2e-13 off
(exp's conditioning is D u).  Fit / posterior / MLL cases use l_k ~ 0.3 sqrt(8/d) and a
WhiteNoise part, and assert on the restatement that K is well away from diagonal.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.optimize

import test_periodic_cpu as R
from oracle import gpr_oracle as O
from test_periodic_cpu import M52, PER, SE, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

U53 = 2.0 ** -53
GPR_E_ARG, GPR_E_UNSUP = -1, -4


def cov_of(kinds):
    cls = {SE: G.SquaredExp, WN: G.WhiteNoise, M52: G.Matern52, PER: G.Periodic}
    c = None
    for k in kinds:
        c = cls[k]() if c is None else c + cls[k]()
    return c


def karr(kinds):
    return (ctypes.c_int * len(kinds))(*[R.KIND_CODE[k] for k in kinds])


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def relnorm(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def khp(kinds, d, rng):
    """kernel-matrix hp: l_k = 0.75 sqrt(8/d) (1 + 0.04 part) within 5 %, distinct p_k."""
    hp, p = [], 0
    for k in kinds:
        if k == WN:
            hp += [0.1]
            continue
        hp += [1.0 - 0.1 * p] + list(0.75 * np.sqrt(8.0 / d) * (1.0 + 0.04 * p) * rng.uniform(0.95, 1.05, d))
        if k == PER:
            hp += list(rng.permutation(np.linspace(0.4, 2.0, d)) if d > 1 else [0.9])
        p += 1
    return np.array(hp)


def fit_hp(kinds, d, rng):
    return R.model_hp(kinds, d, rng, lscale=0.3, noise=0.1)


def assert_well_conditioned(K):
    """the restatement's K: far from diagonal, and factorable"""
    n = K.shape[0]
    off = K[~np.eye(n, dtype=bool)]
    assert np.median(off) > 0.05, f"median off-diagonal {np.median(off):.3g}: K is nearly diagonal"
    return O.chol_upper(K)


# ---------------------------------------------------------------------------------------
# kernel matrices
# ---------------------------------------------------------------------------------------
KSETS = {
    "PER": [PER],
    "PER+WN": [PER, WN],
    "WN+PER": [WN, PER],
    "SE+PER+WN": [SE, PER, WN],
    "PER+M52": [PER, M52],                          # mix, with zero padding of the Matern part
    "SEx4+PER+WN": [SE, SE, SE, SE, PER, WN],       # the part crosses the group-of-4 boundary
    "PER+SEx4+PER": [PER, SE, SE, SE, SE, PER],
}
# feature width de = 2d: compile-time S = ceil(de/4) = 1, 2, 4, 5 (d = 1..3, 8, 10: de = 20 the
# last compile-time width), the run-time-S tile (d = 11: de = 22), de > 32 (d = 17) and raw d > 32
# (d = 33); ragged 64-tiles; an odd n is an odd leading dimension (the 8-byte-store difference
# form kernels), the last three shapes are their even-n twins (the Gram form).
SHAPES = [(1, 1), (63, 2), (65, 3), (130, 8), (98, 10), (70, 11), (66, 17), (66, 33),
          (2, 1), (64, 2), (66, 3)]


@pytest.mark.parametrize("name", list(KSETS))
@pytest.mark.parametrize("n,d", SHAPES)
def test_kernel_matrix(name, n, d):
    kinds = KSETS[name]
    rng = np.random.default_rng(n * 31 + d)
    x = rng.random((d, n))
    xp = rng.random((d, 2 * n))
    hp = khp(kinds, d, rng)
    cov = cov_of(kinds)
    K = G.kernel(cov, hp, x)
    np.testing.assert_allclose(K, R.kernel(kinds, hp, x), rtol=1e-13, atol=1e-15)
    assert np.array_equal(K, K.T), "symmetric K must be bitwise symmetric"
    Kx = G.kernel(cov, hp, x, xp)
    assert Kx.shape == (n, 2 * n)
    np.testing.assert_allclose(Kx, R.kernel(kinds, hp, x, xp), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("name,n,d", [("SE+PER+WN", 130, 4), ("SE+PER+WN", 130, 8),
                                      ("PER+SEx4+PER", 70, 11), ("PER", 66, 3), ("PER+M52", 66, 17)])
def test_kernel_matrix_difference_form(name, n, d, knobs):
    """GPR_KBUILD_EXACT=1: the difference of embedded features -- the 16-B-store kernels
    (compile-time feature width 8, 16) and the generic ones."""
    knobs("GPR_KBUILD_EXACT", 1)
    kinds = KSETS[name]
    rng = np.random.default_rng(n + d)
    x, xp = rng.random((d, n)), rng.random((d, n + 6))
    hp = khp(kinds, d, rng)
    K = G.kernel(cov_of(kinds), hp, x)
    np.testing.assert_allclose(K, R.kernel(kinds, hp, x), rtol=1e-13, atol=1e-15)
    assert np.array_equal(K, K.T)
    np.testing.assert_allclose(G.kernel(cov_of(kinds), hp, x, xp), R.kernel(kinds, hp, x, xp),
                               rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("ldk_extra,off", [(1, 0), (2, 1)])
def test_kernel_matrix_odd_ldk_and_unaligned(ldk_extra, off):
    """An odd leading dimension, and a K that is only 8-byte aligned: no 16-B stores, so the
    generic difference-form kernels; rows past n of every column stay untouched."""
    kinds = KSETS["SE+PER+WN"]
    n, m, d = 130, 70, 8
    rng = np.random.default_rng(77)
    x, xp = rng.random((d, n)), rng.random((d, m))
    hp = khp(kinds, d, rng)
    ctx = G.default_context()
    L = G._lib.lib
    ldk = n + ldk_extra
    dx, dxp = ctx.colmajor(x), ctx.colmajor(xp)
    for same, cols, want in ((1, n, R.kernel(kinds, hp, x)), (0, m, R.kernel(kinds, hp, x, xp))):
        buf = ctx.colmajor(np.full(ldk * cols + 2, -7.0))
        K = buf[off:off + ldk * cols]
        assert (K.data_ptr() % 16 == 0) == (off == 0)
        rc = L.gpr_kernel(ctx.h, karr(kinds), len(kinds), _dp(hp), d, _P(dx), n,
                          _P(None if same else dxp), cols, same, 1e-8, _P(K), ldk)
        assert rc == 0, L.gpr_last_error(ctx.h)
        got = ctx.host(buf)[off:off + ldk * cols].reshape(cols, ldk).T
        np.testing.assert_allclose(got[:n], want, rtol=1e-13, atol=1e-15)
        assert np.all(got[n:] == -7.0)
        if same:
            assert np.array_equal(got[:n], got[:n].T)


@pytest.mark.parametrize("d", [3, 8, 10])
def test_coincident_points(d):
    """xp holds exact copies of 50 columns of x: finite K, sigma^2 on the matches."""
    n, m = 128, 96
    rng = np.random.default_rng(1000 + d)
    x = rng.random((d, n))
    xp = rng.random((d, m))
    cols = rng.permutation(n)[:50]
    xp[:, :50] = x[:, cols]
    kinds = [PER, WN]
    hp = khp(kinds, d, rng)
    Kx = G.kernel(cov_of(kinds), hp, x, xp)
    assert np.all(np.isfinite(Kx))
    np.testing.assert_allclose(Kx, R.kernel(kinds, hp, x, xp), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(Kx[cols, np.arange(50)], hp[0] ** 2, rtol=1e-13)


def test_kernel_same_object_forms():
    """GPR_SELF (eps per stationary part + noise), GPR_SAME_OBJECT (eps, no noise), GPR_CROSS
    with a copy of x (neither)."""
    rng = np.random.default_rng(31)
    d, n = 4, 160
    x = rng.random((d, n))
    for name in ("PER+WN", "SE+PER+WN", "WN+PER"):
        kinds = KSETS[name]
        hp = khp(kinds, d, rng)
        cov = cov_of(kinds)
        Kself, Ksame, Kcross = G.kernel(cov, hp, x), G.kernel(cov, hp, x, x), G.kernel(cov, hp, x, x.copy())
        np.testing.assert_allclose(Kself, R.kernel(kinds, hp, x), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(Ksame, R.kernel(kinds, hp, x, x), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(Kcross, R.kernel(kinds, hp, x, x.copy()), rtol=1e-13, atol=1e-15)
        nst = sum(R.stationary(k) for k in kinds)
        sn2 = R.split_hp(kinds, hp, d)[kinds.index(WN)][0] ** 2
        np.testing.assert_allclose(np.diag(Kself) - np.diag(Ksame), sn2, rtol=1e-12)
        # (a difference of two diagonals of size <= 8: a few ulp(8) = 1.8e-15 of rounding)
        np.testing.assert_allclose(np.diag(Ksame) - np.diag(Kcross), nst * 1e-8, rtol=0, atol=2e-14)


def test_kind_and_period_are_part_of_the_cached_description():
    """Back to back on one context: SquaredExp and Periodic at equal leading hp, and two Periodic
    parts that differ only in p -- the parameter-block slot of the description made last must
    serve neither."""
    rng = np.random.default_rng(3)
    d, n = 3, 70
    x = rng.random((d, n))
    hp = khp([PER], d, rng)
    hp2 = hp.copy()
    hp2[d + 1:] = hp[d + 1:][::-1] * 1.1
    hse = hp[:d + 1]
    for kinds, h in (([PER], hp), ([SE], hse), ([PER], hp), ([PER], hp2), ([PER], hp), ([SE], hse)):
        np.testing.assert_allclose(G.kernel(cov_of(kinds), h, x), R.kernel(kinds, h, x),
                                   rtol=1e-13, atol=1e-15)


def test_kernels_per_part():
    rng = np.random.default_rng(12)
    d, n = 3, 90
    x = rng.random((d, n))
    kinds = [PER, WN, SE, M52]
    hp = khp(kinds, d, rng)
    Ks, Kr = G.kernels(cov_of(kinds), hp, x), R.kernels(kinds, hp, x)
    assert len(Ks) == 4 and Ks[1].shape == (1, 1)
    for a, b in zip(Ks, Kr):
        np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-15)


# ---------------------------------------------------------------------------------------
# dK / dtheta
# ---------------------------------------------------------------------------------------
def test_kernel_grad():
    kinds = KSETS["SE+PER+WN"]
    rng = np.random.default_rng(2)
    d, n = 3, 70
    x = rng.random((d, n))
    hp = khp(kinds, d, rng)
    cov = cov_of(kinds)
    assert len(hp) == 3 * d + 3
    for i in range(1, len(hp) + 1):
        g, go = G.grad(cov, i, hp, x), R.kernel_grad(kinds, i, hp, x)
        if isinstance(go, tuple):
            assert isinstance(g, G.UniformScaling) and g.lam == go[1]
            continue
        np.testing.assert_allclose(g, go, rtol=1e-12, atol=1e-14)


# ---------------------------------------------------------------------------------------
# MLL and the fused gradient
# ---------------------------------------------------------------------------------------
MLL_KSETS = {"PER+WN": [PER, WN], "SE+PER+WN": [SE, PER, WN]}


@functools.lru_cache(maxsize=None)
def _mll_case(name, n, d):
    kinds = MLL_KSETS[name]
    rng = np.random.default_rng(n + d)
    x = rng.random((d, n))
    y = np.sum(np.sin(x), axis=0)
    hp = fit_hp(kinds, d, rng)
    assert_well_conditioned(R.kernel(kinds, hp, x))
    L, g = R.mll(kinds, hp, x, y), R.mll_grad(kinds, hp, x, y)
    for a in (x, y, hp, g):
        a.setflags(write=False)
    return kinds, x, y, hp, L, g


@pytest.mark.parametrize("name", list(MLL_KSETS))
@pytest.mark.parametrize("n,d", [(130, 3), (256, 16), (96, 33)])
def test_mll_and_grad(name, n, d):
    kinds, x, y, hp, Lo, go = _mll_case(name, n, d)
    hp = hp.copy()
    md = G.GPRModel(cov_of(kinds), hp, x, y.copy())
    cost = G.MarginalLikelihood()
    scale = np.max(np.abs(go)) + 1.0
    L = G.loss(cost, hp, md)
    print(f"{name} n={n} d={d}: MLL rel err {abs(L - Lo) / abs(Lo):.2e}")
    assert L == pytest.approx(Lo, rel=1e-10)
    g = G.grad(cost, hp, md)
    print(f"  grad max err / scale {np.abs(g - go).max() / scale:.2e}")
    np.testing.assert_allclose(g, go, rtol=1e-8, atol=1e-8 * scale)
    tc = G.MllGradCache(md)
    Gv = np.zeros(len(hp))
    F = G.loss_grad_(cost, 0.0, Gv, hp, md, tc)
    assert F == pytest.approx(Lo, rel=1e-10)
    np.testing.assert_allclose(Gv, go, rtol=1e-8, atol=1e-8 * scale)
    Gl = np.zeros(len(hp))
    F = G.log_loss_grad_(cost, 0.0, Gl, np.log(hp), md, tc)
    assert F == pytest.approx(Lo, rel=1e-10)
    gl = go * hp
    np.testing.assert_allclose(Gl, gl, rtol=1e-8, atol=1e-8 * (1 + np.abs(gl).max()))
    assert isinstance(G.islog(cost, md), G.LogScale)


# ---------------------------------------------------------------------------------------
# fit and posterior: n = 256 goes to the tile-DAG directly, n = 300 on its padded copy;
# SE+PER+WN at d = 8 (de = 16) takes the upper-only build + DAG mirror at n = 256, d = 11
# (de = 22) the full-K fallback
# ---------------------------------------------------------------------------------------
FIT_KSETS = {"PER+WN": [PER, WN], "SE+PER+WN": [SE, PER, WN]}


@functools.lru_cache(maxsize=None)
def _fit_case(name, n, d=4):
    kinds = FIT_KSETS[name]
    m = 64
    x, y, xp = O.synthetic(d, n, m, seed_train=n, seed_test=m)
    hp = fit_hp(kinds, d, np.random.default_rng(n + d))
    K = R.kernel(kinds, hp, x)
    U = assert_well_conditioned(K)
    mu, var = R.predict(kinds, hp, x, y, xp, diagonal_var=True)
    _, S = R.predict(kinds, hp, x, y, xp, diagonal_var=False)
    for a in (x, xp, hp, K, U, mu, var, S):
        a.setflags(write=False)
    return kinds, d, x, y, xp, hp, K, U, mu, var, S


@pytest.mark.parametrize("name", list(FIT_KSETS))
@pytest.mark.parametrize("n", [256, 300])
def test_predict_vs_restatement(name, n):
    kinds, d, x, y, xp, hp, K, U, mu_o, var_o, S_o = _fit_case(name, n)
    md = G.GPRModel(cov_of(kinds), hp.copy(), x, y)
    vtol = 1e-8 * R.diag_prior(kinds, hp, d)
    mu, var = G.predict(md, xp, diagonal_var=True)
    np.testing.assert_allclose(mu, mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var, var_o, rtol=1e-8, atol=vtol)
    mu2, S = G.predict(md, xp, diagonal_var=False)
    np.testing.assert_allclose(mu2, mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(S, S_o, rtol=1e-8, atol=vtol)
    np.testing.assert_allclose(G.predict_mean(md, xp), mu_o, rtol=1e-8, atol=1e-10)
    # predict(md, md.x): the same-object rule (eps per stationary part on Kxp, no noise)
    for diag in (True, False):
        mu_s, S_s = G.predict(md, md.x, diagonal_var=diag)
        mu_so, S_so = R.predict(kinds, hp, x, y, x, diagonal_var=diag)
        np.testing.assert_allclose(mu_s, mu_so, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(S_s, S_so, rtol=1e-8, atol=vtol)
    # multi-column y
    Y = np.stack([y, np.cos(3.0 * x.sum(0)), x[0] - x[1]], axis=1)
    md3 = G.GPRModel(cov_of(kinds), hp.copy(), x, Y)
    mu3_o = R.kernel(kinds, hp, xp, x) @ O.cho_solve_upper(U, Y)
    np.testing.assert_allclose(G.predict_mean(md3, xp), mu3_o, rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("name", list(FIT_KSETS))
@pytest.mark.parametrize("n", [256, 300])
def test_fit_predict(name, n):
    """gpr_fit_predict: K, the factor, alpha and the posterior in one call."""
    kinds, d, x, y, xp, hp, K, U, mu_o, var_o, S_o = _fit_case(name, n)
    ctx = G.Context(0)
    L = G._lib.lib
    m = xp.shape[1]
    dx, dy, dxp = ctx.colmajor(x), ctx.colmajor(y), ctx.colmajor(xp)
    dK, alpha, mu, var = ctx.empty(n, n), ctx.empty(n), ctx.empty(m), ctx.empty(m)
    info = ctypes.c_int(-1)
    rc = L.gpr_fit_predict(ctx.h, karr(kinds), len(kinds), _dp(hp.copy()), d, _P(dx), n, _P(dy), 1, n,
                           1e-8, _P(dK), n, _P(alpha), _P(dxp), m, G._lib.GPR_PREDICT_DIAG, _P(mu),
                           _P(var), m, _P(None), ctypes.byref(info))
    assert rc == 0 and info.value == 0, L.gpr_last_error(ctx.h)
    np.testing.assert_allclose(ctx.host(mu), mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(ctx.host(var), var_o, rtol=1e-8, atol=1e-8 * R.diag_prior(kinds, hp, d))
    ctx.close()


@pytest.mark.parametrize("d", [8, 11])
@pytest.mark.parametrize("n", [256, 300])
def test_fit_leaves_factor_above_and_k_below(n, d):
    """gpr_fit of SE+PER+WN: strict lower triangle = K, upper = U, alpha = K^-1 y, whether the
    upper-only build and the DAG's mirror made it (d = 8: feature width 16, n = 256) or the full
    K (d = 11: feature width 22; n = 300: the padded copy)."""
    kinds, d, x, y, xp, hp, K, U, *_ = _fit_case("SE+PER+WN", n, d)
    ctx = G.Context(0)
    L = G._lib.lib
    dx, dy = ctx.colmajor(x), ctx.colmajor(y)
    dK, alpha = ctx.empty(n, n), ctx.empty(n)
    info = ctypes.c_int(-1)
    for _ in range(2):  # (twice on one context: nothing stale from the first call)
        rc = L.gpr_fit(ctx.h, karr(kinds), len(kinds), _dp(hp.copy()), d, _P(dx), n, _P(dy), 1, n,
                       1e-8, _P(dK), n, _P(alpha), ctypes.byref(info))
        assert rc == 0 and info.value == 0, L.gpr_last_error(ctx.h)
        Kd = ctx.host(dK)
        np.testing.assert_allclose(np.tril(Kd, -1), np.tril(K, -1), rtol=1e-13, atol=1e-15)
        assert relnorm(np.triu(Kd), U) < 1e-11
        a_o = O.cho_solve_upper(U, y)
        np.testing.assert_allclose(ctx.host(alpha), a_o, rtol=1e-8, atol=1e-10 * np.abs(a_o).max())
    ctx.close()


# ---------------------------------------------------------------------------------------
# cross-validation (batched launch and fold by fold), training, sampling
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("batched", [1, 0])
def test_cv_batch_mse(batched, knobs):
    knobs("GPR_CV_BATCH", batched)
    kinds = [PER, WN]
    d, n, k = 3, 200, 50
    x, y, _ = O.synthetic(d, n, 0, seed_train=11)
    hp = fit_hp(kinds, d, np.random.default_rng(4))
    md = G.GPRModel(cov_of(kinds), hp, x, y)
    cvset = G.kfoldcv(n, k, rng=np.random.default_rng(5))
    assert len(cvset[0]) == 4
    got = G.cv_batch(md, G.MSE(), x, y, cvset)
    want = R.cv_batch(kinds, hp, "MSE", x, y, cvset)
    np.testing.assert_allclose(got, want, rtol=1e-8)


@functools.lru_cache(maxsize=None)
def _train_case():
    """The restatement's optimum in log hp (L-BFGS-B on its MLL and trace-formula gradient)."""
    kinds = [PER, WN]
    d, n = 1, 120
    rng = np.random.default_rng(23)
    x = rng.random((d, n)) * 3.0
    y = np.sin(2.0 * np.pi * x[0] / 0.8) + 0.1 * rng.standard_normal(n)
    hp0 = np.array([1.0, 0.7, 0.8, 0.15])

    def fg(t):
        h = np.exp(t)
        return R.mll(kinds, h, x, y), R.mll_grad(kinds, h, x, y, log_scale=True)

    r = scipy.optimize.minimize(fg, np.log(hp0), jac=True, method="L-BFGS-B",
                                options=dict(maxiter=200, gtol=1e-7, ftol=1e-14))
    return kinds, x, y, np.exp(r.x), float(r.fun)


def test_train_reaches_the_restatements_optimum():
    """From 3 % beside the restatement's optimum hp* (the period: 0.3 %, inside its basin) the
    device's L-BFGS on the log scale must end at the optimum's value.  The Hessian of the MLL in
    log hp at hp* has eigenvalues 2.07 .. 2.4e5 (central differences of the restatement's
    gradient), so a stop at |g|_inf <= g_tol = 1e-3 leaves L - L* <= |g|_2^2 / (2 lambda_min)
    <= 4e-6 / 4.1 = 1e-6, and L-BFGS-B's other stop, a relative decrease below 2.2e-9, is taken
    only next to that; asserted with 1e-4.  Below L* the run cannot go by more than the
    restatement's own optimiser left: its gradient residual 5e-6 gives 1e-11."""
    kinds, x, y, hps, Ls = _train_case()
    hp_start = hps * np.array([1.03, 0.97, 1.003, 1.03])
    md = G.GPRModel(cov_of(kinds), hp_start.copy(), x, y)
    # (train takes its start as the optimiser's variable, which on the log scale is log hp)
    hp_tr, res = G.train(md, G.MarginalLikelihood(), np.log(hp_start), method=G.LBFGS(),
                         options=G.Options(g_tol=1e-3, iterations=60))
    assert hp_tr.shape == hps.shape and np.all(np.isfinite(hp_tr)) and np.all(hp_tr > 0)
    L0 = R.mll(kinds, hp_start, x, y)
    print(f"L* {Ls:.8f} start {L0:.8f} trained {res.minimum:.8f} hp {hp_tr} hp* {hps}")
    np.testing.assert_allclose(res.minimum, R.mll(kinds, hp_tr, x, y), rtol=1e-8)
    assert res.minimum < L0
    assert Ls - 1e-6 * (1.0 + abs(Ls)) <= res.minimum <= Ls + 1e-4


def test_sample_prior_with_given_z():
    """S = mu + U^T z with U the factor of K' = K + 1e-7 (every element): forward error of a
    backward-stable Cholesky, 8 n u kappa_2(K') ||U||_2 ||Z||_F (tests/test_gpu_sample.py)."""
    kinds = [PER, WN]
    d, n, ns = 2, 200, 3
    rng = np.random.default_rng(17 * n)
    x = rng.random((d, n))
    hp = fit_hp(kinds, d, rng)
    z = rng.standard_normal((n, ns))
    Kp = R.kernel(kinds, hp, x) + 1e-7
    w = np.linalg.eigvalsh(Kp)
    kappa = w[-1] / w[0]
    assert 0.0 < w[0] and kappa < 1e6, f"kappa_2 = {kappa:.3e}: the bound would be empty"
    bound = 8.0 * n * U53 * kappa * np.sqrt(w[-1]) * np.linalg.norm(z)
    mu = x.sum(axis=0)
    S_ref = np.linalg.cholesky(Kp) @ z + mu[:, None]
    gp = G.GaussianProcess(lambda c: c.sum(), cov_of(kinds))
    S = G.sample(gp(x, hp), z=z)
    err = np.linalg.norm(S - S_ref)
    print(f"prior PER+WN n={n}: kappa {kappa:.2e} err {err:.3e} bound {bound:.3e}")
    assert S.shape == (n, ns) and err <= bound


# ---------------------------------------------------------------------------------------
# refused: the calls built on SquaredExp's separability or its erf integrals; bad periods
# ---------------------------------------------------------------------------------------
def _unsup(excinfo):
    msg = str(excinfo.value)
    return f"({GPR_E_UNSUP})" in msg and "part 2 is Periodic" in msg


def test_refusals():
    rng = np.random.default_rng(41)
    d, n = 2, 64
    x = rng.random((d, n))
    y = np.sin(x.sum(0))
    kinds = [SE, PER, WN]
    hp = fit_hp(kinds, d, rng)
    cov = cov_of(kinds)
    md = G.GPRModel(cov, hp, x, y)
    cm = G.Cmap("+", rng.random((d, 5)), rng.random((d, 7)))
    with pytest.raises(G.GprError) as e:
        G.predict(md, cm, diagonal_var=True)
    assert _unsup(e), str(e.value)
    with pytest.raises(G.GprError) as e:
        G.integrate(md, np.zeros(d), np.ones(d))
    assert _unsup(e), str(e.value)
    with pytest.raises(G.GprError) as e:
        G.integrate(md, np.zeros(d), np.ones(d), sample_noise=np.array([0.1]))
    assert _unsup(e), str(e.value)
    with pytest.raises(G.GprError) as e:
        G.split_factors(cov, hp, x, cm, part=0)
    assert _unsup(e), str(e.value)
    # nothing is written: the raw calls leave their outputs as they were
    ctx = G.default_context()
    L = G._lib.lib
    nk = len(kinds)
    dx, dy, dxe, dxq = ctx.colmajor(x), ctx.colmajor(y), ctx.colmajor(cm.xe), ctx.colmajor(cm.xq)
    seven = lambda s: ctx.colmajor(np.full(s, -7.0))  # noqa: E731
    untouched = lambda *ts: all(np.all(ctx.host(t) == -7.0) for t in ts)  # noqa: E731
    err = lambda: L.gpr_last_error(ctx.h)  # noqa: E731
    A, B, C = seven(5 * 7), seven(5 * n), seven(n * 7)
    rc = L.gpr_split_factors(ctx.h, karr(kinds), nk, _dp(hp), d, _P(dx), n, _P(dxe), 5, _P(dxq), 7,
                             0, _P(A), _P(B), _P(C))
    assert rc == GPR_E_UNSUP and b"part 2 is Periodic" in err() and untouched(A, B, C)
    dU, wt, mu, var = seven(n * n), seven(n), seven(5 * 7), seven(5 * 7)
    rc = L.gpr_split_predict(ctx.h, karr(kinds), nk, _dp(hp), d, _P(dx), n, _P(dU), n, _P(wt),
                             _P(dxe), 5, _P(dxq), 7, 0, 5, 0, 5, 1e-8, _P(mu), _P(var))
    assert rc == GPR_E_UNSUP and b"part 2 is Periodic" in err() and untouched(mu, var)
    a, b = np.zeros(d), np.ones(d)
    dK, dwt = seven(n * n), seven(n)
    Iout, ivar = np.full(1, -7.0), np.full(1, -7.0)
    rc = L.gpr_integrate(ctx.h, karr(kinds), nk, _dp(hp), d, _P(dx), n, _P(dy), 1, n, _dp(a), _dp(b),
                         1e-8, _P(dK), n, _P(dwt), _dp(Iout), _dp(ivar))
    assert rc == GPR_E_UNSUP and b"part 2 is Periodic" in err() and untouched(dK, dwt)
    assert Iout[0] == -7.0 and ivar[0] == -7.0
    noise = np.array([0.1, 0.2])
    Iout, ivar = np.full(2, -7.0), np.full(2, -7.0)
    rc = L.gpr_integrate_noise(ctx.h, karr(kinds), nk, _dp(hp), d, _P(dx), n, _P(dy), 1, n, _dp(a),
                               _dp(b), _dp(noise), 1e-8, _dp(Iout), _dp(ivar))
    assert rc == GPR_E_UNSUP and b"part 2 is Periodic" in err()
    assert np.all(Iout == -7.0) and np.all(ivar == -7.0)
    # the one-process multi-GPU split prediction (host arrays)
    from gpr_amd import distributed as Dm
    mg = Dm.MultiGPU([0])
    Dp = ctypes.POINTER(ctypes.c_double)
    c = lambda v: np.ascontiguousarray(v, dtype=np.float64)  # noqa: E731
    X, Xe, Xq = c(x.T), c(cm.xe.T), c(cm.xq.T)
    mu_h, var_h = np.full((7, 5), -7.0), np.full(35, -7.0)
    info = ctypes.c_int(0)
    rc = L.gpr_split_predict_mgpu(mg.h, karr(kinds), nk, _dp(hp), d, X.ctypes.data_as(Dp), n, _dp(y),
                                  Xe.ctypes.data_as(Dp), 5, Xq.ctypes.data_as(Dp), 7, 0, 5, 1e-8, 0,
                                  mu_h.ctypes.data_as(Dp), var_h.ctypes.data_as(Dp), ctypes.byref(info))
    assert rc == GPR_E_UNSUP and b"part 2 is Periodic" in L.gpr_mgpu_last_error(mg.h)
    assert np.all(mu_h == -7.0) and np.all(var_h == -7.0)
    mg.close()
    # and the SquaredExp description next door still works
    A2, _, _ = G.split_factors(cov_of([SE, WN]), np.array([1.0, 1.0, 1.0, 0.1]), x, cm, part=0)
    assert np.all(np.isfinite(A2))


@pytest.mark.parametrize("bad", [0.0, float("nan"), float("inf")])
def test_bad_period_is_an_argument_error(bad):
    """p_k zero, NaN or infinite: GPR_E_ARG naming the part and the dimension, K untouched."""
    rng = np.random.default_rng(8)
    d, n = 3, 40
    x = rng.random((d, n))
    kinds = [SE, PER, WN]
    hp = khp(kinds, d, rng)
    hp[(d + 1) + 1 + d + 1] = bad  # p_2 of part 2
    ctx = G.default_context()
    L = G._lib.lib
    dx = ctx.colmajor(x)
    K = ctx.colmajor(np.full(n * n, -7.0))
    rc = L.gpr_kernel(ctx.h, karr(kinds), 3, _dp(hp), d, _P(dx), n, _P(None), n, 1, 1e-8, _P(K), n)
    msg = L.gpr_last_error(ctx.h).decode()
    assert rc == GPR_E_ARG and "part 2" in msg and "dimension 2" in msg, msg
    assert np.all(ctx.host(K) == -7.0)
    with pytest.raises(G.GprError):
        G.kernel(cov_of(kinds), hp, x)
