"""GPU: the Matern-3/2 and Matern-5/2 kinds through every layer -- K assembly (Gram-form MFMA
tiles, the difference-form fallbacks, groups of four parts), dK/dtheta, the fused MLL gradient
(both kernels), fit / posterior, cross-validation, training, sampling, and the refusals.

Expected values: the NumPy restatement of tests/test_matern_cpu.py (difference form), which
that file pins to oracle/gpr_oracle.py for SquaredExp / WhiteNoise descriptions.

Tolerances are those of the SquaredExp tests of tests/test_gpu_parity.py: kernel matrices rtol
1e-13 / atol 1e-15 (the Gram form's absolute error in D enters K through |d ln k / dD| = W / k
<= 3/2 (M32), 5/6 (M52), 1 (SE): at most 1.5 x SquaredExp's relative error), dK/dtheta rtol
1e-12 / atol 1e-14, MLL rel 1e-10, gradient and posterior rtol 1e-8.
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import test_matern_cpu as R
from oracle import gpr_oracle as O
from test_matern_cpu import M32, M52, SE, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

U53 = 2.0 ** -53
GPR_E_UNSUP = -4


def cov_of(kinds):
    cls = {SE: G.SquaredExp, WN: G.WhiteNoise, M32: G.Matern32, M52: G.Matern52}
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


def model_hp(kinds, d, noise=0.1):
    """sigma = 1, l_k = 3 sqrt(8/d) per stationary part (slightly different per part), sigma_n."""
    hp, p = [], 0
    for k in kinds:
        if k == WN:
            hp += [noise]
        else:
            hp += [1.0 - 0.2 * p] + [3.0 * np.sqrt(8.0 / d) * (1.0 + 0.25 * p)] * d
            p += 1
    return np.array(hp)


# ---------------------------------------------------------------------------------------
# kernel matrices
# ---------------------------------------------------------------------------------------
KSETS = {
    "M52": [M52],
    "M32": [M32],
    "M52+WN": [M52, WN],
    "WN+M32": [WN, M32],
    "SE+M52+WN": [SE, M52, WN],
    "M32+SE": [M32, SE],
    "SEx4+M52+WN": [SE, SE, SE, SE, M52, WN],      # the profile crosses the group-of-4 boundary
    "M52+SEx4+M32": [M52, SE, SE, SE, SE, M32],
}
# the ragged 64-tiles, each compiled S = ceil(d/4) <= 5, the run-time-S tile (d = 21) and d > 32.
# An odd n is an odd leading dimension (the difference-form kernels); the last four shapes take
# the same S = 1, 3, 4, 5 through the Gram form (even n).
SHAPES = [(1, 1), (63, 2), (65, 5), (130, 8), (97, 20), (70, 21), (66, 33),
          (66, 3), (68, 11), (72, 14), (98, 20)]


@pytest.mark.parametrize("name", list(KSETS))
@pytest.mark.parametrize("n,d", SHAPES)
def test_kernel_matrix(name, n, d):
    kinds = KSETS[name]
    rng = np.random.default_rng(n * 31 + d)
    x = rng.random((d, n))
    xp = rng.random((d, 2 * n))
    hp = R.rand_hp(kinds, d, rng)
    cov = cov_of(kinds)
    K = G.kernel(cov, hp, x)
    np.testing.assert_allclose(K, R.kernel(kinds, hp, x), rtol=1e-13, atol=1e-15)
    assert np.array_equal(K, K.T), "symmetric K must be bitwise symmetric"
    Kx = G.kernel(cov, hp, x, xp)
    assert Kx.shape == (n, 2 * n)
    np.testing.assert_allclose(Kx, R.kernel(kinds, hp, x, xp), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("name,n,d", [("SE+M52+WN", 130, 8), ("M52+SEx4+M32", 70, 21),
                                      ("M32", 66, 3)])
def test_kernel_matrix_difference_form(name, n, d, knobs):
    """GPR_KBUILD_EXACT=1: the 16-B-store difference-form kernels (compile-time d) and, for
    more than four parts or another d, the generic ones."""
    knobs("GPR_KBUILD_EXACT", 1)
    kinds = KSETS[name]
    rng = np.random.default_rng(n + d)
    x, xp = rng.random((d, n)), rng.random((d, n + 6))
    hp = R.rand_hp(kinds, d, rng)
    K = G.kernel(cov_of(kinds), hp, x)
    np.testing.assert_allclose(K, R.kernel(kinds, hp, x), rtol=1e-13, atol=1e-15)
    assert np.array_equal(K, K.T)
    np.testing.assert_allclose(G.kernel(cov_of(kinds), hp, x, xp), R.kernel(kinds, hp, x, xp),
                               rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("ldk_extra,off", [(1, 0), (2, 1)])
def test_kernel_matrix_odd_ldk_and_unaligned(ldk_extra, off):
    """An odd leading dimension, and a K that is only 8-byte aligned: no 16-B stores, so the
    generic difference-form kernels; rows past n of every column stay untouched."""
    kinds = KSETS["SE+M52+WN"]
    n, m, d = 130, 70, 8
    rng = np.random.default_rng(77)
    x, xp = rng.random((d, n)), rng.random((d, m))
    hp = R.rand_hp(kinds, d, rng)
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


@pytest.mark.parametrize("kind", [M32, M52])
@pytest.mark.parametrize("d", [5, 8, 20])
def test_coincident_points_are_clamped(kind, d):
    """xp holds exact copies of 50 columns of x: the Gram form's D comes out a few 1e-16 below
    zero for some of them, and sqrt of that is a NaN unless D is clamped at 0."""
    n, m = 128, 96
    rng = np.random.default_rng(1000 + d)
    x = rng.random((d, n))
    xp = rng.random((d, m))
    cols = rng.permutation(n)[:50]
    xp[:, :50] = x[:, cols]
    kinds = [kind, WN]
    hp = R.rand_hp(kinds, d, rng)
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
    for name in ("M52+WN", "SE+M52+WN", "WN+M32"):
        kinds = KSETS[name]
        hp = R.rand_hp(kinds, d, rng)
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


def test_profile_is_part_of_the_cached_description():
    """Equal hp, different profile, back to back on one context: the parameter-block slot of
    the description made last must not serve the other kind."""
    rng = np.random.default_rng(3)
    d, n = 3, 70
    x = rng.random((d, n))
    hp = R.rand_hp([SE], d, rng)
    for kind in (SE, M52, M32, SE, M32):
        np.testing.assert_allclose(G.kernel(cov_of([kind]), hp, x), R.kernel([kind], hp, x),
                                   rtol=1e-13, atol=1e-15)


def test_kernels_per_part():
    rng = np.random.default_rng(12)
    d, n = 3, 90
    x = rng.random((d, n))
    kinds = [M52, WN, SE, M32]
    hp = R.rand_hp(kinds, d, rng)
    Ks, Kr = G.kernels(cov_of(kinds), hp, x), R.kernels(kinds, hp, x)
    assert len(Ks) == 4 and Ks[1].shape == (1, 1)
    for a, b in zip(Ks, Kr):
        np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-15)


# ---------------------------------------------------------------------------------------
# dK / dtheta
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SE+M52+WN", "M32"])
def test_kernel_grad(name):
    kinds = KSETS[name]
    rng = np.random.default_rng(2)
    d, n = 3, 70
    x = rng.random((d, n))
    hp = R.rand_hp(kinds, d, rng)
    cov = cov_of(kinds)
    for i in range(1, len(hp) + 1):
        g, go = G.grad(cov, i, hp, x), R.kernel_grad(kinds, i, hp, x)
        if isinstance(go, tuple):
            assert isinstance(g, G.UniformScaling) and g.lam == go[1]
            continue
        np.testing.assert_allclose(g, go, rtol=1e-12, atol=1e-14)


# ---------------------------------------------------------------------------------------
# MLL and the fused gradient: d <= 32 (mll_grad_tiles_kernel), d > 32 (mll_grad_wide_kernel),
# six parts (the table re-fill between groups of four)
# ---------------------------------------------------------------------------------------
MLL_KSETS = {"M52+WN": [M52, WN], "SE+M32+WN": [SE, M32, WN], "SEx4+M52+WN": KSETS["SEx4+M52+WN"]}


@functools.lru_cache(maxsize=None)
def _mll_case(name, n, d):
    kinds = MLL_KSETS[name]
    rng = np.random.default_rng(n + d)
    x = rng.random((d, n))
    y = np.sum(np.sin(x), axis=0)
    hp = []
    for k in kinds:
        hp += [0.3] if k == WN else [rng.uniform(0.7, 1.2)] + list(rng.uniform(0.5, 2.0, d) / np.sqrt(d))
    hp = np.array(hp)
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
# fit and posterior: n = 256 goes to the tile-DAG directly, n = 300 on its padded copy
# ---------------------------------------------------------------------------------------
FIT_KSETS = {"M52+WN": [M52, WN], "SE+M32+WN": [SE, M32, WN]}


@functools.lru_cache(maxsize=None)
def _fit_case(name, n):
    kinds = FIT_KSETS[name]
    d, m = 4, 64
    x, y, xp = O.synthetic(d, n, m, seed_train=n, seed_test=m)
    hp = model_hp(kinds, d, noise=0.1)
    K = R.kernel(kinds, hp, x)
    U = O.chol_upper(K)
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
def test_fit_leaves_factor_above_and_k_below(name, n):
    """gpr_fit with a Matern part builds the full K under the tile-DAG (no upper-only build, no
    mirror flag left behind): strict lower triangle = K, upper = U, alpha = K^-1 y."""
    kinds, d, x, y, xp, hp, K, U, *_ = _fit_case(name, n)
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
    kinds = [M52, WN]
    d, n, k = 3, 200, 50
    x, y, _ = O.synthetic(d, n, 0, seed_train=11)
    hp = model_hp(kinds, d, noise=0.1)
    md = G.GPRModel(cov_of(kinds), hp, x, y)
    cvset = G.kfoldcv(n, k, rng=np.random.default_rng(5))
    assert len(cvset[0]) == 4
    got = G.cv_batch(md, G.MSE(), x, y, cvset)
    want = R.cv_batch(kinds, hp, "MSE", x, y, cvset)
    np.testing.assert_allclose(got, want, rtol=1e-8)


def test_train():
    kinds = [M52, WN]
    d, n = 2, 200
    x, y, _ = O.synthetic(d, n, 0, seed_train=23)
    hp0 = np.array([1.0, 1.0, 1.0, 0.3])
    md = G.GPRModel(cov_of(kinds), hp0.copy(), x, y)
    hp_tr, res = G.train(md, G.MarginalLikelihood(), hp0, method=G.LBFGS(),
                         options=G.Options(g_tol=1e-2, iterations=30))
    assert hp_tr.shape == hp0.shape and np.all(np.isfinite(hp_tr)) and np.all(hp_tr > 0)
    np.testing.assert_allclose(res.minimum, R.mll(kinds, hp_tr, x, y), rtol=1e-8)
    assert res.minimum < R.mll(kinds, hp0, x, y)


def test_sample_prior_with_given_z():
    """S = mu + U^T z with U the factor of K' = K + 1e-7 (every element): forward error of a
    backward-stable Cholesky, 8 n u kappa_2(K') ||U||_2 ||Z||_F (tests/test_gpu_sample.py)."""
    kinds = [M32, WN]
    d, n, ns = 2, 200, 3
    rng = np.random.default_rng(17 * n)
    x = rng.random((d, n))
    hp = R.rand_hp(kinds, d, rng)
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
    print(f"prior M32+WN n={n}: kappa {kappa:.2e} err {err:.3e} bound {bound:.3e}")
    assert S.shape == (n, ns) and err <= bound


# ---------------------------------------------------------------------------------------
# refused: the calls built on SquaredExp's separability or its erf integrals
# ---------------------------------------------------------------------------------------
def _unsup(excinfo):
    msg = str(excinfo.value)
    return f"({GPR_E_UNSUP})" in msg and "Matern" in msg


def test_refusals():
    rng = np.random.default_rng(41)
    d, n = 2, 64
    x = rng.random((d, n))
    y = np.sin(x.sum(0))
    kinds = [SE, M52, WN]
    hp = model_hp(kinds, d)
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
    # nothing is written: the raw call leaves its outputs as they were
    ctx = G.default_context()
    L = G._lib.lib
    dx, dxe, dxq = ctx.colmajor(x), ctx.colmajor(cm.xe), ctx.colmajor(cm.xq)
    A, B, C = (ctx.colmajor(np.full(s, -7.0)) for s in (5 * 7, 5 * n, n * 7))
    rc = L.gpr_split_factors(ctx.h, karr(kinds), 3, _dp(hp), d, _P(dx), n, _P(dxe), 5, _P(dxq), 7,
                             0, _P(A), _P(B), _P(C))
    assert rc == GPR_E_UNSUP and b"Matern52" in L.gpr_last_error(ctx.h)
    for t in (A, B, C):
        assert np.all(ctx.host(t) == -7.0)
    # and the SquaredExp description next door still works
    A2, _, _ = G.split_factors(cov_of([SE, WN]), model_hp([SE, WN], d), x, cm, part=0)
    assert np.all(np.isfinite(A2))
