"""GPU: product kernels (`*`) through every layer -- the description (markers, term table, groups
cut at term boundaries), K assembly in its PROD instantiations (Gram tiles, the run-time-S tile,
the difference forms, the upper-only build of a fit), dK/dtheta, the fused MLL gradient and the
posterior gradients in their PROD forms, fit / posterior, append, cross-validation, sampling,
training, and the refusals.

Expected values: the NumPy restatement of tests/test_product_cpu.py (per-factor functions of
tests/test_periodic_cpu.py, difference form), which that file pins by central differences.

Tolerances are the project's (tests/test_gpu_periodic.py): kernel matrices rtol 1e-13 / atol
1e-15, dK/dtheta rtol 1e-12 F / atol 1e-14 for a term of F factors, MLL rel 1e-10, gradient and
posterior rtol 1e-8.  Kernel-matrix cases use l_k = 0.75 sqrt(8/d) / sqrt(F) within 5 % for a term
of F factors, so that the product's exponent sum_f D_f stays the size of one part's (there the
float64 difference-form restatement is within 1.1e-14 relative of a long-double evaluation).
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.optimize

import test_periodic_cpu as P
import test_product_cpu as R
from oracle import gpr_oracle as O
from test_append_cpu import TOL_MU, TOL_U
from test_periodic_cpu import M32, M52, PER, SE, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

U53 = 2.0 ** -53
GPR_E_ARG, GPR_E_UNSUP = -1, -4
MUL = R.MUL_CODE
cov_of = R.cov_of


def karr(desc):
    c = R.codes(desc)
    return (ctypes.c_int * len(c))(*c)


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def relnorm(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def khp(desc, d, rng):
    """kernel-matrix hp: l_k = 0.75 sqrt(8/d) / sqrt(F) within 5 % for a term of F factors,
    distinct p_k (as tests/test_gpu_periodic.py's khp)."""
    hp, p = [], 0
    for t in R.terms(desc):
        if t == [WN]:
            hp += [0.1]
            continue
        for k in t:
            hp += [1.0 - 0.1 * p] + list(0.75 * np.sqrt(8.0 / d) / np.sqrt(len(t)) * rng.uniform(0.95, 1.05, d))
            if k == PER:
                hp += list(rng.permutation(np.linspace(0.4, 2.0, d)) if d > 1 else [0.9])
            p += 1
    return np.array(hp)


def fit_hp(desc, d, rng):
    return R.model_hp(desc, d, rng, lscale=0.3, noise=0.1)


def assert_well_conditioned(K):
    """the restatement's K: far from diagonal, and factorable (tests/test_gpu_periodic.py)"""
    n = K.shape[0]
    off = K[~np.eye(n, dtype=bool)]
    assert np.median(off) > 0.05, f"median off-diagonal {np.median(off):.3g}: K is nearly diagonal"
    return O.chol_upper(K)


# ---------------------------------------------------------------------------------------
# kernel matrices
# ---------------------------------------------------------------------------------------
KSETS = {
    "SE*PER": [[SE, PER]],
    "SE*PER+WN": [[SE, PER], WN],
    "WN+M52*PER": [WN, [M52, PER]],
    "SE*M32*M52*PER": [[SE, M32, M52, PER]],          # four factors, mixed profiles
    "PER*PER": [[PER, PER]],
    "SEx3+SE*PER+WN": [SE, SE, SE, [SE, PER], WN],    # the term would straddle the group of four
    "(SE*PER)x3+WN": [[SE, PER], [SE, PER], [SE, PER], WN],  # six parts: groups of 4 and 2
}
# as tests/test_gpu_periodic.py: ragged 64-tiles, every compile-time feature width, the run-time-S
# tile (d = 11), de > 32 (d = 17), d > 32, odd leading dimensions (odd n) and even twins
SHAPES = [(1, 1), (63, 2), (65, 3), (130, 8), (98, 10), (70, 11), (66, 17), (66, 33), (2, 1), (64, 2)]
# rtol of a kernel matrix: the project's 1e-13 for every description (a product's relative errors
# add to first order, so F x 1e-13 would be the ceiling for F factors; it is not needed)
K_RTOL = 1e-13


def check_k(got, want, what):
    err = np.max(np.abs(got - want) / (np.abs(want) + 1e-15 / K_RTOL))
    print(f"  {what}: max |K - ref| / (|ref| + atol/rtol) = {err:.2e}")
    np.testing.assert_allclose(got, want, rtol=K_RTOL, atol=1e-15)


@pytest.mark.parametrize("name", list(KSETS))
@pytest.mark.parametrize("n,d", SHAPES)
def test_kernel_matrix(name, n, d):
    desc = KSETS[name]
    rng = np.random.default_rng(n * 31 + d)
    x = rng.random((d, n))
    xp = rng.random((d, 2 * n))
    hp = khp(desc, d, rng)
    cov = cov_of(desc)
    K = G.kernel(cov, hp, x)
    check_k(K, R.kernel(desc, hp, x), f"{name} n={n} d={d} sym")
    assert np.array_equal(K, K.T), "symmetric K must be bitwise symmetric"
    Kx = G.kernel(cov, hp, x, xp)
    assert Kx.shape == (n, 2 * n)
    check_k(Kx, R.kernel(desc, hp, x, xp), "cross")


@pytest.mark.parametrize("name,n,d", [("SE*PER+WN", 130, 4), ("SE*M32*M52*PER", 130, 8),
                                      ("(SE*PER)x3+WN", 70, 11), ("SEx3+SE*PER+WN", 66, 3)])
def test_kernel_matrix_difference_form(name, n, d, knobs):
    """GPR_KBUILD_EXACT=1: the difference of (embedded) features -- the 16-B-store kernels
    (compile-time feature width 8, 16) and the generic ones (more than four parts, width 22)."""
    knobs("GPR_KBUILD_EXACT", 1)
    desc = KSETS[name]
    rng = np.random.default_rng(n + d)
    x, xp = rng.random((d, n)), rng.random((d, n + 6))
    hp = khp(desc, d, rng)
    K = G.kernel(cov_of(desc), hp, x)
    check_k(K, R.kernel(desc, hp, x), f"{name} exact sym")
    assert np.array_equal(K, K.T)
    check_k(G.kernel(cov_of(desc), hp, x, xp), R.kernel(desc, hp, x, xp), "exact cross")


@pytest.mark.parametrize("ldk_extra,off", [(1, 0), (2, 1)])
def test_kernel_matrix_odd_ldk_and_unaligned(ldk_extra, off):
    """An odd leading dimension, and a K that is only 8-byte aligned, at the C ABI: the generic
    difference-form kernel; rows past n of every column stay untouched."""
    desc = KSETS["SE*PER+WN"]
    n, m, d = 130, 70, 8
    rng = np.random.default_rng(77)
    x, xp = rng.random((d, n)), rng.random((d, m))
    hp = khp(desc, d, rng)
    ctx = G.default_context()
    L = G._lib.lib
    ldk = n + ldk_extra
    nk = len(R.codes(desc))
    dx, dxp = ctx.colmajor(x), ctx.colmajor(xp)
    for same, cols, want in ((1, n, R.kernel(desc, hp, x)), (0, m, R.kernel(desc, hp, x, xp))):
        buf = ctx.colmajor(np.full(ldk * cols + 2, -7.0))
        K = buf[off:off + ldk * cols]
        assert (K.data_ptr() % 16 == 0) == (off == 0)
        rc = L.gpr_kernel(ctx.h, karr(desc), nk, _dp(hp), d, _P(dx), n, _P(None if same else dxp),
                          cols, same, 1e-8, _P(K), ldk)
        assert rc == 0, L.gpr_last_error(ctx.h)
        got = ctx.host(buf)[off:off + ldk * cols].reshape(cols, ldk).T
        check_k(got[:n], want, f"ldk={ldk} off={off} same={same}")
        assert np.all(got[n:] == -7.0)
        if same:
            assert np.array_equal(got[:n], got[:n].T)


@pytest.mark.parametrize("d", [1, 3, 8, 33])
def test_se_times_se_is_one_se_on_the_device(d):
    """SE(s1, l1) * SE(s2, l2) against the single SquaredExp(s1 s2, sqrt(l1^2 + l2^2)), both built
    on the device, off the diagonal: rtol 2e-13 (each side within 1e-13 of its restatement)."""
    rng = np.random.default_rng(40 + d)
    n = 130
    x, xp = rng.random((d, n)), rng.random((d, 70))
    hp = khp([[SE, SE]], d, rng)
    h1, h2 = hp[:d + 1], hp[d + 1:]
    one = np.concatenate([[h1[0] * h2[0]], np.sqrt(h1[1:] ** 2 + h2[1:] ** 2)])
    Kp, K1 = G.kernel(G.SquaredExp() * G.SquaredExp(), hp, x), G.kernel(G.SquaredExp(), one, x)
    offd = ~np.eye(n, dtype=bool)
    np.testing.assert_allclose(Kp[offd], K1[offd], rtol=2e-13, atol=0)
    np.testing.assert_allclose(G.kernel(G.SquaredExp() * G.SquaredExp(), hp, x, xp),
                               G.kernel(G.SquaredExp(), one, x, xp), rtol=2e-13, atol=0)


def test_kernel_same_object_forms():
    """eps once per term: GPR_SELF, GPR_SAME_OBJECT and GPR_CROSS with a copy of x."""
    rng = np.random.default_rng(31)
    d, n = 4, 160
    x = rng.random((d, n))
    desc = [[SE, PER], M52, WN, [SE, SE, SE]]
    hp = khp(desc, d, rng)
    cov = cov_of(desc)
    Kself, Ksame, Kcross = G.kernel(cov, hp, x), G.kernel(cov, hp, x, x), G.kernel(cov, hp, x, x.copy())
    check_k(Kself, R.kernel(desc, hp, x), "self")
    check_k(Ksame, R.kernel(desc, hp, x, x), "same object")
    check_k(Kcross, R.kernel(desc, hp, x, x.copy()), "cross")
    np.testing.assert_allclose(np.diag(Ksame) - np.diag(Kcross), 3 * 1e-8, rtol=0, atol=2e-14)


def test_term_table_is_part_of_the_cached_description():
    """At equal hp on one context: SE+PER, SE*PER, SE+PER -- the parameter-block slot of the
    description made last must not serve the next one."""
    rng = np.random.default_rng(3)
    d, n = 3, 70
    x = rng.random((d, n))
    hp = khp([[SE, PER]], d, rng)
    for desc in ([SE, PER], [[SE, PER]], [SE, PER], [[SE, PER]]):
        check_k(G.kernel(cov_of(desc), hp, x), R.kernel(desc, hp, x), str(desc))


def test_kernels_per_summand():
    rng = np.random.default_rng(12)
    d, n = 3, 90
    x = rng.random((d, n))
    desc = [[PER, SE], WN, SE, [M52, M32]]
    hp = khp(desc, d, rng)
    Ks, Kr = G.kernels(cov_of(desc), hp, x), R.kernels(desc, hp, x)
    assert len(Ks) == 4 and Ks[1].shape == (1, 1)
    for a, b in zip(Ks, Kr):
        np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-15)


# ---------------------------------------------------------------------------------------
# dK / dtheta
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SE*PER+WN", "SE*M52"])
@pytest.mark.parametrize("n,d", [(66, 3), (70, 11)])
def test_kernel_grad(name, n, d):
    desc = {"SE*PER+WN": [[SE, PER], WN], "SE*M52": [[SE, M52]]}[name]
    F = 2
    rng = np.random.default_rng(2 + n)
    x = rng.random((d, n))
    hp = khp(desc, d, rng)
    cov = cov_of(desc)
    for i in range(1, len(hp) + 1):
        g, go = G.grad(cov, i, hp, x), R.kernel_grad(desc, i, hp, x)
        if isinstance(go, tuple):
            assert isinstance(g, G.UniformScaling) and g.lam == go[1]
            continue
        np.testing.assert_allclose(g, go, rtol=1e-12 * F, atol=1e-14)


# ---------------------------------------------------------------------------------------
# MLL and the fused gradient
# ---------------------------------------------------------------------------------------
MLL_KSETS = {"SE*PER+WN": [[SE, PER], WN], "SE*M32*M52*PER+WN": [[SE, M32, M52, PER], WN],
             "SEx3+SE*PER+WN": [SE, SE, SE, [SE, PER], WN]}


@functools.lru_cache(maxsize=None)
def _mll_case(name, n, d):
    desc = MLL_KSETS[name]
    rng = np.random.default_rng(n + d)
    x = rng.random((d, n))
    y = np.sum(np.sin(x), axis=0)
    hp = fit_hp(desc, d, rng)
    assert_well_conditioned(R.kernel(desc, hp, x))
    L, g = R.mll(desc, hp, x, y), R.mll_grad(desc, hp, x, y)
    for a in (x, y, hp, g):
        a.setflags(write=False)
    return desc, x, y, hp, L, g


@pytest.mark.parametrize("name", list(MLL_KSETS))
@pytest.mark.parametrize("n,d", [(130, 3), (256, 16), (96, 33)])
def test_mll_and_grad(name, n, d):
    desc, x, y, hp, Lo, go = _mll_case(name, n, d)
    hp = hp.copy()
    md = G.GPRModel(cov_of(desc), hp, x, y.copy())
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
# fit and posterior: n = 256 goes to the tile-DAG directly (SE*PER at d = 8: feature width 16, the
# upper-only build's PROD form + the DAG's mirror), n = 300 on its padded copy
# ---------------------------------------------------------------------------------------
FIT_KSETS = {"SE*PER+WN": [[SE, PER], WN], "SEx3+SE*PER+WN": [SE, SE, SE, [SE, PER], WN]}


@functools.lru_cache(maxsize=None)
def _fit_case(name, n, d=8):
    desc = FIT_KSETS[name]
    m = 70
    x, y, xp = O.synthetic(d, n, m, seed_train=n, seed_test=m)
    hp = fit_hp(desc, d, np.random.default_rng(n + d))
    K = R.kernel(desc, hp, x)
    U = assert_well_conditioned(K)
    mu, var = R.predict(desc, hp, x, y, xp, diagonal_var=True)
    _, S = R.predict(desc, hp, x, y, xp, diagonal_var=False)
    for a in (x, xp, hp, K, U, mu, var, S):
        a.setflags(write=False)
    return desc, d, x, y, xp, hp, K, U, mu, var, S


@pytest.mark.parametrize("name", list(FIT_KSETS))
@pytest.mark.parametrize("n", [256, 300])
def test_predict_vs_restatement(name, n):
    desc, d, x, y, xp, hp, K, U, mu_o, var_o, S_o = _fit_case(name, n)
    md = G.GPRModel(cov_of(desc), hp.copy(), x, y)
    vtol = 1e-8 * R.diag_prior(desc, hp, d)
    mu, var = G.predict(md, xp, diagonal_var=True)
    np.testing.assert_allclose(mu, mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var, var_o, rtol=1e-8, atol=vtol)
    mu2, S = G.predict(md, xp, diagonal_var=False)
    np.testing.assert_allclose(mu2, mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(S, S_o, rtol=1e-8, atol=vtol)
    np.testing.assert_allclose(G.predict_mean(md, xp), mu_o, rtol=1e-8, atol=1e-10)
    for diag in (True, False):  # the same-object rule: eps once per term on Kxp, no noise
        mu_s, S_s = G.predict(md, md.x, diagonal_var=diag)
        mu_so, S_so = R.predict(desc, hp, x, y, x, diagonal_var=diag)
        np.testing.assert_allclose(mu_s, mu_so, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(S_s, S_so, rtol=1e-8, atol=vtol)


@pytest.mark.parametrize("name", list(FIT_KSETS))
@pytest.mark.parametrize("n", [256, 300])
def test_fit_predict(name, n):
    """gpr_fit_predict: K, the factor, alpha and the posterior in one call."""
    desc, d, x, y, xp, hp, K, U, mu_o, var_o, S_o = _fit_case(name, n)
    ctx = G.Context(0)
    L = G._lib.lib
    m = xp.shape[1]
    nk = len(R.codes(desc))
    dx, dy, dxp = ctx.colmajor(x), ctx.colmajor(y), ctx.colmajor(xp)
    dK, alpha, mu, var = ctx.empty(n, n), ctx.empty(n), ctx.empty(m), ctx.empty(m)
    info = ctypes.c_int(-1)
    rc = L.gpr_fit_predict(ctx.h, karr(desc), nk, _dp(hp.copy()), d, _P(dx), n, _P(dy), 1, n,
                           1e-8, _P(dK), n, _P(alpha), _P(dxp), m, G._lib.GPR_PREDICT_DIAG, _P(mu),
                           _P(var), m, _P(None), ctypes.byref(info))
    assert rc == 0 and info.value == 0, L.gpr_last_error(ctx.h)
    np.testing.assert_allclose(ctx.host(mu), mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(ctx.host(var), var_o, rtol=1e-8, atol=1e-8 * R.diag_prior(desc, hp, d))
    ctx.close()


@pytest.mark.parametrize("d", [8, 11])
@pytest.mark.parametrize("n", [256, 300])
def test_fit_leaves_factor_above_and_product_k_below(n, d):
    """gpr_fit of SE*PER+WN: strict lower triangle = the product K, upper = U, alpha = K^-1 y,
    whether the upper-only build and the DAG's mirror made it (d = 8, n = 256) or the full K."""
    desc, d, x, y, xp, hp, K, U, *_ = _fit_case("SE*PER+WN", n, d)
    ctx = G.Context(0)
    L = G._lib.lib
    nk = len(R.codes(desc))
    dx, dy = ctx.colmajor(x), ctx.colmajor(y)
    dK, alpha = ctx.empty(n, n), ctx.empty(n)
    info = ctypes.c_int(-1)
    for _ in range(2):  # (twice on one context: nothing stale from the first call)
        rc = L.gpr_fit(ctx.h, karr(desc), nk, _dp(hp.copy()), d, _P(dx), n, _P(dy), 1, n, 1e-8,
                       _P(dK), n, _P(alpha), ctypes.byref(info))
        assert rc == 0 and info.value == 0, L.gpr_last_error(ctx.h)
        Kd = ctx.host(dK)
        np.testing.assert_allclose(np.tril(Kd, -1), np.tril(K, -1), rtol=1e-13, atol=1e-15)
        assert relnorm(np.triu(Kd), U) < 1e-11
        a_o = O.cho_solve_upper(U, y)
        np.testing.assert_allclose(ctx.host(alpha), a_o, rtol=1e-8, atol=1e-10 * np.abs(a_o).max())
    ctx.close()


# ---------------------------------------------------------------------------------------
# posterior gradients (tolerance of tests/test_gpu_predict_grad.py: 1e-8 normwise per array)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SE*PER+WN", "SE*M52+SE+WN", "SEx3+SE*PER+WN"])
@pytest.mark.parametrize("d", [3, 17])
def test_predict_grad(name, d, knobs):
    """n = 130 with GPR_PGRAD_SLAB = 64: three slabs are summed; two calls agree bit for bit."""
    desc = {"SE*PER+WN": [[SE, PER], WN], "SE*M52+SE+WN": [[SE, M52], SE, WN],
            "SEx3+SE*PER+WN": [SE, SE, SE, [SE, PER], WN]}[name]
    knobs("GPR_PGRAD_SLAB", 64)
    n, m = 130, 70
    rng = np.random.default_rng(1000 * n + 10 * d + len(name))
    x, xp = rng.random((d, n)), rng.random((d, m))
    hp = fit_hp(desc, d, rng)
    y = np.sin(3.0 * x.sum(0)) + 0.1 * rng.standard_normal(n)
    assert_well_conditioned(R.kernel(desc, hp, x))
    gm_o, gv_o = R.posterior_grad(desc, hp, x, y, xp)
    md = G.GPRModel(cov_of(desc), hp, x, y)
    gm, gv = G.predict_grad(md, xp, var=True)
    gm, gv = np.asarray(gm), np.asarray(gv)
    assert gm.shape == gm_o.shape and gv.shape == gv_o.shape
    em, ev = relnorm(gm, gm_o), relnorm(gv, gv_o)
    print(f"{name} d={d}: mean {em:.2e} variance {ev:.2e}")
    assert np.all(np.isfinite(gm)) and np.all(np.isfinite(gv))
    assert em <= 1e-8 and ev <= 1e-8
    gm2, gv2 = G.predict_grad(md, xp, var=True)
    assert np.array_equal(gm, np.asarray(gm2)) and np.array_equal(gv, np.asarray(gv2))


# ---------------------------------------------------------------------------------------
# append, cross-validation, sampling, training
# ---------------------------------------------------------------------------------------
def test_append_three_points():
    """m = 3 points onto a 130-point fit of SE*PER+WN, against a fit on all points
    (tolerances of tests/test_gpu_append.py)."""
    desc = [[SE, PER], WN]
    d, n0, m = 3, 130, 3
    rng = np.random.default_rng(55)
    x = rng.random((d, n0 + m))
    y = np.sin(3.0 * x.sum(0)) + 0.1 * rng.standard_normal(n0 + m)
    hp = fit_hp(desc, d, rng)
    U = assert_well_conditioned(R.kernel(desc, hp, x))
    alpha = O.cho_solve_upper(U, y)
    md = G.GPRModel(cov_of(desc), hp, x[:, :n0].copy(), y[:n0].copy())
    pc = G.GPRPredictCache(md, 0, capacity=n0 + m)
    G.update_predict_cache_(pc, md)
    G.append_(pc, md, x[:, n0:].copy(), y[n0:].copy())
    assert md.n == n0 + m
    ctx = md.ctx
    np.testing.assert_allclose(ctx.host(pc.wt), alpha, **TOL_U)
    np.testing.assert_allclose(np.triu(ctx.host(pc.Kxx)[:n0 + m, :n0 + m]), U, **TOL_U)
    xp = rng.random((d, 17))
    mu_o, var_o = R.predict(desc, hp, x, y, xp, diagonal_var=True)
    mu, var = ctx.empty(17), ctx.empty(17)
    G.predict_(mu, var, md, xp, pc, True)
    np.testing.assert_allclose(ctx.host(mu), mu_o, **TOL_MU)
    np.testing.assert_allclose(ctx.host(var), var_o, rtol=1e-8, atol=1e-8 * R.diag_prior(desc, hp, d))


def test_cv_batch_mse():
    desc = [[SE, PER], WN]
    d, n, k = 3, 200, 50
    x, y, _ = O.synthetic(d, n, 0, seed_train=11)
    hp = fit_hp(desc, d, np.random.default_rng(4))
    md = G.GPRModel(cov_of(desc), hp, x, y)
    cvset = G.kfoldcv(n, k, rng=np.random.default_rng(5))
    got = G.cv_batch(md, G.MSE(), x, y, cvset)
    want = R.cv_batch(desc, hp, "MSE", x, y, cvset)
    np.testing.assert_allclose(got, want, rtol=1e-8)


def test_sample_prior_with_given_z():
    """S = mu + U^T z with U the factor of K' = K + 1e-7 (every element): forward error of a
    backward-stable Cholesky, 8 n u kappa_2(K') ||U||_2 ||Z||_F (tests/test_gpu_sample.py)."""
    desc = [[SE, PER], WN]
    d, n, ns = 2, 200, 3
    rng = np.random.default_rng(17 * n)
    x = rng.random((d, n))
    hp = fit_hp(desc, d, rng)
    z = rng.standard_normal((n, ns))
    Kp = R.kernel(desc, hp, x) + 1e-7
    w = np.linalg.eigvalsh(Kp)
    kappa = w[-1] / w[0]
    assert 0.0 < w[0] and kappa < 1e6, f"kappa_2 = {kappa:.3e}: the bound would be empty"
    bound = 8.0 * n * U53 * kappa * np.sqrt(w[-1]) * np.linalg.norm(z)
    mu = x.sum(axis=0)
    S_ref = np.linalg.cholesky(Kp) @ z + mu[:, None]
    gp = G.GaussianProcess(lambda c: c.sum(), cov_of(desc))
    S = G.sample(gp(x, hp), z=z)
    err = np.linalg.norm(S - S_ref)
    print(f"prior SE*PER+WN n={n}: kappa {kappa:.2e} err {err:.3e} bound {bound:.3e}")
    assert S.shape == (n, ns) and err <= bound


@functools.lru_cache(maxsize=None)
def _train_case():
    """The restatement's optimum in log hp (L-BFGS-B on its MLL and trace-formula gradient)."""
    desc = [[SE, PER], WN]
    d, n = 1, 120
    rng = np.random.default_rng(23)
    x = rng.random((d, n)) * 3.0
    y = np.exp(-0.3 * (x[0] - 1.5) ** 2) * np.sin(2.0 * np.pi * x[0] / 0.8) + 0.1 * rng.standard_normal(n)
    hp0 = np.array([1.0, 0.5, 1.0, 0.7, 0.8, 0.15])

    def fg(t):
        h = np.exp(t)
        return R.mll(desc, h, x, y), R.mll_grad(desc, h, x, y, log_scale=True)

    r = scipy.optimize.minimize(fg, np.log(hp0), jac=True, method="L-BFGS-B",
                                options=dict(maxiter=300, gtol=1e-7, ftol=1e-14))
    return desc, x, y, np.exp(r.x), float(r.fun)


def test_train_reaches_the_restatements_optimum():
    """As tests/test_gpu_periodic.py's: from 3 % beside the restatement's optimum (the period:
    0.3 %) the device's L-BFGS must end at the optimum's VALUE -- the two sigmas of the product are
    identifiable only as their product, so hp itself is not compared.  The flat direction
    (log sigma_1 - log sigma_2) has zero gradient and zero curvature, so L-BFGS neither moves
    along it nor is slowed by it; the bound on the value is that test's: 1e-4 above, and below by
    no more than the restatement's own optimiser left."""
    desc, x, y, hps, Ls = _train_case()
    hp_start = hps * np.array([1.03, 0.97, 0.97, 1.03, 1.003, 1.03])
    md = G.GPRModel(cov_of(desc), hp_start.copy(), x, y)
    hp_tr, res = G.train(md, G.MarginalLikelihood(), np.log(hp_start), method=G.LBFGS(),
                         options=G.Options(g_tol=1e-3, iterations=60))
    assert hp_tr.shape == hps.shape and np.all(np.isfinite(hp_tr)) and np.all(hp_tr > 0)
    L0 = R.mll(desc, hp_start, x, y)
    print(f"L* {Ls:.8f} start {L0:.8f} trained {res.minimum:.8f} hp {hp_tr} hp* {hps}")
    np.testing.assert_allclose(res.minimum, R.mll(desc, hp_tr, x, y), rtol=1e-8)
    assert res.minimum < L0
    assert Ls - 1e-6 * (1.0 + abs(Ls)) <= res.minimum <= Ls + 1e-4


# ---------------------------------------------------------------------------------------
# refusals at the C ABI
# ---------------------------------------------------------------------------------------
def _raw_kernel(codes, hp, d, x):
    ctx = G.default_context()
    L = G._lib.lib
    n = x.shape[1]
    dx = ctx.colmajor(x)
    K = ctx.colmajor(np.full(n * n, -7.0))
    arr = (ctypes.c_int * len(codes))(*codes)
    rc = L.gpr_kernel(ctx.h, arr, len(codes), _dp(hp), d, _P(dx), n, _P(None), n, 1, 1e-8, _P(K), n)
    return rc, L.gpr_last_error(ctx.h).decode(), ctx.host(K)


@pytest.mark.parametrize("codes,code,word", [
    ([MUL, 1, 2], GPR_E_ARG, "kinds[0]"),            # marker first
    ([1, 5, MUL], GPR_E_ARG, "kinds[2]"),            # marker last
    ([1, MUL, MUL, 5], GPR_E_ARG, "kinds[2]"),       # doubled
    ([1, MUL, 2], GPR_E_ARG, "WhiteNoise"),          # beside WhiteNoise
    ([2, MUL, 1], GPR_E_ARG, "WhiteNoise"),
    ([1, MUL, 1, MUL, 3, MUL, 4, MUL, 1, 2], GPR_E_UNSUP, "kinds[8]"),  # a five-factor term
])
def test_bad_descriptions(codes, code, word):
    rng = np.random.default_rng(8)
    d, n = 2, 40
    x = rng.random((d, n))
    hp = np.full(64, 0.7)
    rc, msg, K = _raw_kernel(codes, hp, d, x)
    assert rc == code and msg and word in msg, (rc, msg)
    assert np.all(K == -7.0)
    # and the description next door still works
    rc, msg, K = _raw_kernel([1, MUL, 1, 2], hp, d, x)
    assert rc == 0 and np.all(np.isfinite(K)) and not np.any(K == -7.0), msg


def test_white_noise_factor_and_sum_factor_are_type_errors():
    with pytest.raises(TypeError):
        G.SquaredExp() * G.WhiteNoise()
    with pytest.raises(TypeError, match="not distributed"):
        (G.SquaredExp() + G.Periodic()) * G.Matern32()


def test_refused_calls():
    """The calls built on SquaredExp's separability or its erf integrals refuse a marker:
    GPR_E_UNSUP naming it, outputs untouched."""
    rng = np.random.default_rng(41)
    d, n = 2, 64
    x = rng.random((d, n))
    y = np.sin(x.sum(0))
    desc = [[SE, SE], WN]
    hp = fit_hp(desc, d, rng)
    cov = cov_of(desc)
    md = G.GPRModel(cov, hp, x, y)
    cm = G.Cmap("+", rng.random((d, 5)), rng.random((d, 7)))
    word = "part 2 is a product marker"

    def unsup(e):
        return f"({GPR_E_UNSUP})" in str(e.value) and word in str(e.value)

    with pytest.raises(G.GprError) as e:
        G.predict(md, cm, diagonal_var=True)
    assert unsup(e), str(e.value)
    with pytest.raises(G.GprError) as e:
        G.integrate(md, np.zeros(d), np.ones(d))
    assert unsup(e), str(e.value)
    with pytest.raises(G.GprError) as e:
        G.integrate(md, np.zeros(d), np.ones(d), sample_noise=np.array([0.1]))
    assert unsup(e), str(e.value)
    with pytest.raises(G.GprError) as e:
        G.split_factors(cov, hp, x, cm, part=0)
    assert unsup(e), str(e.value)
    ctx = G.default_context()
    L = G._lib.lib
    nk = len(R.codes(desc))
    bword = word.encode()
    dx, dy, dxe, dxq = ctx.colmajor(x), ctx.colmajor(y), ctx.colmajor(cm.xe), ctx.colmajor(cm.xq)
    seven = lambda s: ctx.colmajor(np.full(s, -7.0))  # noqa: E731
    untouched = lambda *ts: all(np.all(ctx.host(t) == -7.0) for t in ts)  # noqa: E731
    err = lambda: L.gpr_last_error(ctx.h)  # noqa: E731
    A, B, C = seven(5 * 7), seven(5 * n), seven(n * 7)
    rc = L.gpr_split_factors(ctx.h, karr(desc), nk, _dp(hp), d, _P(dx), n, _P(dxe), 5, _P(dxq), 7,
                             0, _P(A), _P(B), _P(C))
    assert rc == GPR_E_UNSUP and bword in err() and untouched(A, B, C)
    dU, wt, mu, var = seven(n * n), seven(n), seven(5 * 7), seven(5 * 7)
    rc = L.gpr_split_predict(ctx.h, karr(desc), nk, _dp(hp), d, _P(dx), n, _P(dU), n, _P(wt),
                             _P(dxe), 5, _P(dxq), 7, 0, 5, 0, 5, 1e-8, _P(mu), _P(var))
    assert rc == GPR_E_UNSUP and bword in err() and untouched(mu, var)
    a, b = np.zeros(d), np.ones(d)
    dK, dwt = seven(n * n), seven(n)
    Iout, ivar = np.full(1, -7.0), np.full(1, -7.0)
    rc = L.gpr_integrate(ctx.h, karr(desc), nk, _dp(hp), d, _P(dx), n, _P(dy), 1, n, _dp(a), _dp(b),
                         1e-8, _P(dK), n, _P(dwt), _dp(Iout), _dp(ivar))
    assert rc == GPR_E_UNSUP and bword in err() and untouched(dK, dwt)
    assert Iout[0] == -7.0 and ivar[0] == -7.0
    noise = np.array([0.1, 0.2])
    Iout, ivar = np.full(2, -7.0), np.full(2, -7.0)
    rc = L.gpr_integrate_noise(ctx.h, karr(desc), nk, _dp(hp), d, _P(dx), n, _P(dy), 1, n, _dp(a),
                               _dp(b), _dp(noise), 1e-8, _dp(Iout), _dp(ivar))
    assert rc == GPR_E_UNSUP and bword in err()
    assert np.all(Iout == -7.0) and np.all(ivar == -7.0)
    from gpr_amd import distributed as Dm
    mg = Dm.MultiGPU([0])
    Dp = ctypes.POINTER(ctypes.c_double)
    c = lambda v: np.ascontiguousarray(v, dtype=np.float64)  # noqa: E731
    X, Xe, Xq = c(x.T), c(cm.xe.T), c(cm.xq.T)
    mu_h, var_h = np.full((7, 5), -7.0), np.full(35, -7.0)
    info = ctypes.c_int(0)
    rc = L.gpr_split_predict_mgpu(mg.h, karr(desc), nk, _dp(hp), d, X.ctypes.data_as(Dp), n, _dp(y),
                                  Xe.ctypes.data_as(Dp), 5, Xq.ctypes.data_as(Dp), 7, 0, 5, 1e-8, 0,
                                  mu_h.ctypes.data_as(Dp), var_h.ctypes.data_as(Dp), ctypes.byref(info))
    assert rc == GPR_E_UNSUP and bword in L.gpr_mgpu_last_error(mg.h)
    assert np.all(mu_h == -7.0) and np.all(var_h == -7.0)
    mg.close()
