"""GPU parity above the old fixed-size envelope: input dimension d > 20 (the run-time-S Gram
tile), d > 32 (the wide MLL gradient), d > 64, and more than 4 SquaredExp parts (part groups),
all against the CPU oracle on seeded inputs.

Inputs as tests/test_gpu_parity.py (x uniform on [0, 1), sigma in U(0.3, 2)) with length-scales
U(0.3, 2) * sqrt(8/d), the scaling of O.default_hp: D = |l .* (x - x')|^2 stays O(1) whatever d
is, so the kernel-matrix bar rtol 1e-13 measures the assembly's rounding ((d + 2) u (|y_a|^2 +
|y_b|^2) for the Gram form, < 1e-14 up to d = 256) and not the conditioning of exp at D ~ 100.

Kernel matrices are built through the C ABI with an even leading dimension (n rounded up to
even) unless a test says otherwise: the Gram kernels store 16-B pairs and decline an odd
leading dimension, so with ld = n the odd sizes would only ever exercise the 8-byte-store
fallback.  On the parent of this file's commit every case with d > 64, every gradient case with
d > 32 and every case with 5 or more SE parts failed with GPR_E_UNSUP.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import gpr_oracle as O

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

SE, WN = O.SE, O.WN
KSETS = {"SE": [SE], "SE+SE+WN": [SE, SE, WN], "WN+SE": [WN, SE], "SE+WN": [SE, WN]}
PARTS = {
    "5SE": [SE] * 5,
    "5SE+WN": [SE] * 5 + [WN],
    "SE+WN+5SE": [SE, WN] + [SE] * 5,
    "8SE": [SE] * 8,
    "9SE+WN": [SE] * 9 + [WN],
}
UNLIMITED = 1 << 30


def cov_of(kinds):
    parts = [G.SquaredExp() if k == SE else G.WhiteNoise() for k in kinds]
    c = parts[0]
    for p in parts[1:]:
        c = c + p
    return c


def hd_hp(kinds, d, rng):
    """sigma, sigma_n ~ U(0.3, 2); length-scales ~ U(0.3, 2) * sqrt(8/d)."""
    out = []
    for k in kinds:
        if k == SE:
            out.append(rng.uniform(0.3, 2.0, 1))
            out.append(rng.uniform(0.3, 2.0, d) * np.sqrt(8.0 / d))
        else:
            out.append(rng.uniform(0.3, 2.0, 1))
    return np.concatenate(out)


def kmat(kinds, hp, x, xp=None, same=None, ld=None):
    """gpr_kernel into a buffer of leading dimension ld (default: n rounded up to even)."""
    ctx = G.default_context()
    lib = G._lib.lib
    dx = ctx.colmajor(x)
    n, d = dx.shape
    if xp is None:
        m, dxp = n, None
        same = G._lib.GPR_SELF if same is None else same
    else:
        dxp = ctx.colmajor(xp)
        m, same = dxp.shape[0], G._lib.GPR_CROSS
    ld = n + (n & 1) if ld is None else ld
    buf = ctx.zeros(m, ld)
    kc = (ctypes.c_int * len(kinds))(*[1 if k == SE else 2 for k in kinds])
    hpa = np.ascontiguousarray(hp, dtype=np.float64)
    rc = lib.gpr_kernel(ctx.h, kc, len(kinds), hpa.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                        d, ctypes.c_void_p(dx.data_ptr()), n,
                        ctypes.c_void_p(dxp.data_ptr() if dxp is not None else 0), m, same, 1e-8,
                        ctypes.c_void_p(buf.data_ptr()), ld)
    ctx.check(rc, "gpr_kernel")
    return ctx.host(buf)[:n, :]


@functools.lru_cache(maxsize=None)
def kcase(name, n, d):
    """Seeded inputs and the oracle's matrices of one (kinds, n, d) case, computed once."""
    kinds = (KSETS.get(name) or PARTS[name])
    rng = np.random.default_rng(1000 * d + n + len(kinds))
    x, xp = rng.random((d, n)), rng.random((d, 2 * n))
    hp = hd_hp(kinds, d, rng)
    ref = {"sym": O.kernel(kinds, hp, x), "cross": O.kernel(kinds, hp, x, xp),
           "same": O.kernel(kinds, hp, x, x)}
    for a in (x, xp, hp, *ref.values()):
        a.setflags(write=False)
    return kinds, x, xp, hp, ref


def check_k(name, n, d, **kw):
    kinds, x, xp, hp, ref = kcase(name, n, d)
    K = kmat(kinds, hp, x, **kw)
    np.testing.assert_allclose(K, ref["sym"], rtol=1e-13, atol=1e-15)
    assert np.array_equal(K, K.T), "symmetric K must be bitwise symmetric"
    Kx = kmat(kinds, hp, x, xp, **kw)
    assert Kx.shape == (n, 2 * n)
    np.testing.assert_allclose(Kx, ref["cross"], rtol=1e-13, atol=1e-15)
    # the same-object form (predict(md, md.x)'s kernel): eps per SE part, no noise
    Ks = kmat(kinds, hp, x, same=G._lib.GPR_SAME_OBJECT, **kw)
    np.testing.assert_allclose(Ks, ref["same"], rtol=1e-13, atol=1e-15)
    assert np.array_equal(Ks, Ks.T)


# d = 21: first d past the compiled Gram range; 33, 65: a one-dimension last k-step; 100: a
# ragged last chunk of k-steps; n = 65, 97, 130, 257: ragged 64-tiles
HD_CASES = [(65, 21), (130, 24), (130, 32), (257, 33), (130, 64), (130, 65), (97, 100)]


@pytest.mark.parametrize("name", ["SE", "SE+SE+WN", "WN+SE"])
@pytest.mark.parametrize("n,d", HD_CASES)
def test_kernel_matrix_high_d(name, n, d):
    check_k(name, n, d)


@pytest.mark.parametrize("name", ["SE", "SE+SE+WN", "WN+SE"])
@pytest.mark.parametrize("n,d", [(130, 24), (130, 32)])
@pytest.mark.parametrize("maxd", [20, UNLIMITED])
def test_kernel_matrix_both_sides_of_dispatch(name, n, d, maxd, knobs):
    """GPR_KBUILD_GRAM_MAXD = 20 (the difference form above d = 20) and unlimited (the Gram form
    at every d) both match the oracle, whatever the knob's default is."""
    knobs("GPR_KBUILD_GRAM_MAXD", maxd)
    check_k(name, n, d)


def test_gram_maxd_knob_is_registered():
    ctx = G.default_context()
    old = ctx.get_knob("GPR_KBUILD_GRAM_MAXD")
    assert old >= 20
    ctx.set_knob("GPR_KBUILD_GRAM_MAXD", 20)
    assert ctx.get_knob("GPR_KBUILD_GRAM_MAXD") == 20
    ctx.set_knob("GPR_KBUILD_GRAM_MAXD", old)


@pytest.mark.parametrize("name", ["SE", "SE+SE+WN"])
def test_kernel_matrix_odd_leading_dimension_d65(name):
    """An odd leading dimension keeps the 8-byte-store kernels (the 16-B pairs need an even one)."""
    check_k(name, 130, 65, ld=131)


@pytest.mark.parametrize("name", ["SE", "SE+SE+WN"])
def test_kernel_matrix_exact_form_d65(name, knobs):
    knobs("GPR_KBUILD_EXACT", 1)
    check_k(name, 130, 65)


def test_kernel_python_surface_d65():
    """G.kernel (leading dimension n) at d = 65, the three forms."""
    kinds, x, xp, hp, ref = kcase("SE+SE+WN", 130, 65)
    cov = cov_of(kinds)
    np.testing.assert_allclose(G.kernel(cov, hp, x), ref["sym"], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(G.kernel(cov, hp, x, xp), ref["cross"], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(G.kernel(cov, hp, x, x), ref["same"], rtol=1e-13, atol=1e-15)


# ---- more than four SE parts: groups of four ---------------------------------------------
@pytest.mark.parametrize("name", list(PARTS))
@pytest.mark.parametrize("d", [3, 33])
def test_part_groups(name, d):
    n = 130
    check_k(name, n, d)
    kinds, x, _, hp, ref = kcase(name, n, d)
    cov = cov_of(kinds)
    K = G.kernel(cov, hp, x)
    np.testing.assert_allclose(K, ref["sym"], rtol=1e-13, atol=1e-15)
    # K = sum of kernels() per part (each with its eps) + sigma_n^2 of the first WhiteNoise
    Ks = G.kernels(cov, hp, x)
    assert len(Ks) == len(kinds)
    tot = np.zeros((n, n))
    off, noise2 = 0, None
    for k, Kp in zip(kinds, Ks):
        if k == SE:
            tot = tot + Kp
            off += d + 1
        else:
            assert Kp.shape == (1, 1)
            noise2 = hp[off] ** 2 if noise2 is None else noise2
            off += 1
    if noise2 is not None:
        tot = tot + noise2 * np.eye(n)
    np.testing.assert_allclose(K, tot, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("name", ["5SE+WN", "9SE+WN"])
def test_part_groups_exact_form_and_odd_ld(name, knobs):
    """The fallbacks take every part in one launch: the difference form (compiled d = 3, where
    the 16-B-store kernels' LDS tables hold four parts only) and the 8-byte-store kernels."""
    check_k(name, 130, 3, ld=131)
    knobs("GPR_KBUILD_EXACT", 1)
    check_k(name, 130, 3)
    check_k(name, 130, 33)


# ---- dK/dtheta ---------------------------------------------------------------------------
@pytest.mark.parametrize("kinds,d", [([SE], 65), ([SE] * 6, 3), ([SE, WN] + [SE] * 4 + [WN, SE], 33)])
def test_kernel_grad_high_d_and_parts(kinds, d):
    rng = np.random.default_rng(17 + d)
    n = 100
    x = rng.random((d, n))
    hp = hd_hp(kinds, d, rng)
    cov = cov_of(kinds)
    D = len(hp)
    last = D - d  # 1-based index of the last part's sigma (the last part is an SE here)
    for i in (last, last + 1 + d // 2, D):
        g = G.grad(cov, i, hp, x)
        go = O.kernel_grad(kinds, i, hp, x)
        np.testing.assert_allclose(g, go, rtol=1e-12, atol=1e-14)
    g1 = G.grad(cov, 1, hp, x)
    np.testing.assert_allclose(g1, O.kernel_grad(kinds, 1, hp, x), rtol=1e-12, atol=1e-14)


# ---- MLL value and gradient --------------------------------------------------------------
def mll_problem(kinds, n, d):
    rng = np.random.default_rng(7 * n + d + len(kinds))
    x = rng.random((d, n))
    y = np.sum(np.sin(x), axis=0)
    return x, y, hd_hp(kinds, d, rng)


@pytest.mark.parametrize("kinds,n,d", [
    ([SE, WN], 100, 33), ([SE, WN], 130, 64), ([SE, WN], 130, 65), ([SE, WN], 100, 100),
    ([SE, SE, WN], 100, 33), ([SE] * 5 + [WN], 100, 5)])
def test_mll_value_and_grad(kinds, n, d):
    x, y, hp = mll_problem(kinds, n, d)
    md = G.GPRModel(cov_of(kinds), hp, x, y)
    L = G.loss(G.MarginalLikelihood(), hp, md)
    assert L == pytest.approx(O.mll(kinds, hp, x, y), rel=1e-10)
    g = G.grad(G.MarginalLikelihood(), hp, md)
    go = O.mll_grad(kinds, hp, x, y)
    np.testing.assert_allclose(g, go, rtol=1e-8, atol=1e-8 * (1 + np.abs(go).max()))


@pytest.mark.parametrize("kinds,d", [([SE, WN], 33), ([SE] * 5 + [WN], 33)])
def test_log_loss_grad_d33(kinds, d):
    n = 100
    x, y, hp = mll_problem(kinds, n, d)
    md = G.GPRModel(cov_of(kinds), hp, x, y)
    tc = G.MllGradCache(md)
    Gv = np.zeros(len(hp))
    F = G.log_loss_grad_(G.MarginalLikelihood(), 0.0, Gv, np.log(hp), md, tc)
    assert F == pytest.approx(O.mll(kinds, hp, x, y), rel=1e-10)
    go = O.mll_grad(kinds, hp, x, y, log_scale=True)
    np.testing.assert_allclose(Gv, go, rtol=1e-8, atol=1e-8 * (1 + np.abs(go).max()))


# ---- the callers around the path at d = 65 -----------------------------------------------
def test_predict_d65():
    kinds, d, n, m = [SE, WN], 65, 200, 77
    x, y, xp = O.synthetic(d, n, m, seed_train=n, seed_test=m)
    hp = O.default_hp(kinds, d, noise=0.05)
    md = G.GPRModel(cov_of(kinds), hp, x, y)
    vtol = 1e-8 * O.diag_prior(kinds, hp, d)
    mu, var = G.predict(md, xp, diagonal_var=True)
    mu_o, var_o = O.predict(kinds, hp, x, y, xp, diagonal_var=True)
    np.testing.assert_allclose(mu, mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var, var_o, rtol=1e-8, atol=vtol)
    mu2, S = G.predict(md, xp, diagonal_var=False)
    _, S_o = O.predict(kinds, hp, x, y, xp, diagonal_var=False)
    np.testing.assert_allclose(mu2, mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(S, S_o, rtol=1e-8, atol=vtol)
    mu3, S3 = G.predict(md, md.x, diagonal_var=True)
    mu3_o, S3_o = O.predict(kinds, hp, x, y, x, diagonal_var=True)
    np.testing.assert_allclose(mu3, mu3_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(S3, S3_o, rtol=1e-8, atol=vtol)


@pytest.mark.parametrize("kinds", [[SE, WN], [SE] * 5 + [WN]])
def test_split_predict_d65(kinds):
    d, n, ne, nq = 65, 200, 12, 9
    rng = np.random.default_rng(d * 7 + n + ne + nq)
    x, xe, xq = rng.random((d, n)), 0.5 * rng.random((d, ne)), 0.5 * rng.random((d, nq))
    y = np.sin(x.sum(0)) ** 2
    hp = O.default_hp(kinds, d, noise=0.05)
    md = G.GPRModel(cov_of(kinds), hp, x, y)
    yps, varps = G.predict(md, G.Cmap("+", xe, xq), diagonal_var=True, var_range=(1, 3))
    mu_o, var_o = O.split_predict(kinds, hp, x, y, xe, xq, var_range=(1, 3))
    np.testing.assert_allclose(yps, mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(varps, var_o, rtol=1e-8, atol=1e-8 * O.diag_prior(kinds, hp, d))


def test_cv_batch_d65():
    kinds, d, n, k = [SE, WN], 65, 200, 20
    rng = np.random.default_rng(65)
    x = rng.random((d, n))
    y = np.sin(x.sum(axis=0)) ** 2
    hp = O.default_hp(kinds, d)
    md = G.GPRModel(cov_of(kinds), hp, x, y)
    cvset = G.kfoldcv(n, k, rng=np.random.default_rng(5))
    got = G.cv_batch(md, G.MSE(), x, y, cvset)
    np.testing.assert_allclose(got, O.cv_batch(kinds, hp, "MSE", x, y, cvset), rtol=1e-8, atol=0)


def test_integrate_d65():
    kinds, d, n = [SE, WN], 65, 200
    x, y, _ = O.synthetic(d, n, 0, seed_train=n)
    hp = O.default_hp(kinds, d, noise=0.05)
    Y = np.stack([y, np.cos(x.sum(0))], axis=1)
    md = G.GPRModel(cov_of(kinds), hp, x, Y)
    a, b = np.full(d, 0.1), np.full(d, 0.8)
    k1 = G.antideriv(G.SquaredExp(), x, hp[:d + 1], a, b)
    np.testing.assert_allclose(k1, O.antideriv_se(x, hp[:d + 1], a, b), rtol=1e-12, atol=1e-300)
    I, v = G.integrate(md, a, b)
    Io, vo = O.integrate(kinds, hp, x, Y, a, b)
    np.testing.assert_allclose(I, Io, rtol=1e-8, atol=1e-12)
    assert v[0] == pytest.approx(vo, rel=1e-8, abs=1e-10 * O.antideriv2_se(hp, a, b))


def test_train_d33():
    """A handful of iterations at d = 33: the loss does not rise, and the device gradient at the
    returned point is the oracle's."""
    kinds, d, n = [SE, WN], 33, 120
    rng = np.random.default_rng(33)
    x = rng.random((d, n))
    y = np.sum(np.sin(x), axis=0)
    hp0 = O.default_hp(kinds, d)
    md = G.GPRModel(cov_of(kinds), hp0, x, y)
    L0 = G.loss(G.MarginalLikelihood(), hp0, md)
    hp_tr, res = G.train(md, G.MarginalLikelihood(), hp0, method=G.LBFGS(),
                         options=G.Options(g_tol=1e-2, iterations=5))
    assert np.isfinite(res.minimum) and res.minimum <= L0 * (1 + 1e-12) + 1e-12
    np.testing.assert_allclose(res.minimum, O.mll(kinds, hp_tr, x, y), rtol=1e-8)
    g = G.grad(G.MarginalLikelihood(), hp_tr, md)
    go = O.mll_grad(kinds, hp_tr, x, y)
    np.testing.assert_allclose(g, go, rtol=1e-8, atol=1e-8 * (1 + np.abs(go).max()))
