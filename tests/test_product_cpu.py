"""CPU: product kernels (`*`) restated in NumPy, and the description plumbing.

A kernel is a sum of terms; a term is one WhiteNoise or a product of 1..4 stationary factors.  A
description here is a list of terms in `+` order, a term being a kind (one factor) or a list of
kinds (its factors in `*` order): `[[SE, PER], WN]` is `SE * PER + WN`.  The per-factor functions
are those of tests/test_periodic_cpu.py (difference form, feature by feature); this file only
restates what is done with their values, as include/gpr_hip.h defines it:

    k_f = sigma_f^2 f_f(D_f)                 the factor's value, without eps
    T   = prod_f k_f  (+ eps once per term on a same-object diagonal)
    K   = sum of the terms in order (+ sigma_n^2 of the first WhiteNoise in the 4-arg form)
    dK/dsigma_f = (2/|sigma_f|) T            (T with its eps)
    dK/dl_k, dK/dp_k of factor f: that factor's own formula with W_f C_f for W_f,
    C_f = prod_{g != f} k_g, formed as a product
    diagonal-variance prior: sum over terms of prod_f sigma_f^2 (WhiteNoise: sigma_n^2)

hp is the concatenation of the factors' own layouts in order, so a product of F factors has F
sigmas of which only the product is identifiable.  A description without a product must equal
tests/test_periodic_cpu.py bit for bit.  tests/test_gpu_product.py imports this restatement.
"""
import numpy as np
import pytest

import test_periodic_cpu as P
from oracle import gpr_oracle as O
from test_periodic_cpu import M32, M52, PER, SE, WN

EPS = 1e-8
MUL_CODE = 6
KMAXP = 4


# ---------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------
def terms(desc):
    return [list(t) if isinstance(t, (list, tuple)) else [t] for t in desc]


def flat(desc):
    """the factors in hp order"""
    return [f for t in terms(desc) for f in t]


def codes(desc):
    """kinds[] of the C ABI: the factors of a term joined by the marker"""
    out = []
    for t in terms(desc):
        for j, f in enumerate(t):
            out += ([MUL_CODE] if j else []) + [P.KIND_CODE[f]]
    return out


def has_product(desc):
    return any(len(t) > 1 for t in terms(desc))


def term_hps(desc, hp, d):
    """per term the list of its factors' hp vectors"""
    hps = P.split_hp(flat(desc), hp, d)
    out, c = [], 0
    for t in terms(desc):
        out.append(hps[c:c + len(t)])
        c += len(t)
    return out


def term_kernel(t, hps, x, xq, same, eps=EPS):
    if len(t) == 1:
        return P.part_kernel(t[0], hps[0], x, xq, same, eps)
    K = P.part_kernel(t[0], hps[0], x, xq, False, eps)
    for f, h in zip(t[1:], hps[1:]):
        K = K * P.part_kernel(f, h, x, xq, False, eps)
    if same:
        K[np.diag_indices(K.shape[0])] += eps
    return K


def kernel(desc, hp, x, xp=None, eps=EPS):
    d = x.shape[0]
    noise = xp is None
    same = noise or xp is x
    xq = x if same else xp
    ts, hps = terms(desc), term_hps(desc, hp, d)
    st = [i for i, t in enumerate(ts) if t != [WN]]
    assert st, "kernel needs at least one stationary part"
    K = term_kernel(ts[st[0]], hps[st[0]], x, xq, same, eps)
    for i in st[1:]:
        K = K + term_kernel(ts[i], hps[i], x, xq, same, eps)
    if noise and [WN] in ts:
        K[np.diag_indices(K.shape[0])] += hps[ts.index([WN])][0][0] ** 2
    return K


def kernels(desc, hp, x, eps=EPS):
    """one matrix per summand, a 1 x 1 zero for WhiteNoise"""
    return [np.zeros((1, 1)) if t == [WN] else term_kernel(t, h, x, x, True, eps)
            for t, h in zip(terms(desc), term_hps(desc, hp, x.shape[0]))]


def kernel_grad(desc, i, hp, x, eps=EPS):
    """1-based i; WhiteNoise -> ("I", 2 sigma_n)."""
    d = x.shape[0]
    fl = flat(desc)
    hps = P.split_hp(fl, hp, d)
    kidx, hpidx = P.find_idx(fl, i, d)
    part, kind = hps[kidx], fl[kidx]
    if kind == WN:
        return ("I", 2.0 * part[0])
    # the term that owns factor kidx, and the product C of its other factors (None: no other)
    c, C = 0, None
    for t in terms(desc):
        if c <= kidx < c + len(t):
            for g in range(c, c + len(t)):
                if g != kidx:
                    Kg = P.part_kernel(fl[g], hps[g], x, x, False, eps)
                    C = Kg if C is None else C * Kg
            break
        c += len(t)
    Kf, W = P.part_kernel(kind, part, x, x, C is None, eps, want_w=True)
    if C is not None:
        Kf = Kf * C
        Kf[np.diag_indices(Kf.shape[0])] += eps
        W = W * C
    if hpidx == 1:
        return (2.0 / abs(part[0])) * Kf
    k = (hpidx - 2) % d
    r = x[k][:, None] - x[k][None, :]
    if kind != PER:
        return -2.0 * part[hpidx - 1] * W * r ** 2
    l, p = part[1 + k], part[1 + d + k]
    if hpidx <= d + 1:
        return -2.0 * l * W * (2.0 * np.sin(np.pi * r / p)) ** 2
    return (4.0 * np.pi * l * l / (p * p)) * W * r * np.sin(2.0 * np.pi * r / p)


def mll(desc, hp, x, y, eps=EPS):
    U = O.chol_upper(kernel(desc, hp, x, None, eps))
    return O.mll_value(U, y, O.cho_solve_upper(U, y))


def mll_grad(desc, hp, x, y, eps=EPS, log_scale=False):
    hp = np.asarray(hp, dtype=np.float64)
    U = O.chol_upper(kernel(desc, hp, x, None, eps))
    alpha = O.cho_solve_upper(U, y)
    Kinv = O.kinv_from_upper(U)
    g = np.array([O.mll_grad_term(kernel_grad(desc, i, hp, x, eps), alpha, Kinv)
                  for i in range(1, len(hp) + 1)])
    return g * hp if log_scale else g


def diag_prior(desc, hp, d):
    ths = term_hps(desc, hp, d)
    if len(flat(desc)) == 1:
        return float(ths[0][0][0] ** 2)
    out = []
    for hs in ths:
        v = hs[0][0] ** 2
        for h in hs[1:]:
            v = v * h[0] ** 2
        out.append(v)
    return float(sum(out))


def predict(desc, hp, x, y, xp, diagonal_var=False, eps=EPS):
    import scipy.linalg as sla
    U = O.chol_upper(kernel(desc, hp, x, None, eps))
    wt = O.cho_solve_upper(U, y)
    Kxp = kernel(desc, hp, xp, x, eps)
    mu = Kxp @ wt
    V = sla.solve_triangular(U, Kxp.T, trans="T", lower=False, check_finite=False).T
    if diagonal_var:
        return mu, diag_prior(desc, hp, x.shape[0]) - np.sum(V * V, axis=1)
    return mu, kernel(desc, hp, xp, None, eps) - V @ V.T


def posterior_grad(desc, hp, x, y, xp, eps=EPS):
    """(gm, gv) as test_predict_grad_cpu.posterior_grad: dk/dx*_k of a term is the sum over its
    factors of -W_f C_f dD_f/dx*_k."""
    d, m = x.shape[0], xp.shape[1]
    U = O.chol_upper(kernel(desc, hp, x, None, eps))
    alpha = O.cho_solve_upper(U, y)
    Q = O.cho_solve_upper(U, kernel(desc, hp, x, np.array(xp), eps))  # (a copy: never `xp is x`)
    A = alpha.T if alpha.ndim == 2 else alpha[None, :]
    gm, gv = np.zeros((A.shape[0], d, m)), np.zeros((d, m))
    for t, hs in zip(terms(desc), term_hps(desc, hp, d)):
        if t == [WN]:
            continue
        KW = [P.part_kernel(f, h, x, xp, False, eps, want_w=True) for f, h in zip(t, hs)]
        for fi, (kind, h) in enumerate(zip(t, hs)):
            W = KW[fi][1]
            for gi in range(len(t)):
                if gi != fi:
                    W = W * KW[gi][0]
            for k in range(d):
                r = xp[k][None, :] - x[k][:, None]
                l = h[1 + k]
                if kind == PER:
                    p = h[1 + d + k]
                    dD = (4.0 * np.pi * l * l / p) * np.sin(2.0 * np.pi * r / p)
                else:
                    dD = 2.0 * l * l * r
                T = -W * dD
                gm[:, k, :] += A @ T
                gv[k] += -2.0 * np.sum(Q * T, axis=0)
    return (gm if alpha.ndim == 2 else gm[0]), gv


def cv_batch(desc, hp, cost, x, y, cvset, eps=EPS):
    out = []
    for a, b in zip(*cvset):
        yp, S = predict(desc, hp, x[:, a], y[a], x[:, b], diagonal_var=False, eps=eps)
        out.append(O.cv_loss(cost, y[b], yp, S))
    return np.array(out)


def model_hp(desc, d, rng, lscale=0.75, noise=0.1):
    """As test_periodic_cpu.model_hp, with the length-scale multipliers of a term of F factors
    divided by sqrt(F): the product's exponent sum_f D_f then stays the size of one part's."""
    hp, p = [], 0
    for t in terms(desc):
        if t == [WN]:
            hp += [noise]
            continue
        for k in t:
            hp += [1.0 - 0.1 * p] + list(lscale * np.sqrt(8.0 / d) / np.sqrt(len(t)) * (1.0 + 0.2 * p)
                                         * rng.uniform(0.9, 1.1, d))
            if k == PER:
                hp += list(rng.permutation(np.linspace(0.4, 2.0, d + 2)[1:-1]) if d > 1 else [0.9])
            p += 1
    return np.array(hp)


def cov_of(desc):
    """the Python kernel object of a description"""
    import gpr_amd as G
    cls = {SE: G.SquaredExp, WN: G.WhiteNoise, M32: G.Matern32, M52: G.Matern52, PER: G.Periodic}
    c = None
    for t in terms(desc):
        k = cls[t[0]]()
        for f in t[1:]:
            k = k * cls[f]()
        c = k if c is None else c + k
    return c


# ---------------------------------------------------------------------------------------
# the restatement's own checks
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [[SE], [PER, WN], [WN, M52], [SE, PER, WN, M32], [SE, SE, SE, SE, PER, WN]])
def test_equals_the_periodic_restatement_without_a_product(kinds):
    rng = np.random.default_rng(len(kinds))
    d, n, m = 3, 40, 17
    x, xp = rng.random((d, n)), rng.random((d, m))
    y = np.sin(x.sum(0)) ** 2
    hp = P.model_hp(kinds, d, rng, lscale=0.3)
    assert np.array_equal(model_hp(kinds, d, np.random.default_rng(3)), P.model_hp(kinds, d, np.random.default_rng(3)))
    assert codes(kinds) == [P.KIND_CODE[k] for k in kinds] and not has_product(kinds)
    assert np.array_equal(kernel(kinds, hp, x), P.kernel(kinds, hp, x))
    assert np.array_equal(kernel(kinds, hp, x, x), P.kernel(kinds, hp, x, x))
    assert np.array_equal(kernel(kinds, hp, x, xp), P.kernel(kinds, hp, x, xp))
    for a, b in zip(kernels(kinds, hp, x), P.kernels(kinds, hp, x)):
        assert np.array_equal(a, b)
    for i in range(1, len(hp) + 1):
        a, b = kernel_grad(kinds, i, hp, x), P.kernel_grad(kinds, i, hp, x)
        assert a == b if isinstance(a, tuple) else np.array_equal(a, b)
    assert diag_prior(kinds, hp, d) == P.diag_prior(kinds, hp, d)
    if WN not in kinds:
        return
    assert mll(kinds, hp, x, y) == P.mll(kinds, hp, x, y)
    for log in (False, True):
        assert np.array_equal(mll_grad(kinds, hp, x, y, log_scale=log), P.mll_grad(kinds, hp, x, y, log_scale=log))
    for diag in (True, False):
        for got, want in zip(predict(kinds, hp, x, y, xp, diag), P.predict(kinds, hp, x, y, xp, diag)):
            assert np.array_equal(got, want)


@pytest.mark.parametrize("d", [1, 3, 8])
def test_kernel_grad_by_central_differences(d):
    """Every hyper-parameter of SE*PER+WN+M52*M32*SE against (K(h+) - K(h-)) / 2h, h = 1e-6, in
    the manner and at the bound (1e-8) of test_periodic_cpu.test_kernel_grad_by_central_differences:
    a product's third derivatives are sums of products of its factors' derivatives, each factor
    <= 1, and the length-scale multipliers are divided by sqrt(F), so the truncation h^2 |K'''| / 6
    stays below that file's 2e-9."""
    rng = np.random.default_rng(5 + d)
    n, h = 40, 1e-6
    x = rng.random((d, n))
    desc = [[SE, PER], WN, [M52, M32, SE]]
    hp = model_hp(desc, d, rng, lscale=0.5)
    fl = flat(desc)
    for i in range(1, len(hp) + 1):
        ga = kernel_grad(desc, i, hp, x)
        if isinstance(ga, tuple):
            continue
        e = np.zeros(len(hp))
        e[i - 1] = h
        fd = (kernel(desc, hp + e, x) - kernel(desc, hp - e, x)) / (2.0 * h)
        kidx, hpidx = P.find_idx(fl, i, d)
        if hpidx == 1:  # the rule's T carries eps on the diagonal, which no derivative of K has
            fd[np.diag_indices(n)] += (2.0 / abs(hp[i - 1])) * EPS
        err = np.abs(ga - fd).max()
        print(f"d={d} hp index {i} ({fl[kidx]}): max |analytic - FD| = {err:.2e}")
        assert err <= 1e-8


def test_mll_grad_by_central_differences():
    """The trace-formula gradient of descriptions with products against differences of the MLL,
    at the tolerance of test_periodic_cpu.test_mll_grad_by_central_differences."""
    rng = np.random.default_rng(9)
    d, n, h = 2, 50, 1e-6
    x = rng.random((d, n))
    y = np.sin(x.sum(0)) ** 2
    for desc in ([[SE, PER], WN, M52], [[SE, M32, M52, PER], WN]):
        hp = model_hp(desc, d, rng, lscale=0.3, noise=0.3)
        g = mll_grad(desc, hp, x, y)
        for i in range(len(hp)):
            e = np.zeros(len(hp))
            e[i] = h
            fd = (mll(desc, hp + e, x, y) - mll(desc, hp - e, x, y)) / (2.0 * h)
            # u |MLL| / h ~ 1e-8 rounding of the quotient: 1e-6 of the gradient's scale
            assert abs(g[i] - fd) <= 1e-6 * (1.0 + np.abs(g).max())


def test_posterior_grad_by_central_differences():
    """As test_predict_grad_cpu.test_restatement_by_central_differences (h = 1e-5, 1e-6 normwise),
    and equal to that file's restatement without a product."""
    import test_predict_grad_cpu as PG
    rng = np.random.default_rng(133)
    n, d, m = 130, 3, 37
    x, xp = rng.random((d, n)), rng.random((d, m))
    y = np.sin(3.0 * x.sum(0)) + 0.1 * rng.standard_normal(n)
    desc = [[SE, PER], M52, [M32, SE, PER], WN]
    hp = model_hp(desc, d, rng, lscale=0.3, noise=0.1)
    gm, gv = posterior_grad(desc, hp, x, y, xp)
    fm, fv = PG.central_differences(predict, desc, hp, x, y, xp)
    em, ev = PG.relnorm(gm, fm), PG.relnorm(gv, fv)
    print(f"mean {em:.2e} variance {ev:.2e}")
    assert em <= 1e-6 and ev <= 1e-6
    kinds = [SE, PER, M52, WN]
    hp = P.model_hp(kinds, d, rng, lscale=0.3)
    for a, b in zip(posterior_grad(kinds, hp, x, y, xp), PG.posterior_grad(kinds, hp, x, y, xp)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("d", [1, 3, 8, 33])
def test_se_times_se_is_one_se(d):
    """SE(s1, l1) * SE(s2, l2) = SE(s1 s2, sqrt(l1^2 + l2^2)) off the diagonal (on it the product
    carries one eps and so does the single part: equal there too).  Both sides round D <= 2 sum
    (l1^2 + l2^2) ~ 20 feature by feature: (d + 2) u D each, asserted at rtol 2e-13."""
    rng = np.random.default_rng(d)
    n, m = 50, 30
    x, xp = rng.random((d, n)), rng.random((d, m))
    hp = model_hp([[SE, SE]], d, rng)
    h1, h2 = hp[:d + 1], hp[d + 1:]
    one = np.concatenate([[h1[0] * h2[0]], np.sqrt(h1[1:] ** 2 + h2[1:] ** 2)])
    np.testing.assert_allclose(kernel([[SE, SE]], hp, x, xp), P.kernel([SE], one, x, xp), rtol=2e-13, atol=0)
    np.testing.assert_allclose(kernel([[SE, SE]], hp, x), P.kernel([SE], one, x), rtol=2e-13, atol=0)


def test_product_kernel_is_symmetric_positive_definite():
    """Schur product theorem: the elementwise product of two PSD matrices is PSD."""
    rng = np.random.default_rng(6)
    d, n = 2, 120
    x = rng.random((d, n))
    K = kernel([[SE, PER]], model_hp([[SE, PER]], d, rng, lscale=0.3), x)
    assert np.array_equal(K, K.T)
    assert np.linalg.eigvalsh(K)[0] > 0.0


def test_eps_once_per_term_and_prior():
    rng = np.random.default_rng(2)
    d, n = 2, 30
    x = rng.random((d, n))
    desc = [[SE, PER], M52, WN, [SE, SE, SE]]
    hp = model_hp(desc, d, rng)
    Kself, Ksame, Kcross = kernel(desc, hp, x), kernel(desc, hp, x, x), kernel(desc, hp, x, x.copy())
    np.testing.assert_allclose(np.diag(Ksame) - np.diag(Kcross), 3 * EPS, rtol=0, atol=2e-15)
    hs = P.split_hp(flat(desc), hp, d)
    np.testing.assert_allclose(np.diag(Kself) - np.diag(Ksame), hs[3][0] ** 2, rtol=1e-12)
    want = (hs[0][0] * hs[1][0]) ** 2 + hs[2][0] ** 2 + hs[3][0] ** 2 + (hs[4][0] * hs[5][0] * hs[6][0]) ** 2
    np.testing.assert_allclose(diag_prior(desc, hp, d), want, rtol=1e-15)
    np.testing.assert_allclose(np.diag(Kcross), want - hs[3][0] ** 2, rtol=1e-14)


# ---------------------------------------------------------------------------------------
# the Python description plumbing (no device)
# ---------------------------------------------------------------------------------------
def test_package_exports_the_product():
    import gpr_amd as G
    from gpr_amd import _lib as L
    assert hasattr(G, "ProductKernel") and "ProductKernel" in G.__all__
    assert L.GPR_MUL == MUL_CODE
    assert "#define GPR_MUL 6" in open(L.HEADER).read()
    assert G.is_stationary(G.SquaredExp() * G.Periodic()) is True


def test_multiplication_builds_flat_products():
    import gpr_amd as G
    se, per, m32, m52, wn = G.SquaredExp(), G.Periodic(), G.Matern32(), G.Matern52(), G.WhiteNoise()
    p = se * per
    assert isinstance(p, G.ProductKernel) and repr(p) == "SquaredExp() * Periodic()"
    assert p.factors() == (se, per) and p.parts() == (p,)
    assert p == G.SquaredExp() * G.Periodic() and p != per * se and p != se
    assert len({p, se * per, per * se}) == 2
    q = p * m32
    assert q.factors() == (se, per, m32) and (m52 * p).factors() == (m52, se, per)
    assert (p * (m32 * m52)).factors() == (se, per, m32, m52)
    assert repr(p * (m32 * m52)) == "SquaredExp() * Periodic() * Matern32() * Matern52()"
    for bad in (lambda: se * wn, lambda: wn * se, lambda: p * wn):
        with pytest.raises(TypeError, match="WhiteNoise"):
            bad()
    for bad in (lambda: (se + per) * m32, lambda: m32 * (se + wn), lambda: p * (se + per)):
        with pytest.raises(TypeError, match="not distributed.*duplicate hyper-parameters"):
            bad()
    with pytest.raises(TypeError):
        se * 2.0


def test_description_plumbing():
    import gpr_amd as G
    from gpr_amd import core
    d = 3
    desc = [[SE, PER], WN, M52, [SE, M32, M52, PER]]
    cov = cov_of(desc)
    assert isinstance(cov, G.ComposedKernel) and len(cov.parts()) == 4
    assert cov.kinds() == codes(desc) == [1, 6, 5, 2, 4, 1, 6, 3, 6, 4, 6, 5]
    assert repr(cov) == ("SquaredExp() * Periodic() + WhiteNoise() + Matern52() + "
                         "SquaredExp() * Matern32() * Matern52() * Periodic()")
    assert (G.SquaredExp() * G.Periodic()).kinds() == [1, 6, 5]
    assert (G.SquaredExp() + G.Periodic()).kinds() == [1, 5]
    w = [(d + 1) + (2 * d + 1), 1, d + 1, 3 * (d + 1) + (2 * d + 1)]
    assert [G.part_dim_hp(k, d) for k in cov.parts()] == w
    assert G.dim_hp(cov, d) == sum(w) == len(model_hp(desc, d, np.random.default_rng(0)))
    assert G.dim_hp(G.SquaredExp() * G.Periodic(), d) == 3 * d + 2
    # find_idx returns the summand
    assert core.find_idx(cov, 1, d) == (0, 1, 0)
    assert core.find_idx(cov, w[0], d) == (0, w[0], 0)
    assert core.find_idx(cov, w[0] + 1, d) == (1, 1, w[0])
    assert core.find_idx(cov, w[0] + 2, d) == (2, 1, w[0] + 1)
    assert core.find_idx(cov, sum(w), d) == (3, w[3], sum(w[:3]))
    with pytest.raises(IndexError):
        core.find_idx(cov, sum(w) + 1, d)
    hp = np.arange(1.0, sum(w) + 1)
    assert [len(h) for h in core._part_hps(cov, hp, d)] == w
    parts, kept = G.rm_noise(cov, core._part_hps(cov, hp, d))
    assert len(parts) == 3 and parts[0] == G.SquaredExp() * G.Periodic() and [len(h) for h in kept] == [w[0], w[2], w[3]]
    import types
    mll_cost = G.MarginalLikelihood()
    for c in (G.SquaredExp() * G.Periodic(), cov):
        assert isinstance(G.islog(mll_cost, types.SimpleNamespace(covar=c)), G.LogScale)
    assert np.array_equal(G.init_params(mll_cost, types.SimpleNamespace(covar=cov, params=hp)), np.ones(len(hp)))
