"""Leave-one-out training, the parts that need no device: the exports and the dispatch of the
cost layer, and the identities the device code is built on, restated in numpy on the oracle.

A leave-one-out criterion is L = sum_i f(alpha_i, P_ii) with P = K^-1 and alpha = K^-1 y:
  LogPredictive  f = -1/2 log P_ii + alpha_i^2 / (2 P_ii) + 1/2 log 2pi
  MSE            f = (alpha_i / P_ii)^2
  ChiSq          f = alpha_i^2 / P_ii            (Mahalanobis on a single point: the same)
and, with b = P f_alpha and D = diag(f_P),
  dL/dtheta_j = -sum_ab dK_j,ab [ 1/2 (b_a alpha_b + alpha_a b_b) + (P D P)_ab ].
``loo_reference`` is that, and the reference of tests/test_gpu_loo.py.  Here it is checked
against n brute-force refits (the value) and central differences (the gradient).
"""
import functools
import types

import numpy as np
import pytest

from oracle import gpr_oracle as O

CRITS = ("LogPredictive", "MSE", "ChiSq", "Mahalanobis")


def loo_terms(crit, a, p):
    """(f, f_alpha, f_P) per point from alpha and diag(P)."""
    if crit == "LogPredictive":
        return (-0.5 * np.log(p) + a * a / (2 * p) + 0.5 * np.log(2 * np.pi), a / p,
                -0.5 / p - a * a / (2 * p * p))
    if crit == "MSE":
        return (a / p) ** 2, 2 * a / (p * p), -2 * a * a / p ** 3
    if crit in ("ChiSq", "Mahalanobis"):
        return a * a / p, 2 * a / p, -a * a / (p * p)
    raise ValueError(crit)


def loo_from_matrices(K, dKs, crit, y):
    """(value, grad, f) of the criterion from the kernel matrix K and its derivatives dKs (one per
    hyper-parameter: an n x n matrix, or ("I", lam) for lam I): P and alpha through the Cholesky
    factor, as the oracle's MLL."""
    U = O.chol_upper(K)
    P = O.kinv_from_upper(U)
    P = 0.5 * (P + P.T)
    a = O.cho_solve_upper(U, y)
    f, fa, fp = loo_terms(crit, a, np.diag(P))
    b = P @ fa
    W = 0.5 * (np.outer(b, a) + np.outer(a, b)) + (P * fp) @ P  # P diag(f_P) P
    g = np.array([-(dK[1] * np.trace(W)) if isinstance(dK, tuple) else -np.sum(W * dK)
                  for dK in dKs])
    return float(f.sum()), g, f


def loo_reference(kinds, hp, crit, x, y):
    """(value, grad) of LeaveOneOut(crit) on the oracle's kernel and its kernel_grad (1-based
    index; a WhiteNoise part comes back as ("I", lam))."""
    hp = np.asarray(hp, dtype=np.float64)
    K = O.kernel(kinds, hp, x, None, O.EPS_DEFAULT)
    dKs = [O.kernel_grad(kinds, i + 1, hp, x) for i in range(len(hp))]
    value, g, _ = loo_from_matrices(K, dKs, crit, y)
    return value, g


def loo_abs_sum(kinds, hp, crit, x, y):
    """sum_i |f_i|: the scale of the value's absolute tolerance."""
    K = O.kernel(kinds, np.asarray(hp, dtype=np.float64), x, None, O.EPS_DEFAULT)
    return float(np.abs(loo_from_matrices(K, [], crit, y)[2]).sum())


def data(d, n, seed):
    """The inputs of tests/test_gpu_cv_kfold.py."""
    rng = np.random.default_rng(seed)
    x = rng.random((d, n))
    y = np.sin(x.sum(axis=0)) ** 2
    return x, y


_KINDS = {"SE+WN": ["SE", "WN"], "SE+SE+WN": ["SE", "SE", "WN"]}


@functools.lru_cache(maxsize=None)
def _case(kname):
    d, n = 2, 40
    x, y = data(d, n, 11 + d)
    return x, y, O.default_hp(_KINDS[kname], d, length=2.0)


@functools.lru_cache(maxsize=None)
def _refits(kname):
    """The n leave-one-out predictions by n refits: (residual, variance) per point."""
    x, y, hp = _case(kname)
    n = len(y)
    r, v = np.zeros(n), np.zeros(n)
    for i in range(n):
        tr = np.arange(n) != i
        mu, S = O.predict(_KINDS[kname], hp, x[:, tr], y[tr], x[:, [i]], diagonal_var=False)
        r[i], v[i] = y[i] - mu[0], S[0, 0]
    return r, v


# ---------------------------------------------------------------------------------------
# exports and dispatch (no device)
# ---------------------------------------------------------------------------------------
class _Untouchable:
    """Stands in for a model or a cache: any use of it is device work that must not happen."""

    def __getattr__(self, name):
        raise AssertionError(f"touched .{name} before refusing the cost")


def test_exports():
    import gpr_amd as G
    from gpr_amd import _lib as L
    for name in ("LeaveOneOut", "LogPredictive", "LooLossCache"):
        assert name in G.__all__ and hasattr(G, name)
    assert L.GPR_COST_LOGPRED == 4
    assert "#define GPR_COST_LOGPRED 4" in open(L.HEADER).read()
    assert isinstance(G.LeaveOneOut().cost, G.LogPredictive)
    assert repr(G.LeaveOneOut(G.MSE())) == "LeaveOneOut(MSE())"
    for name in ("gpr_fit_loo", "gpr_loo", "gpr_loo_grad"):
        assert name in L.header_exports() and hasattr(L.lib, name)


def test_caches_per_loss():
    import gpr_amd as G
    mll = G.MarginalLikelihood()
    assert G.loss_cache(mll) is G.MllLossCache
    assert G.grad_cache(mll) is G.MllGradCache and G.loss_grad_cache(mll) is G.MllGradCache
    for c in (None, G.LogPredictive(), G.MSE(), G.ChiSq(), G.Mahalanobis()):
        loo = G.LeaveOneOut(c) if c is not None else G.LeaveOneOut()
        assert G.loss_cache(loo) is G.LooLossCache
        assert G.grad_cache(loo) is G.MllGradCache and G.loss_grad_cache(loo) is G.MllGradCache
    assert not issubclass(G.LooLossCache, G.MllLossCache)
    for bad in (object(), G.MSE(), G.LogPredictive()):
        with pytest.raises(TypeError):
            G.loss_cache(bad)
        with pytest.raises(TypeError):
            G.grad_cache(bad)


def test_unknown_inner_cost_is_refused_before_any_device_work():
    import gpr_amd as G
    md, tc = _Untouchable(), _Untouchable()
    hp = np.ones(4)
    for inner in (G.MarginalLikelihood(), object(), "MSE", G.LeaveOneOut()):
        bad = G.LeaveOneOut(inner)
        calls = (lambda: G.loss(bad, md), lambda: G.loss(bad, hp, md), lambda: G.loss(bad, hp, md, tc),
                 lambda: G.loss(bad, md, tc), lambda: G.grad(bad, hp, md),
                 lambda: G.grad_(np.zeros(4), bad, hp, md, tc),
                 lambda: G.loss_grad_(bad, True, np.zeros(4), hp, md, tc),
                 lambda: G.log_loss_grad_(bad, True, np.zeros(4), np.zeros(4), md, tc),
                 lambda: G.loss_cache(bad), lambda: G.grad_cache(bad))
        for call in calls:
            with pytest.raises(TypeError, match="no leave-one-out criterion"):
                call()
        stub = types.SimpleNamespace(covar=G.SquaredExp() + G.WhiteNoise(), params=hp)
        for method in (G.NelderMead(), G.LBFGS(), G.NewtonTrustRegion()):
            with pytest.raises(TypeError, match="no leave-one-out criterion"):
                G.train(stub, bad, hp, method=method)
    # LogPredictive stays out of cv_batch / cv_kfold
    from gpr_amd import crossval
    for f in (lambda: G.cv_kfold(md, G.LogPredictive(), None, None, None),
              lambda: crossval._cost_code(G.LogPredictive())):  # (what cv_batch asks)
        with pytest.raises(TypeError, match="no cross-validation loss"):
            f()


def test_cache_of_the_wrong_type_is_refused_before_any_device_work():
    import gpr_amd as G
    md = _Untouchable()
    hp = np.ones(4)
    loo = G.LeaveOneOut()
    loss_only = object.__new__(G.MllLossCache)   # (no device buffers: never looked at)
    loo_cache = object.__new__(G.LooLossCache)
    for tc in (loss_only, object()):
        with pytest.raises(TypeError, match="LeaveOneOut needs"):
            G.loss(loo, hp, md, tc)
    with pytest.raises(TypeError, match="LeaveOneOut needs"):
        G.loss(loo, md, loss_only)
    for tc in (loss_only, loo_cache, object()):
        with pytest.raises(TypeError, match="LeaveOneOut needs an MllGradCache"):
            G.grad_(np.zeros(4), loo, hp, md, tc)
        with pytest.raises(TypeError, match="LeaveOneOut needs an MllGradCache"):
            G.loss_grad_(loo, True, np.zeros(4), hp, md, tc)
        with pytest.raises(TypeError, match="LeaveOneOut needs an MllGradCache"):
            G.log_loss_grad_(loo, True, None, np.zeros(4), md, tc)
    # the model-update calls keep refusing what they cannot update
    for f in (G.append_, G.remove_):
        with pytest.raises(TypeError):
            f(loo_cache, md, np.zeros(1), np.zeros(1)) if f is G.append_ else f(loo_cache, md, [0])


def test_init_params_and_islog():
    import gpr_amd as G
    cov = G.SquaredExp() + G.WhiteNoise()
    md = types.SimpleNamespace(covar=cov, params=np.arange(1.0, 5.0))
    assert np.array_equal(G.init_params(G.MarginalLikelihood(), md), np.ones(4))
    p = G.init_params(G.LeaveOneOut(), md, rng=np.random.default_rng(0))
    assert p.shape == (4,) and np.all(p >= 0.0) and np.all(p < 1.0) and len(set(p)) == 4
    assert isinstance(G.islog(G.LeaveOneOut(), md), G.LogScale)
    wn = types.SimpleNamespace(covar=G.WhiteNoise(), params=np.ones(1))
    assert isinstance(G.islog(G.LeaveOneOut(), wn), G.NoLogScale)


# ---------------------------------------------------------------------------------------
# the identities, in numpy
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", list(_KINDS))
@pytest.mark.parametrize("crit", CRITS)
def test_value_equals_n_refits(kname, crit):
    x, y, hp = _case(kname)
    r, v = _refits(kname)
    want = {"LogPredictive": 0.5 * np.log(v) + r * r / (2 * v) + 0.5 * np.log(2 * np.pi),
            "MSE": r * r, "ChiSq": r * r / v, "Mahalanobis": r * r / v}[crit].sum()
    got, _ = loo_reference(_KINDS[kname], hp, crit, x, y)
    np.testing.assert_allclose(got, want, rtol=1e-10)


@pytest.mark.parametrize("kname", list(_KINDS))
@pytest.mark.parametrize("crit", CRITS)
def test_gradient_equals_central_differences(kname, crit):
    x, y, hp = _case(kname)
    kinds = _KINDS[kname]
    L, g = loo_reference(kinds, hp, crit, x, y)
    fd = np.zeros_like(g)
    for i in range(len(hp)):
        h = 1e-6 * max(1.0, abs(hp[i]))
        up, dn = hp.copy(), hp.copy()
        up[i] += h
        dn[i] -= h
        fd[i] = (loo_reference(kinds, up, crit, x, y)[0] - loo_reference(kinds, dn, crit, x, y)[0]) / (2 * h)
    # (the differences' own rounding: two values of size |L| good to ~cond(K) u, over 2 h)
    np.testing.assert_allclose(g, fd, rtol=1e-4, atol=1e-9 * max(1.0, abs(L)))


@pytest.mark.parametrize("kname", list(_KINDS))
def test_classical_costs_are_the_sum_of_singleton_folds(kname):
    x, y, hp = _case(kname)
    n = len(y)
    kinds = _KINDS[kname]
    tst = [np.array([i]) for i in range(n)]
    trn = [np.flatnonzero(np.arange(n) != i) for i in range(n)]
    for crit in ("MSE", "ChiSq", "Mahalanobis"):
        folds = O.cv_batch(kinds, hp, crit, x, y, (trn, tst))
        got, _ = loo_reference(kinds, hp, crit, x, y)
        np.testing.assert_allclose(got, folds.sum(), rtol=1e-10)
