"""gpr_cv_kfold on the device: every complementary fold's loss (and prediction) from one
factorisation of all points, against the oracle's per-fold fit + full-covariance predict + loss
(rtol 1e-8, the posterior tolerance of tests/test_crossval.py), against the per-fold device
path for the kinds the oracle does not have, between its two routes (GPR_CV_KFOLD_GRAM), twice
on the same inputs (bit for bit), and on fold geometries that reach the ends of Z = U^-T.
"""
import functools

import numpy as np
import pytest

from oracle import gpr_oracle as O

G = pytest.importorskip("gpr_amd")

pytestmark = pytest.mark.gpu

_KINDS = {"SE+WN": (["SE", "WN"], lambda: G.SquaredExp() + G.WhiteNoise()),
          "SE+SE+WN": (["SE", "SE", "WN"],
                       lambda: G.SquaredExp() + G.SquaredExp() + G.WhiteNoise())}
_COSTS = {"MSE": G.MSE, "ChiSq": G.ChiSq, "Mahalanobis": G.Mahalanobis}
# (d, n, k): n not a multiple of 16 with k odd; leave-one-out; the LDS kernels' largest fold over
# five 128-row blocks; the large-fold path (4 folds)
_SHAPES = [(2, 200, 20), (3, 331, 37), (3, 331, 1), (3, 640, 128), (3, 640, 129)]


def _data(d, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((d, n))
    y = np.sin(x.sum(axis=0)) ** 2
    return x, y


@functools.lru_cache(maxsize=None)
def _case(kname, d, n, k):
    """Inputs and the fold structure of one shape (shared, never modified)."""
    kinds, _ = _KINDS[kname]
    x, y = _data(d, n, 11 + d)
    hp = O.default_hp(kinds, d, length=2.0)
    _, tst = G.kfoldcv(n, k, rng=np.random.default_rng(5))
    return x, y, hp, tst


@functools.lru_cache(maxsize=None)
def _oracle_folds(kname, d, n, k):
    """Per fold the oracle's (ytst, yp, Sigma_p): one fit per fold, shared by the three costs and
    the prediction tests."""
    kinds, _ = _KINDS[kname]
    x, y, hp, tst = _case(kname, d, n, k)
    out = []
    for a, b in zip(G.complement_folds(n, tst), tst):
        yp, S = O.predict(kinds, hp, x[:, a], y[a], x[:, b], diagonal_var=False)
        out.append((y[b], yp, S))
    return out


def _oracle_losses(kname, cname, d, n, k):
    """O.cv_batch(kinds, hp, cost, x, y, (complement_folds(n, tst), tst)), fold by fold."""
    return np.array([O.cv_loss(cname, yt, yp, S) for yt, yp, S in _oracle_folds(kname, d, n, k)])


def _model(kname, d, n, k):
    x, y, hp, tst = _case(kname, d, n, k)
    return G.GPRModel(_KINDS[kname][1](), hp, x, y), x, y, tst


def test_oracle_reference_is_cv_batch():
    """The shared per-fold references are the oracle's cv_batch on the complementary cvset."""
    kname, d, n, k = "SE+WN", 2, 200, 20
    kinds, _ = _KINDS[kname]
    x, y, hp, tst = _case(kname, d, n, k)
    for cname in _COSTS:
        want = O.cv_batch(kinds, hp, cname, x, y, (G.complement_folds(n, tst), tst))
        np.testing.assert_array_equal(_oracle_losses(kname, cname, d, n, k), want)


@pytest.mark.parametrize("d,n,k", _SHAPES)
@pytest.mark.parametrize("kname", ["SE+WN", "SE+SE+WN"])
def test_cv_kfold_vs_oracle(kname, d, n, k):
    kinds, _ = _KINDS[kname]
    md, x, y, tst = _model(kname, d, n, k)
    assert np.linalg.cond(O.kernel(kinds, _case(kname, d, n, k)[2], x)) <= 3.6e4
    for cname, cost in _COSTS.items():
        got = G.cv_kfold(md, cost(), x, y, tst)
        want = _oracle_losses(kname, cname, d, n, k)
        print(kname, (d, n, k), cname, "max rel", np.max(np.abs(got - want) / np.abs(want)))
        np.testing.assert_allclose(got, want, rtol=1e-8, atol=0, err_msg=cname)


@pytest.mark.parametrize("d,n,k", [(3, 331, 37), (3, 331, 1)])
def test_predictions_vs_oracle(d, n, k):
    kname = "SE+WN"
    md, x, y, tst = _model(kname, d, n, k)
    lss, mu, var = G.cv_kfold(md, G.Mahalanobis(), x, y, tst, return_pred=True)
    assert mu.shape == var.shape == (len(tst), k)
    folds = _oracle_folds(kname, d, n, k)
    mu_o = np.array([yp for _, yp, _ in folds])
    var_o = np.array([np.diag(S) for _, _, S in folds])
    np.testing.assert_allclose(mu, mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(var, var_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_array_equal(lss, G.cv_kfold(md, G.Mahalanobis(), x, y, tst))


def test_cv_loo_is_cv_kfold_with_one_point_folds():
    d, n = 3, 331
    md, x, y, _ = _model("SE+WN", d, n, 1)
    mu, var = G.cv_loo(md, x, y)
    _, mu1, var1 = G.cv_kfold(md, G.ChiSq(), x, y, [np.array([i]) for i in range(n)],
                              return_pred=True)
    np.testing.assert_array_equal(mu, mu1[:, 0])
    np.testing.assert_array_equal(var, var1[:, 0])
    kinds, _ = _KINDS["SE+WN"]
    K = O.kernel(kinds, _case("SE+WN", d, n, 1)[2], x)
    P = np.linalg.inv(K)
    np.testing.assert_allclose(var, 1.0 / np.diag(P), rtol=1e-8)
    np.testing.assert_allclose(mu, y - (P @ y) / np.diag(P), rtol=1e-8, atol=1e-10)


# hyper-parameters per part: [sigma, l_1..l_d] (SquaredExp, Matern), [sigma, l_1..l_d, p_1..p_d]
# (Periodic), [sigma_n] (WhiteNoise); d = 3
_OTHER = {
    "M52*PER+WN": (lambda: G.Matern52() * G.Periodic() + G.WhiteNoise(),
                   [1.0, 2.0, 2.0, 2.0] + [1.0, 2.0, 1.7, 2.3, 1.3, 1.1, 1.6] + [0.1]),
    "SE+M32+WN": (lambda: G.SquaredExp() + G.Matern32() + G.WhiteNoise(),
                  [1.0, 2.0, 2.0, 2.0] + [0.7, 1.5, 1.8, 1.2] + [0.1]),
}


@pytest.mark.parametrize("name", list(_OTHER))
def test_other_kinds_vs_cv_batch(name):
    """Kinds the oracle does not have: against the per-fold device path (the parent's code, not
    under test here) on the same folds."""
    d, n, k = 3, 331, 37
    x, y = _data(d, n, 11 + d)
    mk, hp = _OTHER[name]
    md = G.GPRModel(mk(), np.array(hp), x, y)
    _, tst = G.kfoldcv(n, k, rng=np.random.default_rng(5))
    cvset = (G.complement_folds(n, tst), tst)
    for cname, cost in _COSTS.items():
        got = G.cv_kfold(md, cost(), x, y, tst)
        want = G.cv_batch(md, cost(), x, y, cvset)
        np.testing.assert_allclose(got, want, rtol=1e-8, atol=0, err_msg=cname)


@pytest.mark.parametrize("d,n,k", [(3, 372, 31), (3, 640, 129)])
def test_routes_agree(d, n, k, knobs):
    """GPR_CV_KFOLD_GRAM 1 (fold Grams of Z) and 0 (gathered from the full K^-1): rtol 1e-9
    between them, each within 1e-8 of the oracle."""
    kname = "SE+WN"
    md, x, y, tst = _model(kname, d, n, k)
    for cname, cost in _COSTS.items():
        knobs("GPR_CV_KFOLD_GRAM", 1)
        assert G.default_context().get_knob("GPR_CV_KFOLD_GRAM") == 1
        g1 = G.cv_kfold(md, cost(), x, y, tst)
        knobs("GPR_CV_KFOLD_GRAM", 0)
        g0 = G.cv_kfold(md, cost(), x, y, tst)
        np.testing.assert_allclose(g1, g0, rtol=1e-9, atol=0, err_msg=cname)
        want = _oracle_losses(kname, cname, d, n, k)
        np.testing.assert_allclose(g1, want, rtol=1e-8, atol=0, err_msg=cname)
        np.testing.assert_allclose(g0, want, rtol=1e-8, atol=0, err_msg=cname)


@pytest.mark.parametrize("d,n,k", [(3, 331, 1), (3, 331, 37), (3, 640, 129)])
def test_repeatable_bit_for_bit(d, n, k):
    md, x, y, tst = _model("SE+WN", d, n, k)
    a = G.cv_kfold(md, G.ChiSq(), x, y, tst, return_pred=True)
    b = G.cv_kfold(md, G.ChiSq(), x, y, tst, return_pred=True)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def _geometry(name):
    d, n = 3, 331
    perm = np.random.default_rng(5).permutation(n)
    if name == "one_fold":
        return d, n, [perm[:37]]
    if name == "overlapping":
        return d, n, [perm[i:i + 40] for i in range(0, 200, 25)]
    if name == "first_third":
        return d, n, [perm[i:i + 11] for i in range(0, n // 3 - 10, 11)]
    if name == "first_and_last_row":
        return d, n, [np.array([0, n - 1]), np.array([n - 1, 0])]
    if name == "n_16m_plus_1":
        n = 16 * 20 + 1
        return d, n, [np.array([n - 1, 5, 160]), np.array([7, n - 1, n - 2])]
    raise KeyError(name)


@pytest.mark.parametrize("name", ["one_fold", "overlapping", "first_third", "first_and_last_row",
                                  "n_16m_plus_1"])
def test_fold_geometry_vs_cv_batch(name):
    d, n, tst = _geometry(name)
    x, y = _data(d, n, 11 + d)
    hp = O.default_hp(["SE", "WN"], d, length=2.0)
    md = G.GPRModel(G.SquaredExp() + G.WhiteNoise(), hp, x, y)
    cvset = (G.complement_folds(n, tst), tst)
    for cname, cost in _COSTS.items():
        got = G.cv_kfold(md, cost(), x, y, tst)
        want = G.cv_batch(md, cost(), x, y, cvset)
        np.testing.assert_allclose(got, want, rtol=1e-8, atol=0, err_msg=cname)


def test_conditioning_bound():
    """SE+WN with noise 1e-3: cond_2(K) ~ 1.1e8.  Both the identity and the oracle's own
    Sigma_p = K_FF - V^T V lose about cond_2(K) u, so the bound is 50 cond_2(K) 2^-53 relative
    (about 6e-7) -- a derived condition, not a measurement."""
    kinds = ["SE", "WN"]
    d, n, k = 2, 257, 16
    x, y = _data(d, n, 13)
    hp = O.default_hp(kinds, d, length=2.0, noise=1e-3)
    cond = np.linalg.cond(O.kernel(kinds, hp, x))
    assert 1e7 < cond < 1e9
    bound = 50.0 * cond * 2.0 ** -53
    md = G.GPRModel(G.SquaredExp() + G.WhiteNoise(), hp, x, y)
    _, tst = G.kfoldcv(n, k, rng=np.random.default_rng(5))
    cvset = (G.complement_folds(n, tst), tst)
    for cname, cost in _COSTS.items():
        got = G.cv_kfold(md, cost(), x, y, tst)
        want = O.cv_batch(kinds, hp, cname, x, y, cvset)
        print(cname, "cond", cond, "bound", bound, "max rel",
              np.max(np.abs(got - want) / np.abs(want)))
        np.testing.assert_allclose(got, want, rtol=bound, atol=0, err_msg=cname)


def test_argument_errors():
    d, n = 2, 50
    x, y = _data(d, n, 0)
    md = G.GPRModel(G.SquaredExp() + G.WhiteNoise(), O.default_hp(["SE", "WN"], d), x, y)
    with pytest.raises(G.GprError, match="out of range"):
        G.cv_kfold(md, G.MSE(), x, y, [np.arange(10), np.arange(45, 55)])
    with pytest.raises(G.GprError, match="twice"):
        G.cv_kfold(md, G.MSE(), x, y, [np.arange(10), np.array([3, 4, 5, 6, 7, 8, 9, 3, 11, 12])])
    with pytest.raises(G.GprError, match="ntst"):
        G.cv_kfold(md, G.MSE(), x, y, [np.arange(n)])
    with pytest.raises(ValueError):
        G.cv_kfold(md, G.MSE(), x, y, [np.arange(10), np.arange(9)])
    # the context is still good
    got = G.cv_kfold(md, G.MSE(), x, y, [np.arange(10)])
    want = G.cv_batch(md, G.MSE(), x, y, ([np.arange(10, n)], [np.arange(10)]))
    np.testing.assert_allclose(got, want, rtol=1e-8)
