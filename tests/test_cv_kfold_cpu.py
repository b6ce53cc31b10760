"""Cross-validation of complementary folds from one factorisation (cv_kfold, cv_loo): the host
helpers, and the identity the device code implements, stated in numpy and held to the oracle's
per-fold fit + full-covariance predict + loss.

With K the kernel matrix of ALL points (eps per SquaredExp part and the noise on its diagonal),
P = K^-1 and alpha = K^-1 y, a fold that tests F and trains on everything else has
Sigma_p = (P_FF)^-1 and y_F - yp = (P_FF)^-1 alpha_F.  No device is needed here.
"""
import numpy as np
import pytest

from oracle import gpr_oracle as O

G = pytest.importorskip("gpr_amd")


def test_complement_folds_of_kfoldcv():
    """kfoldcv(53, 7) leaves 53 - 7 * 7 = 4 points in no test set: they belong to every
    training set; each training set is the complement of its test set."""
    n, k = 53, 7
    trn, tst = G.kfoldcv(n, k, rng=np.random.default_rng(5))
    comp = G.complement_folds(n, tst)
    assert len(comp) == len(tst) == n // k
    left = sorted(set(range(n)) - set(np.concatenate(tst).tolist()))
    assert len(left) == n - (n // k) * k
    for a, b, c in zip(trn, tst, comp):
        assert sorted(a.tolist()) == c.tolist()
        assert sorted(np.concatenate([c, b]).tolist()) == list(range(n))
        assert set(left) <= set(c.tolist())
    assert G.is_kfold_complement(n, (trn, tst))
    assert G.is_kfold_complement(n, (comp, tst))


def test_is_kfold_complement_detects_a_dropped_index():
    n, k = 53, 7
    trn, tst = G.kfoldcv(n, k, rng=np.random.default_rng(5))
    short = [a.copy() for a in trn]
    short[3] = short[3][:-1]
    assert not G.is_kfold_complement(n, (short, tst))
    dup = [a.copy() for a in trn]
    dup[2][0] = dup[2][1]  # right length, one index twice
    assert not G.is_kfold_complement(n, (dup, tst))
    assert not G.is_kfold_complement(n, (trn[:-1], tst))
    assert not G.is_kfold_complement(n + 1, (trn, tst))


def test_exports():
    for name in ("cv_kfold", "cv_loo", "complement_folds", "is_kfold_complement"):
        assert name in G.__all__ and callable(getattr(G, name))


def test_cost_type_checked_before_anything_runs():
    """The cost is checked first: no model, no device."""
    with pytest.raises(TypeError):
        G.cv_kfold(None, G.MarginalLikelihood(), None, None, [[0]])


def _data(d, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((d, n))
    y = np.sin(x.sum(axis=0)) ** 2
    return x, y


def kfold_identity(kinds, hp, cost, x, y, tst, eps=O.EPS_DEFAULT):
    """The identity in numpy: kernel -> Cholesky -> P, alpha -> the fold losses."""
    K = O.kernel(kinds, hp, x, None, eps)
    U = O.chol_upper(K)
    P = O.kinv_from_upper(U)
    alpha = O.cho_solve_upper(U, y)
    out = []
    for F in tst:
        S = np.linalg.inv(P[np.ix_(F, F)])
        r = S @ alpha[F]
        out.append(O.cv_loss(cost, r, np.zeros_like(r), S))
    return np.array(out)


@pytest.mark.parametrize("kinds", [["SE", "WN"], ["SE", "SE", "WN"]], ids=["SE+WN", "SE+SE+WN"])
@pytest.mark.parametrize("d,n,k", [(2, 200, 20), (3, 331, 37), (3, 331, 1)])
def test_identity_vs_oracle(kinds, d, n, k):
    x, y = _data(d, n, 11 + d)
    hp = O.default_hp(kinds, d, length=2.0)
    _, tst = G.kfoldcv(n, k, rng=np.random.default_rng(5))
    cvset = (G.complement_folds(n, tst), tst)
    for cost in ("MSE", "ChiSq", "Mahalanobis"):
        want = O.cv_batch(kinds, hp, cost, x, y, cvset)
        got = kfold_identity(kinds, hp, cost, x, y, tst)
        np.testing.assert_allclose(got, want, rtol=1e-8, atol=0, err_msg=cost)
