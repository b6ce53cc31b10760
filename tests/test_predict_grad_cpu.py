"""CPU: the gradients of the posterior with respect to the test inputs, restated in NumPy.

The reference has no such call, so include/gpr_hip.h (gpr_predict_grad) is the contract and
`posterior_grad` below is its checker (tests/test_gpu_predict_grad.py imports it).  With
alpha = K^-1 y and Q = K^-1 K(x, xp), summed over the stationary parts p,

    d mu     / d xp_kj =      sum_p sum_i alpha_i (-W_p(xp_j, x_i)) dD_p/dxp_kj
    d sigma2 / d xp_kj = -2   sum_p sum_i Q_ij    (-W_p(xp_j, x_i)) dD_p/dxp_kj

    SquaredExp / Matern32 / Matern52:  dD/dxp_k = 2 l_k^2 (xp_k - x_k)
    Periodic:                          dD/dxp_k = (4 pi l_k^2 / p_k) sin(2 pi (xp_k - x_k) / p_k)

W = -dk/dD from tests/test_periodic_cpu.py's part_kernel(..., want_w=True); a WhiteNoise part
contributes nothing (the cross kernel has no noise).  Always the cross kernel: the gradients are
those of the smooth function x* -> (mu, sigma^2).  The restatement is pinned by central
differences of that file's predict and of the oracle's own.
"""
import numpy as np
import pytest

import test_periodic_cpu as R
from oracle import gpr_oracle as O
from test_periodic_cpu import M32, M52, PER, SE, WN

EPS = 1e-8


def posterior_grad(kinds, hp, x, y, xp, eps=EPS):
    """(gm, gv): gm[k, j] = d mu(xp_j) / d xp_kj ((ny, d, m) for a 2-D y), gv[k, j] the same of
    the diagonal variance."""
    d, m = x.shape[0], xp.shape[1]
    U = O.chol_upper(R.kernel(kinds, hp, x, None, eps))
    alpha = O.cho_solve_upper(U, y)
    Q = O.cho_solve_upper(U, R.kernel(kinds, hp, x, np.array(xp), eps))  # (a copy: never `xp is x`)
    A = alpha.T if alpha.ndim == 2 else alpha[None, :]
    gm, gv = np.zeros((A.shape[0], d, m)), np.zeros((d, m))
    for kind, h in zip(kinds, R.split_hp(kinds, hp, d)):
        if kind == WN:
            continue
        _, W = R.part_kernel(kind, h, x, xp, False, eps, want_w=True)
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


def central_differences(predict, kinds, hp, x, y, xp, h=1e-5):
    d, m = xp.shape
    fm, fv = np.zeros((d, m)), np.zeros((d, m))
    for k in range(d):
        e = np.zeros((d, 1))
        e[k] = h
        mp, vp = predict(kinds, hp, x, y, xp + e, diagonal_var=True)
        mm, vm = predict(kinds, hp, x, y, xp - e, diagonal_var=True)
        fm[k], fv[k] = (mp - mm) / (2.0 * h), (vp - vm) / (2.0 * h)
    return fm, fv


def relnorm(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def problem(kinds, n, d, m, seed):
    """x, xp uniform in [0, 1], model_hp(lscale=0.3, noise=0.1), y = sin(3 sum x) + 0.1 noise."""
    rng = np.random.default_rng(seed)
    x, xp = rng.random((d, n)), rng.random((d, m))
    hp = R.model_hp(kinds, d, rng, lscale=0.3, noise=0.1)
    y = np.sin(3.0 * x.sum(0)) + 0.1 * rng.standard_normal(n)
    return x, y, xp, hp


CASES = [([SE, WN], 130, 8, 37), ([M32, WN], 97, 2, 20), ([SE, PER, M52, WN], 130, 3, 37),
         ([PER, WN], 66, 11, 9), ([M52, WN], 200, 1, 33)]


@pytest.mark.parametrize("kinds,n,d,m", CASES, ids=["+".join(c[0]) for c in CASES])
def test_restatement_by_central_differences(kinds, n, d, m):
    """Against (f(x + h) - f(x - h)) / 2h of the restated predict, h = 1e-5: truncation ~ h^2 |f'''|
    ~ 1e-8, round-off ~ u |f| / h ~ 1e-11 on these inputs; 1e-6 normwise catches any wrong factor
    or sign."""
    x, y, xp, hp = problem(kinds, n, d, m, n + d)
    gm, gv = posterior_grad(kinds, hp, x, y, xp)
    fm, fv = central_differences(R.predict, kinds, hp, x, y, xp)
    em, ev = relnorm(gm, fm), relnorm(gv, fv)
    print(f"{'+'.join(kinds)} n={n} d={d} m={m}: mean {em:.2e} variance {ev:.2e}")
    assert gm.shape == (d, m) and gv.shape == (d, m)
    assert em <= 1e-6 and ev <= 1e-6


def test_restatement_against_the_oracles_predict():
    """SE+WN against central differences of oracle/gpr_oracle.py's own predict."""
    kinds, n, d, m = [SE, WN], 130, 8, 37
    x, y, xp, hp = problem(kinds, n, d, m, 5)
    gm, gv = posterior_grad(kinds, hp, x, y, xp)
    fm, fv = central_differences(O.predict, [O.SE, O.WN], hp, x, y, xp)
    em, ev = relnorm(gm, fm), relnorm(gv, fv)
    print(f"SE+WN vs the oracle: mean {em:.2e} variance {ev:.2e}")
    assert em <= 1e-6 and ev <= 1e-6


def test_two_columns_of_y():
    kinds, n, d, m = [SE, M32, WN], 80, 3, 11
    x, y, xp, hp = problem(kinds, n, d, m, 3)
    Y = np.stack([y, 2.0 * y - 1.0], axis=1)
    gm2, gv2 = posterior_grad(kinds, hp, x, Y, xp)
    gm, gv = posterior_grad(kinds, hp, x, y, xp)
    gmb, _ = posterior_grad(kinds, hp, x, Y[:, 1].copy(), xp)
    assert gm2.shape == (2, d, m)
    np.testing.assert_allclose(gm2[0], gm, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(gm2[1], gmb, rtol=1e-12, atol=1e-14)
    assert np.array_equal(gv2, gv)


def test_periodicity():
    """PER+WN: a test coordinate shifted by its period leaves both gradients unchanged.  The
    shifted angle 2 pi (r + p) / p carries ~ u 2 pi (|r| / p + 1) ~ 3e-15 of rounding: 1e-9."""
    kinds, n, d, m = [PER, WN], 66, 4, 9
    x, y, xp, hp = problem(kinds, n, d, m, 17)
    ps = hp[1 + d:1 + 2 * d]
    gm, gv = posterior_grad(kinds, hp, x, y, xp)
    for k in (0, 2):
        xs = xp.copy()
        xs[k] += ps[k]
        gms, gvs = posterior_grad(kinds, hp, x, y, xs)
        assert relnorm(gms, gm) <= 1e-9 and relnorm(gvs, gv) <= 1e-9


def test_package_exports_predict_grad():
    import gpr_amd as G
    from gpr_amd import _lib as L
    for name in ("predict_grad", "predict_grad_"):
        assert hasattr(G, name) and name in G.__all__
    assert "gpr_predict_grad" in L._SIGS and hasattr(L.lib, "gpr_predict_grad")
    assert "gpr_predict_grad" in L.header_exports()
    assert len(L._SIGS["gpr_predict_grad"][1]) == 18
