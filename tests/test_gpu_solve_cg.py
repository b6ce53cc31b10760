"""GPU: K^{-1} B by matrix-free conjugate gradients (gpr_solve_cg).

SquaredExp + WhiteNoise, n = 300, d = 3, sigma = sigma_n = 1: lambda_min >= 1 and lambda_max <=
n + 1, so cond_2 <= 301 and the textbook bound 0.5 sqrt(cond) ln(2 sqrt(cond) / tol) allows about
231 iterations at tol = 1e-10; the cap is 400.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")
from oracle import gpr_oracle as O  # noqa: E402

N, D, TOL, MAXIT = 300, 3, 1e-10, 400
KINDS = [O.SE, O.WN]


def _problem(nrhs):
    x, y, _ = O.synthetic(D, N, 0)
    hp = O.default_hp(KINDS, D, sigma=1.0, noise=1.0)
    B = y if nrhs == 1 else np.column_stack(
        [y] + [np.random.default_rng(c).standard_normal(N) for c in range(1, nrhs)])
    md = G.GPRModel(G.SquaredExp() + G.WhiteNoise(), hp, x, B)
    return md, O.kernel(KINDS, hp, x), B.reshape(N, -1)


@pytest.mark.parametrize("nrhs", [1, 3])
def test_cg_converges_to_the_dense_solution(nrhs):
    md, K, B = _problem(nrhs)
    X, iters, relres = G.solve_cg(md, tol=TOL, maxit=MAXIT)
    X = X.reshape(N, -1)
    assert iters < MAXIT
    assert relres.shape == (nrhs,) and np.all(relres <= 10 * TOL)
    Xs = np.linalg.solve(K, B)
    cond = np.linalg.cond(K, 2)
    err = np.linalg.norm(X - Xs, axis=0) / np.linalg.norm(Xs, axis=0)
    print(f"iters {iters}, relres {relres}, err {err}, cond {cond:.1f}")
    assert np.all(err <= cond * relres)


def test_maxit_is_reported_not_raised():
    md, K, B = _problem(1)
    X, iters, relres = G.solve_cg(md, tol=TOL, maxit=3)
    assert iters == 3
    true = np.linalg.norm(B[:, 0] - K @ X) / np.linalg.norm(B[:, 0])
    assert relres[0] > TOL
    np.testing.assert_allclose(relres[0], true, rtol=1e-6)
