"""CPU: the block formulas behind gpr_fit_append restated in NumPy, and the case tables that
tests/test_gpu_append.py runs on the device.

With K = U^T U the fitted n0 x n0 block, B = K(x, x_new), K_new = K(x_new, x_new) in the 4-arg
(GPR_SELF) form and c = y_new - B^T alpha:

    V = U^{-T} B,   S = K_new - V^T V = R^T R,   U' = [U V; 0 R]
    alpha'_tail = S^{-1} c,   alpha'_head = alpha - U^{-1} (V alpha'_tail)

The reference is always the full fit of all n0 + m points (O.chol_upper / O.cho_solve_upper on
K from oracle.gpr_oracle.kernel for SquaredExp / WhiteNoise descriptions, from the restated
kernels of tests/test_periodic_cpu.py for Matern and Periodic parts).  Every case of the GPU
file's tables is checked here first, at the GPU file's tolerances: this pins the formulas, and
shows that they meet those tolerances on these inputs in exact-enough arithmetic.  Every case
carries a WhiteNoise part sigma_n = 0.1 and l_k ~ 0.3 sqrt(8/d), and asserts that K is far from
diagonal and factorable.

The targets are smooth and noise-free, y = cos(sum_k x_k) (a second column 0.25 sin^2(2 sum_k x_k)),
so that max |alpha| stays near 1: with sigma_n = 0.1 the condition number of K is about
n sigma^2 / sigma_n^2 ~ 1e5, any solve -- the reference's own included -- leaves alpha with
an error of a few 1e-13 max |alpha| (measured: 4e-13 max |alpha| between two orders of the same
arithmetic), and the entries of alpha that pass near zero are held to atol 1e-12 alone.  A noisy
target (max |alpha| ~ 30) puts the reference's own rounding above that.
"""
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import test_periodic_cpu as R
from oracle import gpr_oracle as O
from test_periodic_cpu import M32, M52, PER, SE, WN

# tolerances of the same quantities from gpr_fit (tests/test_gpu_parity.py)
TOL_U = dict(rtol=1e-8, atol=1e-12)       # U's upper triangle, alpha
TOL_MU = dict(rtol=1e-8, atol=1e-10)
TOL_K = dict(rtol=1e-13, atol=0.0)        # the strict lower triangle against K
TOL_MLL = 1e-10

# ---- the case tables (shared with the GPU file) -----------------------------------------------
# block edges of the 128-column pipeline: below / at / above one block, a ragged last block, a
# last group of fewer than 16 columns, more than one group, m beyond 128 (the GEMM route)
SHAPES = [(100, 1), (127, 1), (128, 1), (128, 128), (200, 17), (255, 3), (383, 130), (1000, 16),
          (1037, 5), (2048, 33)]
SHAPE_KINDS, SHAPE_D = [SE, WN], 2
KIND_SETS = {
    "SE+M52+WN": [SE, M52, WN],
    "M32+WN": [M32, WN],
    "SE+PER+WN": [SE, PER, WN],
    "SEx5+WN": [SE, SE, SE, SE, SE, WN],
}
KIND_SHAPE = (300, 9)
KIND_DS = [3, 33]
NRHS_CASE = dict(kinds=[SE, WN], n0=300, m=9, d=2, ny=2, ldy_pad=5)
CHAIN = dict(kinds=[SE, WN], d=2, n0=250, steps=[1, 5, 1, 130])
KNOB_SHAPES = [(1000, 16), (1037, 5)]
NOT_PD = dict(kinds=[SE, WN], d=2, n0=150, eps_append=-1.0)


def seed_of(n0, m, d, kinds):
    return 100000 * len(kinds) + 1000 * d + 7 * n0 + m


def kernel(kinds, hp, x, xp=None, eps=R.EPS):
    """K by the oracle where it has the kinds, else by the restated kernels"""
    if all(k in (SE, WN) for k in kinds):
        return O.kernel([O.SE if k == SE else O.WN for k in kinds], hp, x, xp, eps)
    return R.kernel(kinds, hp, x, xp, eps)


def assert_well_conditioned(K):
    """far from diagonal (as tests/test_gpu_predict_grad.py), and factorable"""
    n = K.shape[0]
    off = K[~np.eye(n, dtype=bool)]
    assert np.median(off) > 0.05, f"median off-diagonal {np.median(off):.3g}: K is nearly diagonal"
    return O.chol_upper(K)


@functools.lru_cache(maxsize=None)
def _case(kinds, n, d, seed, ny):
    rng = np.random.default_rng(seed)
    x = rng.random((d, n))
    hp = R.model_hp(list(kinds), d, rng, lscale=0.3, noise=0.1)
    s = x.sum(0)
    y = np.cos(s)  # (smooth and noise-free: alpha stays O(1), see the module docstring)
    if ny > 1:
        y = np.stack([y] + [0.25 * np.sin((c + 1.0) * s) ** 2 for c in range(1, ny)], axis=1)
    K = kernel(list(kinds), hp, x)
    U = assert_well_conditioned(K)
    alpha = O.cho_solve_upper(U, y)
    for a in (x, hp, y, K, U, alpha):  # (shared between tests: kept unchanged)
        a.setflags(write=False)
    return x, y, hp, K, U, alpha


def make_case(kinds, n0, m, d, ny=1):
    """(x, y, hp) of all n0 + m points and the full fit's (K, U, alpha) on them"""
    return _case(tuple(kinds), n0 + m, d, seed_of(n0, m, d, kinds), ny)


# ---- the restatement ----------------------------------------------------------------------------
def block_append(kinds, hp, x, y, n0, U0, alpha0, eps=R.EPS):
    """(info, U', alpha', schur pivots) from the old factor by the block formulas"""
    N = x.shape[1]
    xo, xn = x[:, :n0], x[:, n0:]
    B = kernel(kinds, hp, xo, xn, eps)             # plain cross kernel
    Kn = kernel(kinds, hp, xn, None, eps)          # GPR_SELF form
    c = y[n0:] - B.T @ alpha0
    V = sla.solve_triangular(U0, B, trans="T", lower=False, check_finite=False)
    S = Kn - V.T @ V
    Rf = np.array(S)
    pivots = []
    for j in range(N - n0):   # dpotrf 'U', unblocked: the order of the failing minor
        p = Rf[j, j] - Rf[:j, j] @ Rf[:j, j]
        pivots.append(p)
        if not p > 0.0:
            return n0 + j + 1, None, None, pivots
        Rf[j, j] = np.sqrt(p)
        Rf[j, j + 1:] = (Rf[j, j + 1:] - Rf[:j, j] @ Rf[:j, j + 1:]) / Rf[j, j]
    Rf = np.triu(Rf)
    Un = np.zeros((N, N))
    Un[:n0, :n0], Un[:n0, n0:], Un[n0:, n0:] = np.triu(U0), V, Rf
    tail = O.cho_solve_upper(Rf, c)
    head = alpha0 - sla.solve_triangular(U0, V @ tail, lower=False, check_finite=False)
    return 0, Un, np.concatenate([head, tail], axis=0), pivots


def old_fit(kinds, hp, x, y, n0):
    U0 = O.chol_upper(kernel(kinds, hp, x[:, :n0]))
    return U0, O.cho_solve_upper(U0, y[:n0])


def check_against_full_fit(kinds, n0, m, d, ny=1):
    x, y, hp, K, U, alpha = make_case(kinds, n0, m, d, ny)
    U0, a0 = old_fit(kinds, hp, x, y, n0)
    info, Un, an, _ = block_append(kinds, hp, x, y, n0, U0, a0)
    assert info == 0
    np.testing.assert_allclose(np.triu(Un), np.triu(U), **TOL_U)
    np.testing.assert_allclose(an, alpha, **TOL_U)
    return x, y, hp, Un, an


@pytest.mark.parametrize("n0,m", SHAPES)
def test_block_edge_shapes(n0, m):
    check_against_full_fit(SHAPE_KINDS, n0, m, SHAPE_D)


@pytest.mark.parametrize("d", KIND_DS)
@pytest.mark.parametrize("name", list(KIND_SETS))
def test_kinds(name, d):
    check_against_full_fit(KIND_SETS[name], *KIND_SHAPE, d)


def test_two_columns_of_y():
    c = NRHS_CASE
    x, y, hp, Un, an = check_against_full_fit(c["kinds"], c["n0"], c["m"], c["d"], c["ny"])
    assert an.shape == (c["n0"] + c["m"], 2)


def test_knob_shapes_are_in_the_table():
    assert set(KNOB_SHAPES) <= set(SHAPES)


def test_chained_appends():
    """250 -> +1 -> +5 -> +1 -> +130, each step from the previous step's factor and alpha; then
    the posterior and the MLL from the appended factor against the full fit's"""
    kinds, d, n = CHAIN["kinds"], CHAIN["d"], CHAIN["n0"]
    total = n + sum(CHAIN["steps"])
    x, y, hp, K, U, alpha = make_case(kinds, n, total - n, d)
    Uc, ac = old_fit(kinds, hp, x, y, n)
    for m in CHAIN["steps"]:
        info, Uc, ac, _ = block_append(kinds, hp, x[:, :n + m], y[:n + m], n, Uc, ac)
        assert info == 0
        n += m
        Uf = O.chol_upper(kernel(kinds, hp, x[:, :n]))
        np.testing.assert_allclose(np.triu(Uc), Uf, **TOL_U)
        np.testing.assert_allclose(ac, O.cho_solve_upper(Uf, y[:n]), **TOL_U)
    assert n == total
    np.testing.assert_allclose(O.mll_value(Uc, y, ac), O.mll_value(U, y, alpha), rtol=TOL_MLL)
    xp = np.random.default_rng(5).random((d, 21))
    okinds = [O.SE, O.WN]
    mu, var = O.predict_from_factor(okinds, hp, x, Uc, ac, xp, diagonal_var=True)
    mu_f, var_f = O.predict(okinds, hp, x, y, xp, diagonal_var=True)
    np.testing.assert_allclose(mu, mu_f, **TOL_MU)
    np.testing.assert_allclose(var, var_f, rtol=1e-8, atol=1e-8 * O.diag_prior(okinds, hp, d))


def not_pd_case():
    """SE+WN with sigma = 1, sigma_n = 0.1: n0 points and one more, coincident with training
    point 3 -- (x, y, hp) of all n0 + 1 points"""
    c = NOT_PD
    rng = np.random.default_rng(11)
    x = rng.random((c["d"], c["n0"] + 1))
    x[:, -1] = x[:, 3]
    hp = R.model_hp(c["kinds"], c["d"], rng, lscale=0.3, noise=0.1)
    assert hp[0] == 1.0 and hp[-1] == 0.1
    y = np.cos(x.sum(0))
    return x, y, hp


def test_not_positive_definite_pivot():
    """a coincident point appended with eps = -1: the new diagonal entry is sigma^2 - 1 +
    sigma_n^2 = 0.01, the Schur pivot 0.01 - v^T v with v^T v close to 1: far below zero, so the
    failure does not hang on rounding.  info is n0 + 1, what dpotrf on the whole matrix gives."""
    c = NOT_PD
    x, y, hp = not_pd_case()
    n0 = c["n0"]
    U0, a0 = old_fit(c["kinds"], hp, x, y, n0)
    info, _, _, piv = block_append(c["kinds"], hp, x, y, n0, U0, a0, eps=c["eps_append"])
    assert info == n0 + 1
    assert piv[0] < -0.1, piv
    # the whole matrix, as dpotrf sees it
    K = kernel(c["kinds"], hp, x)
    K[n0, n0] += c["eps_append"] - R.EPS
    with pytest.raises(np.linalg.LinAlgError, match=f"{n0 + 1}-th leading minor"):
        sla.cholesky(K, lower=False)
    # and with the default eps the same append succeeds
    info, Un, an, _ = block_append(c["kinds"], hp, x, y, n0, U0, a0)
    assert info == 0
    np.testing.assert_allclose(np.triu(Un), O.chol_upper(kernel(c["kinds"], hp, x)), **TOL_U)


def test_header_and_binding():
    import gpr_amd as G
    from gpr_amd import _lib as L
    assert "gpr_fit_append" in L.header_exports()
    assert "gpr_fit_append" in L._SIGS and hasattr(L.lib, "gpr_fit_append")
    assert len(L._SIGS["gpr_fit_append"][1]) == 17
    assert hasattr(G, "append_") and "append_" in G.__all__
