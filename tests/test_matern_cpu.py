"""CPU: the Matern-3/2 / Matern-5/2 kernels restated in NumPy, and the description plumbing.

The reference has no Matern kernel, so the definitions of include/gpr_hip.h are the contract and
this restatement is their checker (tests/test_gpu_matern.py imports it).  It is written in the
reference's difference form (scale, subtract, square, sum feature by feature) and composes parts
exactly as oracle/gpr_oracle.py does for SquaredExp: parts summed in `+` order, eps once per
stationary part on a same-object diagonal, the first WhiteNoise's sigma_n^2 only in the 4-arg
form, dK/dsigma = (2/|sigma|) K_p with eps, dK/dl_k = -2 l_k W (x_k - x'_k)^2 on raw x with
W = -dk/dD.  For descriptions of SquaredExp / WhiteNoise parts it must agree with the oracle
(asserted below), which pins the composition rules; the two new profiles are pinned by finite
differences of their own derivatives, their limits at r = 0 and positive definiteness.

    D = sum_k (l_k (x_k - x'_k))^2,  r = sqrt(max(D, 0))
    M32  k = s^2 (1 + sqrt3 r) exp(-sqrt3 r)              W = s^2 (3/2) exp(-sqrt3 r)
    M52  k = s^2 (1 + sqrt5 r + 5 r^2/3) exp(-sqrt5 r)    W = s^2 (5/6) (1 + sqrt5 r) exp(-sqrt5 r)
    SE   k = s^2 exp(-D)                                  W = k
"""
import math
import types

import numpy as np
import pytest
import scipy.linalg as sla

from oracle import gpr_oracle as O

SE, WN, M32, M52 = "SE", "WN", "M32", "M52"
EPS = 1e-8
KIND_CODE = {SE: 1, WN: 2, M32: 3, M52: 4}


# ---------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------
def stationary(kind):
    return kind != WN


def dim_hp(kind, d):
    return d + 1 if stationary(kind) else 1


def split_hp(kinds, hp, d):
    dims = [dim_hp(k, d) for k in kinds]
    assert sum(dims) == len(hp), "Parameter size mismatch."
    out, c = [], 0
    for n in dims:
        out.append(np.asarray(hp[c:c + n], dtype=np.float64))
        c += n
    return out


def profile(kind, D):
    """(f, w) with k = s^2 f(D), W = s^2 w(D)."""
    if kind == SE:
        f = np.exp(-1.0 * D)
        return f, f
    r = np.sqrt(np.maximum(D, 0.0))
    if kind == M32:
        a = math.sqrt(3.0) * r
        e = np.exp(-a)
        return (1.0 + a) * e, 1.5 * e
    if kind == M52:
        a = math.sqrt(5.0) * r
        e = np.exp(-a)
        return (1.0 + a + a * a / 3.0) * e, (5.0 / 6.0) * (1.0 + a) * e
    raise ValueError(kind)


def part_kernel(kind, hp, x, xp, same, eps=EPS, want_w=False):
    sigma, ls = hp[0], hp[1:]
    D = O.distance_euclid(x * ls[:, None], xp * ls[:, None])
    f, w = profile(kind, D)
    K = (sigma ** 2) * f
    if same:
        K[np.diag_indices(K.shape[0])] += eps
    return (K, (sigma ** 2) * w) if want_w else K


def kernel(kinds, hp, x, xp=None, eps=EPS):
    d = x.shape[0]
    noise = xp is None
    same = noise or xp is x
    xq = x if same else xp
    hps = split_hp(kinds, hp, d)
    st = [i for i, k in enumerate(kinds) if stationary(k)]
    assert st, "kernel needs at least one stationary part"
    K = part_kernel(kinds[st[0]], hps[st[0]], x, xq, same, eps)
    for i in st[1:]:
        K = K + part_kernel(kinds[i], hps[i], x, xq, same, eps)
    if noise and WN in kinds:
        K[np.diag_indices(K.shape[0])] += hps[kinds.index(WN)][0] ** 2
    return K


def kernels(kinds, hp, x, eps=EPS):
    hps = split_hp(kinds, hp, x.shape[0])
    return [np.zeros((1, 1)) if k == WN else part_kernel(k, h, x, x, True, eps)
            for k, h in zip(kinds, hps)]


def kernel_grad(kinds, i, hp, x, eps=EPS):
    """1-based i; WhiteNoise -> ("I", 2 sigma_n) as the oracle."""
    d = x.shape[0]
    hps = split_hp(kinds, hp, d)
    dims = np.cumsum([dim_hp(k, d) for k in kinds])
    kidx = int(np.searchsorted(dims, i))
    hpidx = i if kidx == 0 else i - dims[kidx - 1]
    part = hps[kidx]
    if kinds[kidx] == WN:
        return ("I", 2.0 * part[0])
    Kp, W = part_kernel(kinds[kidx], part, x, x, True, eps, want_w=True)
    if hpidx == 1:
        return (2.0 / abs(part[0])) * Kp
    k = hpidx - 2
    return -2.0 * part[hpidx - 1] * W * (x[k][:, None] - x[k][None, :]) ** 2


def mll(kinds, hp, x, y, eps=EPS):
    U = O.chol_upper(kernel(kinds, hp, x, None, eps))
    return O.mll_value(U, y, O.cho_solve_upper(U, y))


def mll_grad(kinds, hp, x, y, eps=EPS, log_scale=False):
    """The trace formula: g_i = -0.5 (alpha' dK_i alpha - <K^-1, dK_i>)."""
    hp = np.asarray(hp, dtype=np.float64)
    U = O.chol_upper(kernel(kinds, hp, x, None, eps))
    alpha = O.cho_solve_upper(U, y)
    Kinv = O.kinv_from_upper(U)
    g = np.array([O.mll_grad_term(kernel_grad(kinds, i, hp, x, eps), alpha, Kinv)
                  for i in range(1, len(hp) + 1)])
    return g * hp if log_scale else g


def diag_prior(kinds, hp, d):
    hps = split_hp(kinds, hp, d)
    return float(hps[0][0] ** 2) if len(kinds) == 1 else float(sum(h[0] ** 2 for h in hps))


def predict(kinds, hp, x, y, xp, diagonal_var=False, eps=EPS):
    U = O.chol_upper(kernel(kinds, hp, x, None, eps))
    wt = O.cho_solve_upper(U, y)
    Kxp = kernel(kinds, hp, xp, x, eps)
    mu = Kxp @ wt
    V = sla.solve_triangular(U, Kxp.T, trans="T", lower=False, check_finite=False).T
    if diagonal_var:
        return mu, diag_prior(kinds, hp, x.shape[0]) - np.sum(V * V, axis=1)
    return mu, kernel(kinds, hp, xp, None, eps) - V @ V.T


def cv_batch(kinds, hp, cost, x, y, cvset, eps=EPS):
    out = []
    for a, b in zip(*cvset):
        yp, S = predict(kinds, hp, x[:, a], y[a], x[:, b], diagonal_var=False, eps=eps)
        out.append(O.cv_loss(cost, y[b], yp, S))
    return np.array(out)


def rand_hp(kinds, d, rng, lo=0.3, hi=2.0):
    return rng.uniform(lo, hi, sum(dim_hp(k, d) for k in kinds))


# ---------------------------------------------------------------------------------------
# the restatement's own checks
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [M32, M52])
def test_kernel_grad_by_central_differences(kind):
    """dK/dsigma and dK/dl_k against (K(h+) - K(h-)) / 2h, h = 1e-6.  Bound 1e-8: the rounding
    of the difference quotient is ~ u |K| / h = 1e-10 per entry (|K| <= 4 here), its truncation
    h^2 |K'''| / 6 ~ 1e-12; 1e-8 leaves two decimal digits over both (measured 6e-10 / 3e-10)."""
    rng = np.random.default_rng(5)
    d, n, h = 3, 40, 1e-6
    x = rng.random((d, n))
    kinds = [kind]
    hp = rand_hp(kinds, d, rng)
    for i in range(1, d + 2):
        e = np.zeros(d + 1)
        e[i - 1] = h
        fd = (kernel(kinds, hp + e, x) - kernel(kinds, hp - e, x)) / (2.0 * h)
        if i == 1:  # the rule's K_p carries eps on the diagonal, which no derivative of K has
            fd[np.diag_indices(n)] += (2.0 / abs(hp[0])) * EPS
        err = np.abs(kernel_grad(kinds, i, hp, x) - fd).max()
        print(f"{kind} hp index {i}: max |analytic - FD| = {err:.2e}")
        assert err <= 1e-8


@pytest.mark.parametrize("kind", [M32, M52])
def test_kernel_is_symmetric_positive_definite(kind):
    rng = np.random.default_rng(6)
    d, n = 2, 120
    x = rng.random((d, n))
    K = kernel([kind], rand_hp([kind], d, rng), x)
    assert np.array_equal(K, K.T)
    assert np.linalg.eigvalsh(K)[0] > 0.0
    sla.cholesky(K, lower=False)


@pytest.mark.parametrize("kind,w0", [(M32, 1.5), (M52, 5.0 / 6.0)])
def test_limit_at_zero_distance(kind, w0):
    """k(r -> 0) = sigma^2 and W(0) finite: 3/2 sigma^2 and 5/6 sigma^2; a D a few 1e-16 below
    zero (what the Gram form returns for coincident points) is clamped, not a NaN."""
    for D in (0.0, 1e-300, -3e-16):
        f, w = profile(kind, np.array([D]))
        assert f[0] == 1.0 and w[0] == w0
    f, w = profile(kind, np.array([1e-12]))
    assert abs(f[0] - 1.0) <= 2e-12 and abs(w[0] - w0) <= 4e-6  # 1 - W D + O(D^1.5), W'(0) ~ r
    x = np.array([[0.25, 0.25, 0.75]])
    K = kernel([kind], np.array([1.7, 2.0]), x, x.copy())
    assert K[0, 1] == 1.7 ** 2 and np.all(np.isfinite(K))


@pytest.mark.parametrize("kinds", [[SE], [SE, WN], [WN, SE], [SE, SE, WN], [SE, WN, SE]])
def test_agrees_with_the_oracle_for_se_and_noise(kinds):
    """The composition rules are the oracle's: every restated function, SE / WN parts only."""
    rng = np.random.default_rng(len(kinds) + 10 * (kinds[0] == WN))
    d, n, m = 3, 60, 25
    x, xp = rng.random((d, n)), rng.random((d, m))
    y = np.sin(x.sum(0)) ** 2
    hp = O.default_hp(kinds, d)
    hp[:] *= rng.uniform(0.8, 1.2, len(hp))
    assert np.array_equal(kernel(kinds, hp, x), O.kernel(kinds, hp, x))
    assert np.array_equal(kernel(kinds, hp, x, x), O.kernel(kinds, hp, x, x))
    assert np.array_equal(kernel(kinds, hp, x, xp), O.kernel(kinds, hp, x, xp))
    for i in range(1, len(hp) + 1):
        a, b = kernel_grad(kinds, i, hp, x), O.kernel_grad(kinds, i, hp, x)
        assert a == b if isinstance(a, tuple) else np.array_equal(a, b)
    assert diag_prior(kinds, hp, d) == O.diag_prior(kinds, hp, d)
    if WN not in kinds:
        return  # (the rest needs a well-conditioned K)
    assert mll(kinds, hp, x, y) == O.mll(kinds, hp, x, y)
    for log in (False, True):
        assert np.array_equal(mll_grad(kinds, hp, x, y, log_scale=log),
                              O.mll_grad(kinds, hp, x, y, log_scale=log))
    for diag in (True, False):
        for got, want in zip(predict(kinds, hp, x, y, xp, diag), O.predict(kinds, hp, x, y, xp, diag)):
            assert np.array_equal(got, want)
    cvset = O.kfoldcv(n, 15)
    assert np.array_equal(cv_batch(kinds, hp, "MSE", x, y, cvset),
                          O.cv_batch(kinds, hp, "MSE", x, y, cvset))


def test_mll_grad_by_central_differences():
    """The trace-formula gradient of a mixed description against differences of the MLL."""
    rng = np.random.default_rng(9)
    d, n, h = 2, 50, 1e-6
    x = rng.random((d, n))
    y = np.sin(x.sum(0)) ** 2
    kinds = [SE, M52, WN, M32]
    hp = rand_hp(kinds, d, rng, 0.5, 1.5)
    g = mll_grad(kinds, hp, x, y)
    for i in range(len(hp)):
        e = np.zeros(len(hp))
        e[i] = h
        fd = (mll(kinds, hp + e, x, y) - mll(kinds, hp - e, x, y)) / (2.0 * h)
        # u |MLL| / h ~ 1e-8 rounding of the quotient: 1e-6 of the gradient's scale
        assert abs(g[i] - fd) <= 1e-6 * (1.0 + np.abs(g).max())


# ---------------------------------------------------------------------------------------
# the Python description plumbing (no device)
# ---------------------------------------------------------------------------------------
def test_package_exports_the_matern_kinds():
    import gpr_amd as G
    from gpr_amd import _lib as L
    for name in ("Matern32", "Matern52"):
        assert hasattr(G, name) and name in G.__all__, name
    assert (G.Matern32.KIND, G.Matern52.KIND) == (L.GPR_M32, L.GPR_M52) == (3, 4)
    hdr = open(L.HEADER).read()
    assert "#define GPR_M32 3" in hdr and "#define GPR_M52 4" in hdr


def test_description_plumbing():
    import gpr_amd as G
    from gpr_amd import core
    cov = G.SquaredExp() + G.Matern52() + G.WhiteNoise() + G.Matern32()
    assert cov.kinds() == [1, 4, 2, 3]
    assert repr(cov) == "SquaredExp() + Matern52() + WhiteNoise() + Matern32()"
    assert repr(G.Matern32()) == "Matern32()" and repr(G.Matern52()) == "Matern52()"
    assert G.Matern52() == G.Matern52() and G.Matern52() != G.Matern32()
    assert G.Matern32() != G.SquaredExp() and G.SquaredExp() != G.Matern52()
    assert len({G.Matern32(), G.Matern32(), G.Matern52(), G.SquaredExp(), G.WhiteNoise()}) == 4
    d = 3
    assert G.dim_hp(G.Matern32(), d) == G.dim_hp(G.Matern52(), d) == d + 1
    assert G.dim_hp(cov, d) == 3 * (d + 1) + 1
    # hp index map: 1-based index -> (part, index in the part, offset of the part)
    assert core.find_idx(cov, 1, d) == (0, 1, 0)
    assert core.find_idx(cov, d + 1, d) == (0, d + 1, 0)
    assert core.find_idx(cov, d + 2, d) == (1, 1, d + 1)
    assert core.find_idx(cov, 2 * d + 3, d) == (2, 1, 2 * d + 2)
    assert core.find_idx(cov, 2 * d + 4, d) == (3, 1, 2 * d + 3)
    assert core.find_idx(cov, 3 * d + 4, d) == (3, d + 1, 2 * d + 3)
    with pytest.raises(IndexError):
        core.find_idx(cov, 3 * d + 5, d)
    hp = np.arange(1.0, 3 * d + 5)
    hps = core._part_hps(cov, hp, d)
    assert [len(h) for h in hps] == [d + 1, d + 1, 1, d + 1] and hps[3][0] == 2 * d + 4
    parts, kept = G.rm_noise(cov, hps)
    assert parts == [G.SquaredExp(), G.Matern52(), G.Matern32()] and len(kept) == 3
    mll_cost = G.MarginalLikelihood()
    for c, want in ((G.Matern32(), G.LogScale), (G.Matern52() + G.WhiteNoise(), G.LogScale),
                    (G.WhiteNoise() + G.Matern52(), G.LogScale), (G.WhiteNoise(), G.NoLogScale),
                    (G.SquaredExp(), G.LogScale)):
        assert isinstance(G.islog(mll_cost, types.SimpleNamespace(covar=c)), want)
    md = types.SimpleNamespace(covar=cov, params=hp)
    assert np.array_equal(G.init_params(mll_cost, md), np.ones(len(hp)))
