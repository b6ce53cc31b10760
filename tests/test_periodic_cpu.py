"""CPU: the Periodic kernel restated in NumPy, and the description plumbing.

The reference has no periodic kernel, so the definition of include/gpr_hip.h is the contract and
this restatement is its checker (tests/test_gpu_periodic.py imports it).  It is written in the
difference form, feature by feature,

    D = sum_k (2 l_k sin(pi (x_k - x'_k) / p_k))^2,   k = s^2 exp(-D),   hp = [s, l_1..l_d, p_1..p_d]

and composes parts exactly as tests/test_matern_cpu.py does (whose SquaredExp / Matern / WhiteNoise
parts it reuses): parts summed in `+` order, eps once per stationary part on a same-object
diagonal, the first WhiteNoise's sigma_n^2 only in the 4-arg form, and

    dK/ds   = (2/|s|) K_p                      (K_p with eps)
    dK/dl_k = -2 l_k K (2 sin(pi r_k / p_k))^2
    dK/dp_k = (4 pi l_k^2 / p_k^2) K r_k sin(2 pi r_k / p_k)     r = x - x' on raw x, K without eps.

For descriptions of SquaredExp / WhiteNoise parts it must agree with oracle/gpr_oracle.py; the
Periodic part is pinned by finite differences of its derivatives, by the embedding identity (it
is the oracle's SquaredExp on the 2d features [cos, sin](2 pi x / p) with l duplicated), by its
periodicity and by its evenness in p.
"""
import types

import numpy as np
import pytest

import test_matern_cpu as M
from oracle import gpr_oracle as O
from test_matern_cpu import M32, M52, SE, WN

PER = "PER"
EPS = 1e-8
KIND_CODE = dict(M.KIND_CODE, **{PER: 5})


# ---------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------
def stationary(kind):
    return kind != WN


def dim_hp(kind, d):
    return 1 if kind == WN else 2 * d + 1 if kind == PER else d + 1


def split_hp(kinds, hp, d):
    dims = [dim_hp(k, d) for k in kinds]
    assert sum(dims) == len(hp), "Parameter size mismatch."
    out, c = [], 0
    for n in dims:
        out.append(np.asarray(hp[c:c + n], dtype=np.float64))
        c += n
    return out


def periodic_distance(ls, ps, x, xp):
    """D[a, b] = sum_k (2 l_k sin(pi (x_ka - x'_kb) / p_k))^2, feature by feature."""
    D = np.zeros((x.shape[1], xp.shape[1]))
    for k in range(x.shape[0]):
        c = 2.0 * ls[k] * np.sin(np.pi * (x[k][:, None] - xp[k][None, :]) / ps[k])
        D += c * c
    return D


def part_kernel(kind, hp, x, xp, same, eps=EPS, want_w=False):
    if kind != PER:
        return M.part_kernel(kind, hp, x, xp, same, eps, want_w)
    d = x.shape[0]
    sigma, ls, ps = hp[0], hp[1:d + 1], hp[d + 1:]
    f = np.exp(-1.0 * periodic_distance(ls, ps, x, xp))
    K = (sigma ** 2) * f
    if same:
        K[np.diag_indices(K.shape[0])] += eps
    return (K, (sigma ** 2) * f) if want_w else K


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


def find_idx(kinds, i, d):
    """1-based i -> (part, 1-based index inside the part)."""
    dims = np.cumsum([dim_hp(k, d) for k in kinds])
    kidx = int(np.searchsorted(dims, i))
    return kidx, int(i if kidx == 0 else i - dims[kidx - 1])


def kernel_grad(kinds, i, hp, x, eps=EPS):
    """1-based i; WhiteNoise -> ("I", 2 sigma_n) as the oracle."""
    d = x.shape[0]
    hps = split_hp(kinds, hp, d)
    kidx, hpidx = find_idx(kinds, i, d)
    part = hps[kidx]
    if kinds[kidx] == WN:
        return ("I", 2.0 * part[0])
    Kp, W = part_kernel(kinds[kidx], part, x, x, True, eps, want_w=True)
    if hpidx == 1:
        return (2.0 / abs(part[0])) * Kp
    k = (hpidx - 2) % d
    r = x[k][:, None] - x[k][None, :]
    if kinds[kidx] != PER:
        return -2.0 * part[hpidx - 1] * W * r ** 2
    l, p = part[1 + k], part[1 + d + k]
    if hpidx <= d + 1:
        return -2.0 * l * W * (2.0 * np.sin(np.pi * r / p)) ** 2
    return (4.0 * np.pi * l * l / (p * p)) * W * r * np.sin(2.0 * np.pi * r / p)


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
    import scipy.linalg as sla
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


def embed(x, ps):
    """u(x) = [cos(2 pi x_k / p_k) | sin(2 pi x_k / p_k)], 2d x n."""
    a = 2.0 * np.pi * x / np.asarray(ps)[:, None]
    return np.vstack([np.cos(a), np.sin(a)])


def model_hp(kinds, d, rng, lscale=0.75, noise=0.1):
    """sigma near 1, l_k = lscale sqrt(8/d) varied per part, distinct p_k in [0.4, 2.0]."""
    hp, p = [], 0
    for k in kinds:
        if k == WN:
            hp += [noise]
            continue
        hp += [1.0 - 0.1 * p] + list(lscale * np.sqrt(8.0 / d) * (1.0 + 0.2 * p) * rng.uniform(0.9, 1.1, d))
        if k == PER:
            hp += list(rng.permutation(np.linspace(0.4, 2.0, d + 2)[1:-1]) if d > 1 else [0.9])
        p += 1
    return np.array(hp)


# ---------------------------------------------------------------------------------------
# the restatement's own checks
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [[SE], [SE, WN], [WN, SE], [SE, SE, WN], [SE, WN, SE]])
def test_agrees_with_the_oracle_for_se_and_noise(kinds):
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
        return
    assert mll(kinds, hp, x, y) == O.mll(kinds, hp, x, y)
    for log in (False, True):
        assert np.array_equal(mll_grad(kinds, hp, x, y, log_scale=log),
                              O.mll_grad(kinds, hp, x, y, log_scale=log))
    for diag in (True, False):
        for got, want in zip(predict(kinds, hp, x, y, xp, diag), O.predict(kinds, hp, x, y, xp, diag)):
            assert np.array_equal(got, want)


@pytest.mark.parametrize("d", [1, 3, 8])
def test_kernel_grad_by_central_differences(d):
    """dK/dsigma, dK/dl_k, dK/dp_k against (K(h+) - K(h-)) / 2h, h = 1e-6.  Bound 1e-8: the
    rounding of the quotient is ~ u |K| / h = 1e-10 per entry, its truncation h^2 |K'''| / 6 with
    |K'''| up to ~ (2 pi l / p)^3 (|x - x'| / p)^3 ~ 1e4 at the smallest period: 2e-9."""
    rng = np.random.default_rng(5 + d)
    n, h = 40, 1e-6
    x = rng.random((d, n))
    kinds = [PER]
    hp = model_hp(kinds, d, rng, lscale=0.5)
    for i in range(1, 2 * d + 2):
        e = np.zeros(2 * d + 1)
        e[i - 1] = h
        fd = (kernel(kinds, hp + e, x) - kernel(kinds, hp - e, x)) / (2.0 * h)
        if i == 1:  # the rule's K_p carries eps on the diagonal, which no derivative of K has
            fd[np.diag_indices(n)] += (2.0 / abs(hp[0])) * EPS
        err = np.abs(kernel_grad(kinds, i, hp, x) - fd).max()
        print(f"d={d} hp index {i}: max |analytic - FD| = {err:.2e}")
        assert err <= 1e-8


def test_mll_grad_by_central_differences():
    """The trace-formula gradient of a mixed description against differences of the MLL."""
    rng = np.random.default_rng(9)
    d, n, h = 2, 50, 1e-6
    x = rng.random((d, n))
    y = np.sin(x.sum(0)) ** 2
    kinds = [SE, PER, WN, M52]
    hp = model_hp(kinds, d, rng, lscale=0.3, noise=0.3)
    g = mll_grad(kinds, hp, x, y)
    for i in range(len(hp)):
        e = np.zeros(len(hp))
        e[i] = h
        fd = (mll(kinds, hp + e, x, y) - mll(kinds, hp - e, x, y)) / (2.0 * h)
        # u |MLL| / h ~ 1e-8 rounding of the quotient: 1e-6 of the gradient's scale
        assert abs(g[i] - fd) <= 1e-6 * (1.0 + np.abs(g).max())


@pytest.mark.parametrize("d", [1, 3, 8, 33])
def test_embedding_identity(d):
    """Periodic(x; s, l, p) is the oracle's SquaredExp on the 2d embedded inputs with l
    duplicated: 2 l sin(pi r / p) is the chord between (cos a, sin a) and (cos b, sin b).
    Both sides carry ~ (2d + 2) u D of rounding in D <= 4 sum l^2 = 18 here: rtol 1e-13."""
    rng = np.random.default_rng(d)
    n, m = 50, 30
    x, xp = rng.random((d, n)), rng.random((d, m))
    hp = model_hp([PER], d, rng)
    s, ls, ps = hp[0], hp[1:d + 1], hp[d + 1:]
    hpe = np.concatenate([[s], ls, ls])
    np.testing.assert_allclose(kernel([PER], hp, x, xp), O.kernel([SE], hpe, embed(x, ps), embed(xp, ps)),
                               rtol=1e-13, atol=0)
    np.testing.assert_allclose(kernel([PER], hp, x), O.kernel([SE], hpe, embed(x, ps)), rtol=1e-13, atol=0)


def test_periodicity():
    """Shifting xp by integer multiples m <= 3 of p_k in some dimensions leaves K unchanged.
    Bound: the shifted angle pi (r + m p) / p carries an error u 2 pi (|x| / p + m) (the sum
    x + m p and the division are rounded), which enters D times 4 sum_k l_k^2 = 18: with
    |x| / p <= 2.5 and m = 3 about 7e-14 relative in K; asserted at rtol 1e-12."""
    rng = np.random.default_rng(21)
    d, n, m = 4, 40, 30
    x, xp = rng.random((d, n)), rng.random((d, m))
    hp = model_hp([PER], d, rng)
    ps = hp[d + 1:]
    K = kernel([PER], hp, x, xp)
    for shift in ([1, 0, 0, 0], [0, -2, 3, 0], [3, 3, -3, 1]):
        xs = xp + (np.array(shift) * ps)[:, None]
        np.testing.assert_allclose(kernel([PER], hp, x, xs), K, rtol=1e-12, atol=0)


def test_even_in_the_period():
    rng = np.random.default_rng(22)
    d, n = 3, 40
    x = rng.random((d, n))
    hp = model_hp([SE, PER, WN], d, rng)
    hm = hp.copy()
    hm[d + 1 + d + 1:d + 1 + 2 * d + 1] *= -1.0
    assert np.array_equal(kernel([SE, PER, WN], hp, x), kernel([SE, PER, WN], hm, x))
    for i in (1, d + 2, d + 3):  # sigma and l entries: even; p entries: odd
        assert np.array_equal(kernel_grad([SE, PER, WN], i, hp, x), kernel_grad([SE, PER, WN], i, hm, x))
    i = 2 * d + 3
    np.testing.assert_array_equal(kernel_grad([SE, PER, WN], i, hp, x), -kernel_grad([SE, PER, WN], i, hm, x))


def test_kernel_is_symmetric_positive_definite():
    rng = np.random.default_rng(6)
    d, n = 2, 120
    x = rng.random((d, n))
    K = kernel([PER, WN], model_hp([PER, WN], d, rng, lscale=0.3), x)
    assert np.array_equal(K, K.T)
    assert np.linalg.eigvalsh(K)[0] > 0.0


# ---------------------------------------------------------------------------------------
# the Python description plumbing (no device)
# ---------------------------------------------------------------------------------------
def test_package_exports_the_periodic_kind():
    import gpr_amd as G
    from gpr_amd import _lib as L
    assert hasattr(G, "Periodic") and "Periodic" in G.__all__
    assert G.Periodic.KIND == L.GPR_PER == 5
    assert "#define GPR_PER 5" in open(L.HEADER).read()
    assert G.is_stationary(G.Periodic()) is True


def test_description_plumbing():
    import gpr_amd as G
    from gpr_amd import core
    d = 3
    cov = G.SquaredExp() + G.Periodic() + G.WhiteNoise()
    assert cov.kinds() == [1, 5, 2] and repr(cov) == "SquaredExp() + Periodic() + WhiteNoise()"
    assert G.Periodic() == G.Periodic() and G.Periodic() != G.SquaredExp()
    assert len({G.Periodic(), G.Periodic(), G.SquaredExp()}) == 2
    assert G.dim_hp(G.Periodic(), d) == 2 * d + 1
    assert G.dim_hp(cov, d) == (d + 1) + (2 * d + 1) + 1
    assert core.find_idx(cov, d + 1, d) == (0, d + 1, 0)
    assert core.find_idx(cov, d + 2, d) == (1, 1, d + 1)
    assert core.find_idx(cov, 3 * d + 2, d) == (1, 2 * d + 1, d + 1)
    assert core.find_idx(cov, 3 * d + 3, d) == (2, 1, 3 * d + 2)
    with pytest.raises(IndexError):
        core.find_idx(cov, 3 * d + 4, d)
    hp = np.arange(1.0, 3 * d + 4)
    hps = core._part_hps(cov, hp, d)
    assert [len(h) for h in hps] == [d + 1, 2 * d + 1, 1] and hps[2][0] == 3 * d + 3
    parts, kept = G.rm_noise(cov, hps)
    assert parts == [G.SquaredExp(), G.Periodic()] and [len(h) for h in kept] == [d + 1, 2 * d + 1]
    # the other mixed descriptions of the issue, against the restatement's own map
    for kinds, c in (([PER, M52], G.Periodic() + G.Matern52()), ([WN, PER], G.WhiteNoise() + G.Periodic())):
        D = sum(dim_hp(k, d) for k in kinds)
        assert G.dim_hp(c, d) == D
        assert [len(h) for h in core._part_hps(c, np.zeros(D), d)] == [dim_hp(k, d) for k in kinds]
        for i in range(1, D + 1):
            p, loc, _ = core.find_idx(c, i, d)
            assert (p, loc) == find_idx(kinds, i, d)
    mll_cost = G.MarginalLikelihood()
    for c in (G.Periodic(), G.Periodic() + G.WhiteNoise(), G.WhiteNoise() + G.Periodic()):
        assert isinstance(G.islog(mll_cost, types.SimpleNamespace(covar=c)), G.LogScale)
    md = types.SimpleNamespace(covar=cov, params=hp)
    assert np.array_equal(G.init_params(mll_cost, md), np.ones(len(hp)))
