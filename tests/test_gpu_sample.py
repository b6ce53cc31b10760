"""GPU: GP sampling -- gpr_randn, gpr_mvn_sample, gpr_mvn_factor, gpr_sample_prior and the
Python layer above them (NormalDistribution, GaussianProcess, sample, sample_posterior;
src/distributions.jl).

Bounds (u = 2^-53):
  gpr_randn        |z - z_ref| <= 1e-13 max(1, r) against the NumPy restatement of
                   tests/test_sample_cpu.py (the project's K-assembly bar; the derived error of
                   log, sqrt and sin/cos is ~10 ulp of r), and 5-sigma moment bounds at N = 2^22
  gpr_mvn_sample   |S - (mu + triu(U)^T Z)| <= 4 n u (|U|^T |Z| + |mu|) elementwise: the
                   componentwise dot-product bound, once for each side of the comparison
  draws            ||S - S_ref||_F <= 8 n u kappa_2(K') ||U||_2 ||Z||_F with K' the matrix that is
                   factored: the forward error of a backward-stable Cholesky; kappa_2 is
                   computed in the test and asserted small enough for the bound to mean something
  factor           ||U^T U - K'||_F <= 8 n u ||K'||_F, and the same check against K and against
                   K + 1e-7 I must FAIL: the shift goes to every element (src/distributions.jl:21)
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import gpr_oracle as O
from test_sample_cpu import moment_bounds_hold, randn_ref

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

U53 = 2.0 ** -53
SHIFT = 1e-7
SE, WN = O.SE, O.WN


def _ctx():
    return G.default_context()


def _lib():
    from gpr_amd import _lib as L
    return L


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def cov_of(kinds):
    c = None
    for k in kinds:
        p = G.SquaredExp() if k == SE else G.WhiteNoise()
        c = p if c is None else c + p
    return c


def device_randn(seed, offset, count):
    ctx, L = _ctx(), _lib()
    Z = ctx.empty(count)
    assert L.lib.gpr_randn(ctx.h, seed, offset, _ptr(Z), count) == 0, L.lib.gpr_last_error(ctx.h)
    return ctx.host(Z)


# ---------------------------------------------------------------------------------------
# gpr_randn
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,offset,count", [(1, 0, 1), (1, 0, 2), (1, 1, 1), (7, 3, 1000),
                                               (2 ** 63 + 5, 2 ** 33 + 1, 4097)])
def test_randn_matches_the_restatement(seed, offset, count):
    z = device_randn(seed, offset, count)
    z_ref, r = randn_ref(seed, offset, count, with_r=True)
    err = np.abs(z - z_ref) / np.maximum(1.0, r)
    print(f"randn seed={seed} offset={offset} count={count}: max err / max(1, r) = {err.max():.3e}")
    assert np.all(np.isfinite(z))
    assert np.all(err <= 1e-13)


def test_randn_is_a_function_of_seed_and_global_index():
    a = device_randn(1, 0, 4099)
    assert np.array_equal(a, device_randn(1, 0, 4099))            # the same call twice
    parts = np.concatenate([device_randn(1, 0, 1001), device_randn(1, 1001, 3098)])
    assert np.array_equal(a, parts)                               # an odd split across a pair
    assert not np.array_equal(a, device_randn(2, 0, 4099))        # another seed


def test_randn_moments():
    z = device_randn(1, 0, 1 << 22)
    ok, (mean, var, tail) = moment_bounds_hold(z)
    print(f"gpr_randn, seed 1, N = 2^22: mean {mean:.3e} var-1 {var - 1:.3e} tail {tail:.6f}")
    assert ok, (mean, var, tail)


# ---------------------------------------------------------------------------------------
# gpr_mvn_sample
# ---------------------------------------------------------------------------------------
def _padded(a, ld, fill):
    """Column-major device copy of the (rows, cols) array `a` with leading dimension ld; the
    padding rows hold `fill`."""
    buf = np.full((ld, a.shape[1]), fill)
    buf[:a.shape[0]] = a
    return _ctx().colmajor(buf)


def _mvn(dU, n, ldu, dmu, dZ, ns, ldz, dS, lds):
    ctx, L = _ctx(), _lib()
    return L.lib.gpr_mvn_sample(ctx.h, _ptr(dU), n, ldu, _ptr(dmu), _ptr(dZ), ns, ldz, _ptr(dS), lds)


def _check_mvn(n, ns, ldu, ldz, lds, with_mu, seed):
    rng = np.random.default_rng(seed)
    U = np.triu(rng.standard_normal((n, n)))
    U[np.diag_indices(n)] = rng.uniform(1.0, 2.0, n)
    buf = U.copy()
    buf[np.tril_indices(n, -1)] = np.nan          # the factor buffer's strict lower triangle
    Z = rng.standard_normal((n, ns))
    mu = rng.standard_normal(n) if with_mu else None
    ctx = _ctx()
    dU, dZ = _padded(buf, ldu, np.nan), _padded(Z, ldz, np.nan)
    dS = _padded(np.full((n, ns), -7.0), lds, -7.0)
    dmu = ctx.colmajor(mu) if with_mu else None
    assert _mvn(dU, n, ldu, dmu, dZ, ns, ldz, dS, lds) == 0, _lib().lib.gpr_last_error(ctx.h)
    out = ctx.host(dS)
    S = out[:n]
    assert np.all(np.isfinite(S))
    assert np.all(out[n:] == -7.0)                # nothing written past row n
    m0 = np.zeros(n) if mu is None else mu
    ref = U.T @ Z + m0[:, None]
    bound = 4.0 * n * U53 * (np.abs(U).T @ np.abs(Z) + np.abs(m0)[:, None])
    ratio = (np.abs(S - ref) / bound).max()
    print(f"mvn_sample n={n} ns={ns} mu={with_mu}: max |err| / bound = {ratio:.3e}")
    assert ratio <= 1.0


@pytest.mark.parametrize("with_mu", [True, False])
@pytest.mark.parametrize("ns", [1, 3, 128, 130])
@pytest.mark.parametrize("n", [1, 16, 127, 128, 129, 300])
def test_mvn_sample_nan_below_the_diagonal(n, ns, with_mu):
    _check_mvn(n, ns, n + 3, n + 1, n + 1, with_mu, seed=1000 * n + 2 * ns + with_mu)


@pytest.mark.parametrize("n,ns", [(256, 5), (400, 130), (1040, 7)])
def test_mvn_sample_nan_below_the_diagonal_aligned_operands(n, ns):
    """Even leading dimensions and 16-B aligned operands take the 16-B staged loads (n = 256)
    and, above 256, the two-launch form: rows above the diagonal tiles through the pipelined
    kernel, the diagonal tiles masked.  n = 1040: a ragged last tile row."""
    _check_mvn(n, ns, n, n, n, True, seed=n + ns)


def test_mvn_sample_rejects_aliased_output():
    ctx, L = _ctx(), _lib()
    n, ns = 32, 4
    dU = ctx.colmajor(np.triu(np.ones((n, n))) + np.eye(n))
    dZ = ctx.zeros(ns, n)
    assert _mvn(dU, n, n, None, dZ, ns, n, dZ, n) == -1          # GPR_E_ARG: dS == dZ
    dB = ctx.zeros(2 * ns, n)                                      # dS overlapping dZ's tail
    dS = dB[ns - 1:]
    assert _mvn(dU, n, n, None, dB, ns, n, dS, n) == -1
    assert b"overlap" in L.lib.gpr_last_error(ctx.h)


def test_mvn_sample_from_a_real_factor_leaves_the_buffer_alone():
    """U from gpr_potrf_upper at n = 384: the strict lower triangle of the buffer holds K."""
    ctx, L = _ctx(), _lib()
    n, ns = 384, 6
    rng = np.random.default_rng(384)
    A = rng.standard_normal((n, n))
    K = A @ A.T / n + np.eye(n)
    dK = ctx.colmajor(K)
    info = ctypes.c_int(0)
    assert L.lib.gpr_potrf_upper(ctx.h, _ptr(dK), n, n, ctypes.byref(info)) == 0 and info.value == 0
    before = ctx.host(dK)
    assert np.array_equal(np.tril(before, -1), np.tril(K, -1))    # K below the diagonal
    Z = rng.standard_normal((n, ns))
    mu = rng.standard_normal(n)
    dZ, dmu, dS = ctx.colmajor(Z), ctx.colmajor(mu), ctx.empty(ns, n)
    assert _mvn(dK, n, n, dmu, dZ, ns, n, dS, n) == 0
    S = ctx.host(dS)
    assert np.array_equal(ctx.host(dK), before)                   # the factor buffer is read only
    U = np.triu(before)
    bound = 4.0 * n * U53 * (np.abs(U).T @ np.abs(Z) + np.abs(mu)[:, None])
    ratio = (np.abs(S - (U.T @ Z + mu[:, None])) / bound).max()
    print(f"mvn_sample, potrf factor n={n}: max |err| / bound = {ratio:.3e}")
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------------
# draws: sample(gp(x, theta), z = z), NormalDistribution(mu, Sigma), sample_posterior
# ---------------------------------------------------------------------------------------
def _draw_bound(Kp, Z, kappa_max):
    """(reference factor L, 8 n u kappa_2(K') ||U||_2 ||Z||_F), kappa_2 asserted < kappa_max."""
    n = Kp.shape[0]
    w = np.linalg.eigvalsh(Kp)
    kappa = w[-1] / w[0]
    assert 0.0 < w[0] and kappa < kappa_max, f"kappa_2 = {kappa:.3e}: the bound would be empty"
    Lc = np.linalg.cholesky(Kp)
    return Lc, 8.0 * n * U53 * kappa * np.sqrt(w[-1]) * np.linalg.norm(Z), kappa


@functools.lru_cache(maxsize=None)
def _prior_case(name, n):
    kinds = {"SE+WN": (SE, WN), "SE+SE+WN": (SE, SE, WN)}[name]
    d = 2
    rng = np.random.default_rng(17 * n + len(kinds))
    x = rng.random((d, n))
    hp = rng.uniform(0.3, 2.0, sum(O.dim_hp(k, d) for k in kinds))
    Kp = O.kernel(list(kinds), hp, x) + SHIFT       # the 4-arg kernel, every element shifted
    z = rng.standard_normal((n, 5))
    for a in (x, hp, Kp, z):
        a.setflags(write=False)
    return list(kinds), x, hp, Kp, z


@pytest.mark.parametrize("n_samples", [1, 5])
@pytest.mark.parametrize("n", [64, 200, 384])
@pytest.mark.parametrize("name", ["SE+WN", "SE+SE+WN"])
def test_sample_prior_with_given_z(name, n, n_samples):
    kinds, x, hp, Kp, z5 = _prior_case(name, n)
    z = z5[:, :n_samples]
    mu = x.sum(axis=0)
    Lc, bound, kappa = _draw_bound(Kp, z, 1e6)
    S_ref = Lc @ z + mu[:, None]
    gp = G.GaussianProcess(lambda c: c.sum(), cov_of(kinds))
    S = G.sample(gp(x, hp), z=z)
    assert S.shape == (n, n_samples)
    err = np.linalg.norm(S - S_ref)
    print(f"prior {name} n={n} ns={n_samples}: kappa {kappa:.2e} err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    if n_samples == 1:                                 # the vector forms: sample(gp, x, theta)
        s = G.sample(gp, x, hp, z=z[:, 0])
        assert s.shape == (n,) and np.array_equal(s, S[:, 0])


@pytest.mark.parametrize("n", [128, 200])
def test_single_se_factor_pins_the_all_elements_shift(n):
    d = 2
    rng = np.random.default_rng(n)
    x = rng.random((d, n))
    hp = rng.uniform(0.3, 2.0, d + 1)
    N = G.GaussianProcess(lambda c: 0.0, G.SquaredExp())(x, hp)
    U = N.Sigma_ch
    assert np.array_equal(U, np.triu(U))
    K = O.kernel([SE], hp, x)
    R = U.T @ U

    def ok(M):
        return np.linalg.norm(R - M) <= 8.0 * n * U53 * np.linalg.norm(M)

    print(f"single SE n={n}: ||U'U - K'|| / (8 n u ||K'||) = "
          f"{np.linalg.norm(R - (K + SHIFT)) / (8.0 * n * U53 * np.linalg.norm(K + SHIFT)):.3e}")
    assert ok(K + SHIFT)
    assert not ok(K)
    assert not ok(K + SHIFT * np.eye(n))
    np.testing.assert_allclose(N.Sigma, K, rtol=1e-13, atol=1e-15)   # .Sigma is the unshifted K


def test_normal_distribution_from_a_host_sigma():
    n, d = 200, 2
    kinds, x, hp, Kp, z5 = _prior_case("SE+WN", n)
    Sigma = O.kernel(kinds, hp, x)
    mu = np.cos(np.arange(n, dtype=float))
    N = G.NormalDistribution(mu, Sigma)
    assert np.array_equal(N.mu, mu) and N.Sigma is not None and N.dim == n
    Lc, bound, _ = _draw_bound(Kp, z5, 1e6)
    S = G.sample(N, z=z5)
    err = np.linalg.norm(S - (Lc @ z5 + mu[:, None]))
    print(f"NormalDistribution n={n}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    bad = np.eye(n)
    bad[5, 5] = -1.0                                  # the leading minor of order 6 fails
    with pytest.raises(G.PosDefException) as e:
        G.NormalDistribution(mu, bad)
    assert e.value.info == 6


@functools.lru_cache(maxsize=None)
def _posterior_case():
    d, n, m = 2, 128, 96
    rng = np.random.default_rng(12896)
    x, xp = rng.random((d, n)), rng.random((d, m))
    y = np.sin(3.0 * x[0]) + x[1] ** 2 + 0.1 * rng.standard_normal(n)
    hp = np.array([1.0, 1.5, 0.8, 0.5])              # sigma, l_1, l_2, sigma_n
    z = rng.standard_normal((m, 4))
    for a in (x, xp, z):      # (the 1-D y and hp are uploaded as they are: kept writable)
        a.setflags(write=False)
    return x, xp, y, hp, z


def test_sample_posterior():
    x, xp, y, hp, z = _posterior_case()
    m, jitter = xp.shape[1], 1e-6
    kinds = [SE, WN]
    md = G.GPRModel(cov_of(kinds), hp, x, y)
    # precondition on the oracle's Sigma_p, checkable without a GPU
    _, Sp_o = O.predict(kinds, hp, x, y, xp, diagonal_var=False)
    w = np.linalg.eigvalsh(Sp_o + SHIFT + jitter * np.eye(m))
    assert w[0] > 0.0 and w[-1] / w[0] < 1e8
    mu_p, Sp = G.predict(md, xp)
    Lc, bound, kappa = _draw_bound(Sp + SHIFT + jitter * np.eye(m), z, 1e8)
    S = G.sample_posterior(md, xp, z=z, jitter=jitter)
    assert S.shape == (m, 4)
    err = np.linalg.norm(S - (mu_p[:, None] + Lc @ z))
    print(f"sample_posterior m={m}: kappa {kappa:.2e} err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    for j in range(4):                                 # columns are independent draws
        sj = G.sample_posterior(md, xp, z=z[:, j], jitter=jitter)
        assert sj.shape == (m, 1) and np.array_equal(sj[:, 0], S[:, j])


def test_sample_posterior_default_seed_is_repeatable():
    x, xp, y, hp, _ = _posterior_case()
    md = G.GPRModel(cov_of([SE, WN]), hp, x, y)
    a = G.sample_posterior(md, xp, n_samples=3, jitter=1e-6)
    assert a.shape == (xp.shape[1], 3) and np.all(np.isfinite(a))
    assert np.array_equal(a, G.sample_posterior(md, xp, n_samples=3, jitter=1e-6))   # seed = 1
    assert not np.array_equal(a, G.sample_posterior(md, xp, n_samples=3, jitter=1e-6, seed=2))
    # the draw is mu_p + L z with z = gpr_randn(1, 0, m * 3), column-major
    # (both draws use the same device factor L; they differ by L dz with |dz| <= 1e-13 max(1, r),
    # the generator's bound, and by the rounding of the two products, 4 m u |L| |z| each)
    m = xp.shape[1]
    zz, r = randn_ref(1, 0, a.size, with_r=True)
    zz, r = zz.reshape(3, m).T, r.reshape(3, m).T
    b = G.sample_posterior(md, xp, z=zz, jitter=1e-6)
    _, Sp = G.predict(md, xp)
    Labs = np.abs(np.linalg.cholesky(Sp + SHIFT + 1e-6 * np.eye(m)))
    tol = Labs @ (1e-13 * np.maximum(1.0, r)) + 8.0 * m * U53 * (Labs @ np.abs(zz))
    assert np.all(np.abs(a - b) <= tol)
