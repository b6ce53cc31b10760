"""GPU: gpr_rff_draw / gpr_rff_matmul against the header's definition in long double, the law of
the drawn frequencies against the exact kernels, and sample_paths against Matheron's formula.

Product bound, per element of Out (u = 2^-53, derived in the issue and in DESIGN 3.21):
    sum_p (|sigma_p| / sqrt(F)) sum_j (|A| + |B|)_jc (2 pi (4 ceil(d/4) + 1) u sum_k |Omega_jk l_k x_k| + C u)
    + (2 nse F + 2) u sum |terms|
-- the projection's rounding through the derivative 2 pi, the sincos polynomial (C = 2 C_POLY: the
NumPy restatement's measured 1.41 u, doubled because the device fuses its multiply-adds), and the
second product's accumulation with the two roundings of the folded sigma_p / sqrt(F)."""
import numpy as np
import pytest

import kernel_ref_ld as R
import test_product_cpu as PR
from kernel_ref_ld import LD, M32, M52, PER, SE, U, WN
from test_rff_cpu import C_POLY

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")
from gpr_amd import _lib, core  # noqa: E402
from oracle import gpr_oracle as O  # noqa: E402

DESCS = {"SE": [SE], "M32": [M32], "M52": [M52], "SE+WN": [SE, WN], "SE+M52+WN": [SE, M52, WN]}


def _parts(desc, hp, d):
    return [h for t in R.split_hp(desc, hp, d) for k, h in t if k != WN]


def _hp(desc, d, rng):
    return rng.uniform(0.3, 2.0, sum(R.width(k, d) for k in R.flat(desc)))


def _draw(desc, d, F, seed=7):
    """Omega on the device and as host blocks [part][F x d]"""
    ctx = core.default_context()
    kinds, nk = core._kinds_arr(PR.cov_of(desc))
    nse = sum(k != WN for k in R.flat(desc))
    dOm = ctx.empty(nse * F * d)
    ctx.check(_lib.lib.gpr_rff_draw(ctx.h, kinds, nk, d, F, seed, core._ptr(dOm)), "gpr_rff_draw")
    return dOm, [b.reshape(d, F).T for b in ctx.host(dOm).reshape(nse, F * d)]


def _matmul(desc, hp, x, dOm, F, W, dOut=None):
    """(rc, Out n x ns) of gpr_rff_matmul, unchecked"""
    ctx = core.default_context()
    kinds, nk = core._kinds_arr(PR.cov_of(desc))
    _, hpp = core._hp_arr(hp)
    dx, dW = ctx.colmajor(x), ctx.colmajor(W)
    n, ns = x.shape[1], W.shape[1]
    dOut = ctx.empty(ns, n) if dOut is None else dOut
    rc = _lib.lib.gpr_rff_matmul(ctx.h, kinds, nk, hpp, x.shape[0], core._ptr(dx), n, core._ptr(dOm),
                                 F, core._ptr(dW), ns, W.shape[0], core._ptr(dOut), n)
    return rc, ctx.host(dOut)


def _prior_ld(desc, hp, x, Om, W, bound=False):
    """f_prior(x) (n x ns, long double) and, if asked, its element bound"""
    d, F = x.shape[0], Om[0].shape[0]
    parts = _parts(desc, hp, d)
    out = np.zeros((x.shape[1], W.shape[1]), dtype=LD)
    e1 = np.zeros_like(out)
    terms = np.zeros_like(out)
    Wl = W.astype(LD)
    for p, h in enumerate(parts):
        s = LD(h[0]) / np.sqrt(LD(F))
        xs = (LD(1) * h[1:d + 1, None]) * x.astype(LD)
        t = Om[p].astype(LD) @ xs
        a = 2 * R.PI_LD * (t - np.rint(t))
        A, B = Wl[2 * p * F:(2 * p + 1) * F], Wl[(2 * p + 1) * F:(2 * p + 2) * F]
        out += s * (np.cos(a).T @ A + np.sin(a).T @ B)
        if bound:
            tabs = np.abs(Om[p]).astype(LD) @ np.abs(xs)
            err = 2 * R.PI_LD * (4 * ((d + 3) // 4) + 1) * U * tabs + 2 * C_POLY * U
            e1 += abs(s) * (err.T @ (np.abs(A) + np.abs(B)))
            terms += abs(s) * (np.abs(np.cos(a)).T @ np.abs(A) + np.abs(np.sin(a)).T @ np.abs(B))
    return (out, e1 + (2 * len(parts) * F + 2) * U * terms) if bound else out


# every value of each axis meets at least two values of each other axis; one case forces S > 1
CASES = [("SE", 1, 1, 1, 1, 0), ("SE", 8, 64, 64, 16, 0), ("M32", 9, 65, 65, 17, 0),
         ("M32", 21, 130, 200, 65, 0), ("SE+M52+WN", 1, 130, 64, 17, 3),
         ("SE+M52+WN", 8, 65, 200, 1, 0), ("SE+M52+WN", 21, 1, 65, 65, 0),
         ("SE", 21, 64, 1, 65, 0), ("M32", 9, 130, 1, 16, 0)]


@pytest.mark.parametrize("name,d,n,F,ns,slabs", CASES)
def test_product_against_the_definition(knobs, name, d, n, F, ns, slabs):
    desc = DESCS[name]
    rng = np.random.default_rng(1000 * d + n + F + ns)
    hp, x = _hp(desc, d, rng), rng.random((d, n))
    dOm, Om = _draw(desc, d, F)
    W = rng.standard_normal((2 * len(Om) * F, ns))
    knobs("GPR_RFF_SLABS", slabs)
    rc, out = _matmul(desc, hp, x, dOm, F, W)
    assert rc == 0
    ref, bound = _prior_ld(desc, hp, x, Om, W, bound=True)
    ratio = float((np.abs(out.astype(LD) - ref) / bound).max())
    print(f"max |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("kind", [SE, M32, M52])
def test_draw_has_the_kernels_law(kind):
    """k^(x_a, x_0) = (sigma^2 / F) sum_j cos(2 pi (t_j(x_a) - t_j(x_0))) within 0.02 sigma^2 of k at
    64 distances r in [0, 2]: Hoeffding puts a correct draw's chance of missing below 1e-9 at
    F = 2^17; a swapped Matern law misses by 0.049."""
    d, F, desc = 3, 1 << 17, [kind]
    rng = np.random.default_rng(5)
    hp = _hp(desc, d, rng)
    x0 = rng.random((d, 1))
    u = rng.standard_normal(d)
    x = x0 + (np.linspace(0.0, 2.0, 64)[None, :] * (u / np.linalg.norm(u) / hp[1:])[:, None])
    dOm, Om = _draw(desc, d, F, seed=11)
    a0 = 2 * np.pi * (Om[0] @ (hp[1:, None] * x0))
    W = hp[0] / np.sqrt(F) * np.vstack([np.cos(a0), np.sin(a0)])
    rc, out = _matmul(desc, hp, x, dOm, F, W)
    assert rc == 0
    k = R.kernel_ld(desc, hp, x, x0).astype(np.float64)
    err = np.abs(out.reshape(-1) - k.reshape(-1)).max() / hp[0] ** 2
    print(f"max |k^ - k| / sigma^2 = {err:.2e}")
    assert err <= 0.02


@pytest.mark.parametrize("solver", ["factor", "cg"])
@pytest.mark.parametrize("name", ["SE+WN", "SE+M52+WN"])
def test_paths_against_the_formula(name, solver):
    desc, d, n, m, ns = DESCS[name], 2, 130, 70, 3
    x, y, xp = O.synthetic(d, n, m)
    hp = np.random.default_rng(n + m).uniform(0.5, 1.5, sum(R.width(k, d) for k in R.flat(desc)))
    hp[-1] = 0.3  # sigma_n
    md = G.GPRModel(PR.cov_of(desc), hp, x, y)
    paths = G.sample_paths(md, n_samples=ns, n_features=256, seed=3, solver=solver)
    ctx = md.ctx
    F, nse = 256, len(_parts(desc, hp, d))
    Om = [b.reshape(d, F).T for b in ctx.host(paths.omega).reshape(nse, F * d)]
    W, noise = ctx.host(paths.weights), ctx.host(paths.noise)
    K = R.kernel_ld(desc, hp, x).astype(np.float64)
    Kpx = R.kernel_ld(desc, hp, xp, x).astype(np.float64)
    Rm = y[:, None] - _prior_ld(desc, hp, x, Om, W).astype(np.float64) - noise
    ref = _prior_ld(desc, hp, xp, Om, W).astype(np.float64) + Kpx @ np.linalg.solve(K, Rm)
    got = paths(xp)
    tol = 1e-8 * np.abs(ref) + 1e-10
    if solver == "cg":
        tol = tol + np.linalg.norm(Kpx, 2) * paths.relres * np.linalg.norm(Rm, axis=0) / hp[-1] ** 2
    print(f"max |err| / tol = {(np.abs(got - ref) / tol).max():.3g}")
    assert got.shape == (m, ns) and np.all(np.abs(got - ref) <= tol)
    assert np.array_equal(paths(xp), got)
    assert np.array_equal(np.vstack([paths(xp[:, :35]), paths(xp[:, 35:])]), got)


def test_refusals_and_repeatability():
    d, n, F, ns = 3, 70, 200, 2
    rng = np.random.default_rng(9)
    x, W = rng.random((d, n)), rng.standard_normal((2 * F, ns))
    dOm, Om = _draw([SE], d, F)
    ctx = core.default_context()
    for desc in ([PER], [[SE, PER], WN]):
        dOut = ctx.colmajor(np.full((n, ns), 7.0))
        rc, out = _matmul(desc, np.ones(20), x, dOm, F, W, dOut)
        assert rc == -4 and np.all(out == 7.0)  # GPR_E_UNSUP, Out untouched
    hp = _hp([SE], d, rng)
    assert np.array_equal(_matmul([SE], hp, x, dOm, F, W)[1], _matmul([SE], hp, x, dOm, F, W)[1])
    big = _draw([SE, M32], d, 300)[1]
    for a, b in zip(_draw([SE, M32], d, 200)[1], big):
        assert np.array_equal(a, b[:200])
