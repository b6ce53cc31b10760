"""CPU: the extended-precision reference of tests/kernel_ref_ld.py against the project's float64
restatements and against mpmath, every input family's preconditions, and a float64 NumPy emulation
of both distance forms (and of the table exponential) held to the derived bounds -- with two
mutations of the emulation that must break them, which shows that the families reach the clamp
and the cross centre.
"""
import mpmath
import numpy as np
import pytest

import kernel_ref_ld as R
import test_matern_cpu as M
import test_periodic_cpu as P
import test_product_cpu as PR
from kernel_ref_ld import LD, M32, M52, PER, SE, WN
from oracle import gpr_oracle as O

KLISTS = {"SE": [SE], "SE+SE+WN": [SE, SE, WN], "M52+WN": [M52, WN], "SE+M32": [SE, M32],
          "SE*SE+WN": [[SE, SE], WN]}
PLISTS = {"PER+WN": [PER, WN], "SE*PER+WN": [[SE, PER], WN]}

FAMILIES = {
    "F1": lambda desc: R.f1_ladder(desc, 1.0),
    "F1s-6": lambda desc: R.f1_ladder(desc, 1e-6),
    "F1s5": lambda desc: R.f1_ladder(desc, 1e5),
    "F2-1e4-d3": lambda desc: R.f2_far(desc, 1e4, 3),
    "F2-1e4-d8": lambda desc: R.f2_far(desc, 1e4, 8),
    "F2-1e4-d21": lambda desc: R.f2_far(desc, 1e4, 21),
    "F2-1e6-d3": lambda desc: R.f2_far(desc, 1e6, 3),
    "F2-1e6-d8": lambda desc: R.f2_far(desc, 1e6, 8),
    "F2-1e6-d21": lambda desc: R.f2_far(desc, 1e6, 21),
    "F3a": R.f3a_grid,
    "F3b": R.f3b_spread,
    "F5": R.f5_periodic,
}


def rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b) / np.abs(b)))


# ---------------------------------------------------------------------------------------
# the reference against the restatements and mpmath
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [[SE], [SE, WN], [SE, SE, WN], [WN, SE]])
def test_agrees_with_the_oracle_on_the_unit_cube(kinds):
    """rtol 1e-14 is the oracle's own rounding, (d + 2) u D, at D <= 3 (1.2 x 1.22)^2 = 6.5:
    3.6e-15; hence l_k = 0.75 sqrt(8/d) within 20 %, not the default 3 sqrt(8/d) (D up to 100)."""
    rng = np.random.default_rng(len(kinds))
    d, n, m = 3, 60, 25
    x, xp = rng.random((d, n)), rng.random((d, m))
    hp = O.default_hp(kinds, d, length=0.75 * np.sqrt(8.0 / d))
    hp = hp * rng.uniform(0.8, 1.2, len(hp))
    assert rel(O.kernel(kinds, hp, x), R.kernel_ld(kinds, hp, x)) <= 1e-14
    assert rel(O.kernel(kinds, hp, x, x), R.kernel_ld(kinds, hp, x, x)) <= 1e-14
    assert rel(O.kernel(kinds, hp, x, xp), R.kernel_ld(kinds, hp, x, xp)) <= 1e-14
    for i in range(1, len(hp) + 1):
        a, b = O.kernel_grad(kinds, i, hp, x), R.kernel_grad_ld(kinds, i, hp, x)
        if isinstance(a, tuple):
            assert b[0] == "I" and abs(a[1] - float(b[1])) <= 1e-15 * abs(a[1])
            continue
        np.testing.assert_allclose(a, b.astype(np.float64), rtol=1e-13, atol=1e-16)


@pytest.mark.parametrize("desc", [[M32, WN], [SE, M52, WN], [PER, WN], [SE, PER, M32],
                                  [[SE, PER], WN], [WN, [M52, PER]], [[SE, M32, M52, PER]]])
def test_agrees_with_the_restatements(desc):
    """tests/test_matern_cpu.py, test_periodic_cpu.py and test_product_cpu.py, l_k = 0.75 sqrt(8/d) /
    sqrt(F): their float64 difference forms carry ~ (d + 2) u D of rounding per factor (D <= 20
    here, F <= 4 factors): rtol 1e-13, as those files assert among themselves."""
    rng = np.random.default_rng(len(str(desc)))
    d, n, m = 3, 50, 21
    x, xp = rng.random((d, n)), rng.random((d, m))
    hp = PR.model_hp(desc, d, rng)
    assert rel(PR.kernel(desc, hp, x), R.kernel_ld(desc, hp, x)) <= 1e-13
    assert rel(PR.kernel(desc, hp, x, x), R.kernel_ld(desc, hp, x, x)) <= 1e-13
    assert rel(PR.kernel(desc, hp, x, xp), R.kernel_ld(desc, hp, x, xp)) <= 1e-13
    if not PR.has_product(desc):
        fl = R.flat(desc)
        if PER not in fl:
            assert rel(M.kernel(fl, hp, x), R.kernel_ld(desc, hp, x)) <= 1e-13
        assert rel(P.kernel(fl, hp, x, xp), R.kernel_ld(desc, hp, x, xp)) <= 1e-13
    for i in range(1, len(hp) + 1):
        a, b = PR.kernel_grad(desc, i, hp, x), R.kernel_grad_ld(desc, i, hp, x)
        if isinstance(a, tuple):
            assert abs(a[1] - float(b[1])) <= 1e-15 * abs(a[1])
            continue
        np.testing.assert_allclose(a, b.astype(np.float64), rtol=1e-12, atol=1e-15)


def test_agrees_with_mpmath_on_the_ladder():
    """Fourteen F1 rungs against the base point at 40 digits: within 1e-18 absolute (sigma = 1, so
    the values are at most 1), and within (D + 4) 2^-63 relative, which is what rounding D to the
    long double format alone costs in exp(-D)."""
    mpmath.mp.dps = 40
    x, xp, hp = R.f1_ladder([SE, M52, WN])
    tg = R.f1_targets()
    picks = [0, 1, 2, 15, 29, 30, 31, 32, 36, 40, 44, 46, 50, len(tg) - 2]
    K = R.kernel_ld([SE, M52, WN], hp, x, xp)
    s1, l1, s2, l2 = hp[0], hp[1:4], hp[4], hp[5:8]
    for r in picks:
        a, worst = 2 + r, 0.0
        D1 = sum((mpmath.mpf(float(l1[k])) * (mpmath.mpf(float(x[k, a])) - mpmath.mpf(float(xp[k, 0])))) ** 2
                 for k in range(3))
        D2 = sum((mpmath.mpf(float(l2[k])) * (mpmath.mpf(float(x[k, a])) - mpmath.mpf(float(xp[k, 0])))) ** 2
                 for k in range(3))
        ar = mpmath.sqrt(5) * mpmath.sqrt(D2)
        want = mpmath.mpf(float(s1)) ** 2 * mpmath.exp(-D1) + \
            mpmath.mpf(float(s2)) ** 2 * (1 + ar + ar * ar / 3) * mpmath.exp(-ar)
        got = mpmath.mpf(np.format_float_scientific(K[a, 0], precision=25, unique=False))
        err = abs(got - want)
        assert err <= mpmath.mpf(10) ** -18, (r, tg[r][0], err)
        if want > 0:
            rmax = (float(max(D1, ar)) + 4.0) * 2.0 ** -63
            assert err <= rmax * want + mpmath.mpf(2) ** -16445, (r, tg[r][0], float(err / want), rmax)


# ---------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------
def lists_of(fam):
    return PLISTS if fam == "F5" else KLISTS


CASES = [(f, name) for f in FAMILIES for name in lists_of(f)]


@pytest.mark.parametrize("fam,name", CASES)
def test_family_preconditions(fam, name):
    """Each family asserts its own construction; here also the cap that keeps the bounds
    meaningful: B_gram <= 1e-8 on every pair with D_ref < 40."""
    desc = lists_of(fam)[name]
    x, xp, hp = FAMILIES[fam](desc)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(xp)) and np.all(np.isfinite(hp))
    worst = R.assert_north_star(desc, hp, x, xp)
    print(f"{fam} {name}: n={x.shape[1]} m={xp.shape[1]} d={x.shape[0]}  max B_gram (D < 40) = {worst:.2e}")


@pytest.mark.parametrize("d", [3, 8])
@pytest.mark.parametrize("variant", ["i", "ii"])
@pytest.mark.parametrize("name", ["SE+WN", "SE+SE+WN", "SE*SE+WN"])
def test_f4_preconditions(name, variant, d):
    desc = {"SE+WN": [SE, WN], "SE+SE+WN": [SE, SE, WN], "SE*SE+WN": [[SE, SE], WN]}[name]
    x, _, hp = R.f4_planted(desc, d, variant)
    worst = R.assert_north_star(desc, hp, x, None, skip=R.F4_IDX)
    print(f"F4({variant}) {name} d={d}: max B_gram (D < 40, planted rows/columns aside) = {worst:.2e}")


# ---------------------------------------------------------------------------------------
# float64 emulation of both distance forms against the bounds
# ---------------------------------------------------------------------------------------
def emulation_ratio(desc, hp, x, xp, form, **mut):
    """max |D^ - D_ref| / B over the pairs and factors (pairs with B = 0 must be exact)"""
    Bs = R.dist_bounds(desc, hp, x, xp, None, form)
    fs = [kh for t in R.split_hp(desc, hp, x.shape[0]) for kh in t if kh[0] != WN]
    worst = 0.0
    for (kind, h), B in zip(fs, Bs):
        Dh = R.emulate_dist(kind, h, x, xp, form, **mut)
        Dr = R.factor_dist_ld(kind, h, x, x if xp is None else xp)
        err = np.abs(Dh.astype(LD) - Dr).astype(np.float64)
        assert np.all(err[B == 0.0] == 0.0)
        pos = B > 0.0
        worst = max(worst, float(np.max(err[pos] / B[pos])))
    return worst


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_emulated_distances_stay_inside_the_bounds(fam):
    name = "SE*PER+WN" if fam == "F5" else "SE+SE+WN"
    desc = lists_of(fam)[name]
    x, xp, hp = FAMILIES[fam](desc)
    for form in ("diff", "gram"):
        for xq in (None, xp):
            r = emulation_ratio(desc, hp, x, xq, form)
            print(f"{fam} {name} {form} {'sym' if xq is None else 'cross'}: max |D^ - D| / B = {r:.3f}")
            assert r <= 1.0


@pytest.mark.parametrize("variant", ["i", "ii"])
def test_emulated_distances_f4(variant):
    desc = [SE, SE, WN]
    x, _, hp = R.f4_planted(desc, 8, variant)
    for form in ("diff", "gram"):
        r = emulation_ratio(desc, hp, x, None, form)
        print(f"F4({variant}) d=8 {form}: max |D^ - D| / B = {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("fam", ["F2-1e6-d8", "F3a", "F3b"])
def test_a_centre_per_operand_breaks_the_cross_bound(fam):
    """Mutation: centring xp by its own mean must push the emulated Gram distance out of B_gram --
    the family's cross points do not share the row points' centre."""
    desc = KLISTS["SE+SE+WN"]
    x, xp, hp = FAMILIES[fam](desc)
    r = emulation_ratio(desc, hp, x, xp, "gram", xp_own_centre=True)
    print(f"{fam}: ratio with a centre per operand = {r:.3g}")
    assert r > 1.0


@pytest.mark.parametrize("fam", ["F1", "F1s-6", "F1s5", "F2-1e4-d3"])
@pytest.mark.parametrize("name", ["SE+M52+WN", "SE+SE+WN"])
def test_restated_gradients_stay_inside_the_bounds(fam, name):
    """The float64 restatement of dK/dtheta (difference form, the library exponential's accuracy)
    plays the device here: every index inside kernel_grad_bound.  (Not the Periodic formulas: the
    restatement rounds their angle pi r / p three times, sinpi(fl(r / p)) twice.)"""
    desc = {"SE+M52+WN": [SE, M52, WN], "SE+SE+WN": [SE, SE, WN]}[name]
    x, _, hp = FAMILIES[fam](desc)
    worst = 0.0
    for i in range(1, len(hp) + 1):
        ref, bound = R.kernel_grad_bound(desc, i, hp, x)
        if isinstance(ref, tuple):
            continue
        g = PR.kernel_grad(desc, i, hp, x)
        worst = max(worst, float(np.max(np.abs(g.astype(LD) - ref) / bound)))
    print(f"{fam} {name}: max |dK^ - dK| / bound = {worst:.3f}")
    assert worst <= 1.0


def emulated_kernel_ratio(sigma, form, clamp):
    """SquaredExp on the ladder: the emulated distance through the emulated table exponential,
    against the element bound"""
    desc = [SE]
    x, xp, hp = R.f1_ladder(desc, sigma)
    worst = 0.0
    for xq in (None, xp):
        Kr, bound, zero = R.element_bound(desc, hp, x, xq, None, R.EPS, form)
        Dh = R.emulate_dist(SE, hp, x, xq, form)
        K = R.emulate_kexp(Dh, hp[0], clamp)
        if xq is None:
            K[np.diag_indices(K.shape[0])] += R.EPS
        if not np.all(np.isfinite(K)):
            return np.inf
        if clamp:
            assert np.all(K[np.asarray(zero)] == 0.0)
        worst = max(worst, float(np.max(np.abs(K.astype(LD) - Kr) / bound)))
    return worst


@pytest.mark.parametrize("sigma", [1.0, 1e-6, 1e5])
@pytest.mark.parametrize("form", ["diff", "gram"])
def test_emulated_table_exponential_on_the_ladder(sigma, form):
    r = emulated_kernel_ratio(sigma, form, True)
    print(f"F1 sigma={sigma:g} {form}: max |K^ - K| / bound = {r:.3f}")
    assert r <= 1.0


def test_dropping_the_clamp_breaks_the_ladder():
    """Mutation: without the clamp at 800 the rung at D = 1e7 wraps n past int32."""
    r = emulated_kernel_ratio(1.0, "gram", False)
    print(f"ratio without the clamp = {r:.3g}")
    assert r > 1.0
