"""GPU: kernel evaluation outside the unit cube -- gpr_kernel (Gram and difference form), the
fits' upper-only build around its clamp limit, gpr_kernel_grad and gpr_mll_grad's fused pass --
against the extended-precision reference and the derived rounding bounds of
tests/kernel_ref_ld.py, on its input families:

  F1  the exponential's ladder: D = 0, 1e-20, 1e-8, the reduction's ties and zero crossings up to
      n = 2e5, the normal/subnormal edge, the last non-zero values, exact zeros up to and past the
      clamp at 800, D = 1e4 and 1e7 (past kexp_s2_nc's proven range), sigma in {1, 1e-6, 1e5}
  F2  x = c0 + cube, c0 in {1e4, 1e6}, d = 3, 8, 21
  F3  a centre that is not the data's: a sorted grid of 2304 points in d = 1, and d = 8 with one
      axis spanning 2300 length-scales
  F4  planted points on both sides of KU_NC_LIM in the fit's upper-only build
  F5  Periodic at |x / p| up to 1e4

Nothing here is tuned to the device's output: every tolerance is the bound that module derives.
Each test prints max |err| / bound.
"""
import ctypes
import functools

import numpy as np
import pytest

import kernel_ref_ld as R
import test_product_cpu as PR
from kernel_ref_ld import LD, M32, M52, PER, SE, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

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


def lists_of(fam):
    return PLISTS if fam == "F5" else KLISTS


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def karr(desc):
    c = PR.codes(desc)
    return (ctypes.c_int * len(c))(*c), len(c)


@functools.lru_cache(maxsize=None)
def _inputs(fam, name):
    x, xp, hp = FAMILIES[fam](lists_of(fam)[name])
    hp.setflags(write=False)  # (x and xp go to torch.from_numpy, which wants them writable)
    return x, xp, hp


FORMS = ("gram", "diff")


@functools.lru_cache(maxsize=4)
def _reference_both(fam, name, cross):
    x, xp, hp = _inputs(fam, name)
    Kr, bounds, zero = R.element_bound(lists_of(fam)[name], hp, x, xp if cross else None, None,
                                       R.EPS, FORMS)
    for a in (Kr, zero) + bounds:
        a.setflags(write=False)
    return Kr, bounds, zero


def _reference(fam, name, form, cross):
    """(K_ref, bound, zero) -- the reference is computed once per case and matrix, shared by the
    two forms, never written"""
    Kr, bounds, zero = _reference_both(fam, name, cross)
    return Kr, bounds[FORMS.index(form)], zero


def check_matrix(K, ref, what):
    """finite, exactly 0.0 where every term has a factor with sigma^2 exp(-arg) below half the
    least subnormal (for sigma = 1: D_ref > 745.14, so every entry with D_ref > 745.2; a larger
    sigma moves the edge by ln sigma^2), and inside the element bound everywhere"""
    Kr, bound, zero = ref
    assert K.shape == Kr.shape
    assert np.all(np.isfinite(K)), f"{what}: non-finite entries"
    ratio = float(np.max(np.abs(K.astype(LD) - Kr) / bound))
    nz = int(np.count_nonzero(zero))
    print(f"  {what}: max |K - ref| / bound = {ratio:.3f}   ({nz} entries must be exactly 0)")
    assert np.all(K[np.asarray(zero)] == 0.0), f"{what}: an entry past the underflow is not 0.0"
    assert ratio <= 1.0, f"{what}: element bound exceeded {ratio:.3g} times"
    return ratio


# ---------------------------------------------------------------------------------------
# gpr_kernel
# ---------------------------------------------------------------------------------------
K_CASES = [(f, name) for f in FAMILIES for name in lists_of(f)]


@pytest.mark.parametrize("form", ["gram", "diff"])
@pytest.mark.parametrize("fam,name", K_CASES)
def test_kernel_matrix(fam, name, form, knobs):
    """Symmetric and cross K: finite, bitwise symmetric, exactly 0 past the underflow, and inside
    the element bound -- B_gram for the default Gram form, B_diff with GPR_KBUILD_EXACT=1."""
    if form == "diff":
        knobs("GPR_KBUILD_EXACT", 1)
    desc = lists_of(fam)[name]
    x, xp, hp = _inputs(fam, name)
    cov = PR.cov_of(desc)
    print(f"{fam} {name} {form}: n={x.shape[1]} m={xp.shape[1]} d={x.shape[0]}")
    K = G.kernel(cov, hp, x)
    check_matrix(K, _reference(fam, name, form, False), "sym")
    assert np.array_equal(K, K.T), "symmetric K must be bitwise symmetric"
    Kx = G.kernel(cov, hp, x, xp)
    check_matrix(Kx, _reference(fam, name, form, True), "cross")
    if name == "SE" and fam in ("F1", "F1s-6"):  # sigma <= 1: D_ref > 745.2 is exactly 0.0
        far = np.asarray(R.factor_dist_ld(SE, hp, x, xp) > 745.2)
        assert far.sum() >= 20 and np.all(Kx[far] == 0.0)
        far = np.asarray(R.factor_dist_ld(SE, hp, x, x) > 745.2)
        assert far.sum() >= 20 and np.all(K[far] == 0.0)


@pytest.mark.parametrize("sigma,fam", [(1.0, "F1"), (1e-6, "F1s-6")])
def test_measured_exponential_error(sigma, fam, knobs):
    """E, measured, in units of u relative to the value, with the distance's own error taken out
    exactly instead of by its bound.  Between the ladder's base (0, .5, .5) and a rung (r, .5, .5)
    the difference form (l = 1: the scaling is exact) forms D^ = fma(r, r, 0) + 0 + 0 = fl(r r),
    which float64 NumPy reproduces bit for bit; so |K - sigma^2 exp(-D^)| is the table
    exponential's error alone, on every rung whose value is normal: D from 1e-20 up, both sides
    of the reduction's ties and zero crossings up to n = 2e5 (D = 541), and at sigma = 1 the rung
    at D = 700, n = 2.6e5 (the largest D is printed).
    sigma = 1 (sigma^2 and its product with the table exact) must stay inside E_EXP, sigma = 1e-6
    inside E_EXP + E_S2.  Rows: base and its copy against the rungs (symmetric K), rungs against
    the base (cross K)."""
    knobs("GPR_KBUILD_EXACT", 1)
    desc = [SE]
    x, xp, hp = _inputs(fam, "SE")
    assert np.all(hp[1:] == 1.0) and np.all(xp[:, 0] == x[:, 0]) and np.all(x[:, 0] == x[:, 1])
    nr = len(R.f1_targets())
    rung = x[0, 2:2 + nr]
    assert np.all(x[1:, 2:2 + nr] == 0.5) and x[0, 0] == 0.0
    Dh = (rung * rung).astype(LD)  # fl(r r), exactly what the kernel forms
    k = LD(hp[0]) ** 2 * np.exp(-Dh)
    normal = np.asarray(k > LD(2.0) ** -1021)
    K = G.kernel(PR.cov_of(desc), hp, x)
    Kx = G.kernel(PR.cov_of(desc), hp, x, xp)
    worst = {"D < 1": 0.0, "1 <= D < 100": 0.0, "D >= 100": 0.0}
    for got in (K[0, 2:2 + nr], K[1, 2:2 + nr], K[2:2 + nr, 0], Kx[2:2 + nr, 0]):
        for band, sel in (("D < 1", Dh < 1), ("1 <= D < 100", (Dh >= 1) & (Dh < 100)), ("D >= 100", Dh >= 100)):
            sel = np.asarray(sel) & normal
            assert sel.sum() >= 3
            e = np.abs(got[sel].astype(LD) - k[sel]) / (LD(R.U) * k[sel])
            worst[band] = max(worst[band], float(np.max(e)))
    derived = R.E_EXP if sigma == 1.0 else R.E_TOT
    print(f"{fam}: measured E = " + ", ".join(f"{v:.3f} ({b})" for b, v in worst.items())
          + f"; largest normal D = {float(Dh[normal].max()):.1f}  (derived: {derived})")
    assert max(worst.values()) <= derived


# ---------------------------------------------------------------------------------------
# the fit's upper-only build around KU_NC_LIM (F4)
# ---------------------------------------------------------------------------------------
F4_LISTS = {"SE+WN": [SE, WN], "SE+SE+WN": [SE, SE, WN], "SE*SE+WN": [[SE, SE], WN]}


@functools.lru_cache(maxsize=2)
def _f4_reference(name, variant, d):
    x, _, hp = R.f4_planted(F4_LISTS[name], d, variant)
    out = (x, hp) + R.element_bound(F4_LISTS[name], hp, x, None, R.SELF, R.EPS, "gram")
    for a in out:
        a.setflags(write=False)
    return out


def _fit_buffer(desc, hp, x):
    ctx = G.default_context()
    L = G._lib.lib
    d, n = x.shape
    y = np.sin(x.sum(0))
    dx, dy = ctx.colmajor(x), ctx.colmajor(y)
    dK, alpha = ctx.empty(n, n), ctx.empty(n)
    info = ctypes.c_int(-7)
    ka, nk = karr(desc)
    hpa = np.array(hp)  # (held: the pointer does not own it)
    rc = L.gpr_fit(ctx.h, ka, nk, _dp(hpa), d, _P(dx), n, _P(dy), 1, n, R.EPS, _P(dK), n,
                   _P(alpha), ctypes.byref(info))
    assert rc == 0 and info.value == 0, (rc, info.value, L.gpr_last_error(ctx.h))
    return ctx.host(dK)


@pytest.mark.parametrize("d", [3, 8])
@pytest.mark.parametrize("variant", ["i", "ii"])
@pytest.mark.parametrize("name", list(F4_LISTS))
def test_fit_upper_build_around_the_clamp_limit(name, variant, d, knobs):
    """gpr_fit leaves the mirrored K in the strict lower triangle (as
    tests/test_gpu_parity.py::test_fit_buffer_upper_build_dag_mirror): inside the element bound,
    exactly 0 for the far pairs, bit for bit gpr_kernel's full K, info = 0; SE+WN with the column
    stores on and off, bitwise equal.  Variant (i): four points just below KU_NC_LIM, so that no
    interior unit clamps, and elements (300, 700) and (5, 300), D = 5.3e6-5.4e6, go through
    kexp_s2_nc in interior units and column-store items (kernel_ref_ld.f4_planted asserts which
    units those are); (5, 1039) and (700, 1039) meet the same distances in the clamped edge
    units.  Variant (ii) adds one point that every strip, unit and item it touches must clamp
    for."""
    desc = F4_LISTS[name]
    x, hp, Kr, bound, zero = _f4_reference(name, variant, d)
    n = x.shape[1]
    low = np.tril(np.ones((n, n), dtype=bool), -1)
    Kfull = G.kernel(PR.cov_of(desc), hp, x)
    print(f"F4({variant}) {name} d={d}")
    check_matrix(Kfull, (Kr, bound, zero), "gpr_kernel")
    bufs = []
    for cs in ((1, 0) if name == "SE+WN" else (None,)):
        if cs is not None:
            knobs("GPR_KBUILD_COLSTORE", cs)
        Rb = _fit_buffer(desc, hp, x)
        got = np.where(low, Rb, 0.0)
        assert np.all(np.isfinite(got))
        ratio = float(np.max(np.abs(got.astype(LD) - Kr)[low] / bound[low]))
        print(f"  fit (colstore {cs}): max |K - ref| / bound = {ratio:.3f}")
        assert np.all(got[np.asarray(zero) & low] == 0.0)
        assert ratio <= 1.0
        assert np.array_equal(got[low], Kfull[low])
        bufs.append(got)
    if len(bufs) == 2:
        assert np.array_equal(bufs[0], bufs[1])


# ---------------------------------------------------------------------------------------
# gpr_kernel_grad
# ---------------------------------------------------------------------------------------
GRAD_LISTS = {"SE+M52+WN": [SE, M52, WN], "PER+WN": [PER, WN]}
GRAD_FAMS = {"F1": lambda desc: R.f1_ladder(desc, 1.0), "F1s-6": lambda desc: R.f1_ladder(desc, 1e-6),
             "F1s5": lambda desc: R.f1_ladder(desc, 1e5), "F2-1e4-d3": lambda desc: R.f2_far(desc, 1e4, 3)}


@pytest.mark.parametrize("name", list(GRAD_LISTS))
@pytest.mark.parametrize("fam", list(GRAD_FAMS))
def test_kernel_grad(fam, name):
    """Every hyper-parameter index against kernel_grad_ld, B_diff propagated through the formula
    (kernel_ref_ld.grad_bound, which tabulates the rounding counts)."""
    desc = GRAD_LISTS[name]
    x, _, hp = GRAD_FAMS[fam](desc)
    cov = PR.cov_of(desc)
    worst = 0.0
    for i in range(1, len(hp) + 1):
        g = G.grad(cov, i, hp, x)
        ref, bound = R.kernel_grad_bound(desc, i, hp, x)
        if isinstance(ref, tuple):
            assert isinstance(g, G.UniformScaling) and abs(LD(g.lam) - ref[1]) <= bound
            continue
        assert np.all(np.isfinite(g)), f"index {i}"
        ratio = float(np.max(np.abs(g.astype(LD) - ref) / bound))
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{fam} {name} index {i}: bound exceeded {ratio:.3g} times"
    print(f"{fam} {name}: max |dK - ref| / bound over all indices = {worst:.3f}")


# ---------------------------------------------------------------------------------------
# gpr_mll_grad's fused pass, with a synthetic K^-1 and alpha
# ---------------------------------------------------------------------------------------
MLL_LISTS = {"SE+SE+WN": [SE, SE, WN], "SE*PER+WN": [[SE, PER], WN]}
MLL_FAMS = {"F1": lambda desc: R.f1_ladder(desc, 1.0),
            "F2-1e4-d3": lambda desc: R.f2_far(desc, 1e4, 3, n=192)}


@pytest.mark.parametrize("name", list(MLL_LISTS))
@pytest.mark.parametrize("fam", list(MLL_FAMS))
def test_mll_grad_fused_pass(fam, name):
    """g_i = -1/2 sum_ab (alpha_a alpha_b - Kinv_ab) dK_i,ab with a seeded normal alpha and a
    symmetric normal Kinv (nothing is factored).  Tolerance: the element bounds of dK_i weighted by
    |w_ab| (at most rho sum |w dK| with rho the largest relative element bound), plus n^2 u sum
    |w dK|, the worst case of any summation order.  The summation term dominates, so the assertion
    catches errors of the weights, the formulas and the slots, not single roundings; the error is
    therefore also printed in units of u sum |w dK| (a sum of n^2 terms in any tree of depth k
    stays below k of them)."""
    desc = MLL_LISTS[name]
    x, _, hp = MLL_FAMS[fam](desc)
    d, n = x.shape
    assert n == 192
    rng = np.random.default_rng(n + len(name))
    alpha = rng.standard_normal(n)
    A = rng.standard_normal((n, n))
    Kinv = 0.5 * (A + A.T)
    ctx = G.default_context()
    ka, nk = karr(desc)
    g = np.full(len(hp), np.nan)
    hpa = np.array(hp)  # (held, like the device arrays: the pointers do not own them)
    dx, dKinv, dalpha = ctx.colmajor(x), ctx.colmajor(Kinv), ctx.colmajor(alpha)
    rc = G._lib.lib.gpr_mll_grad(ctx.h, ka, nk, _dp(hpa), d, _P(dx), n, _P(dKinv), n, _P(dalpha),
                                 R.EPS, 0, _dp(g))
    assert rc == 0, G._lib.lib.gpr_last_error(ctx.h)
    assert np.all(np.isfinite(g))
    aa = np.outer(alpha.astype(LD), alpha.astype(LD))
    w = aa - Kinv.astype(LD)
    worst = worst_u = 0.0
    for i in range(1, len(hp) + 1):
        dK, bound = R.kernel_grad_bound(desc, i, hp, x)
        if isinstance(dK, tuple):
            dK, bound = dK[1] * np.eye(n, dtype=LD), bound * np.eye(n, dtype=LD)
        want = LD(-0.5) * np.sum(w * dK)
        mass = np.sum(np.abs(w * dK))
        tol = LD(0.5) * (np.sum(np.abs(w) * bound) + LD(n * n * R.U) * mass)
        err = abs(LD(g[i - 1]) - want)
        ratio = float(err / tol)
        worst, worst_u = max(worst, ratio), max(worst_u, float(err / (LD(0.5 * R.U) * mass)))
        assert ratio <= 1.0, f"{fam} {name} index {i}: {g[i - 1]!r} vs {want!r}, tolerance {tol!r}"
    print(f"{fam} {name}: max |g - ref| / tolerance = {worst:.3g}; max |g - ref| = {worst_u:.2f} u sum |w dK|")
