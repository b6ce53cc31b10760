"""Leave-one-out training on the device: gpr_fit_loo / gpr_loo / gpr_loo_grad and the cost layer's
LeaveOneOut dispatch, against the numpy identity of tests/test_loo_cpu.py (``loo_reference``: the
oracle's kernel, its kernel_grad, P and alpha through a Cholesky factor).

Bars.  Value: rtol 1e-8 with atol 1e-8 sum_i |f_i| -- the bar gpr_cv_kfold's fold losses are held
to, the value being a sum of them.  Gradient: rtol 1e-8, atol 1e-8 max|g_ref| -- the MLL gradient's
bar of test_mll_and_grad without its "+ 1" (MSE gradients are of order 1e-5).  Two float64 routes
to the reference (Cholesky against inv) differ by at most 3e-12 of max|g| at these shapes.
Every comparison prints its measured error before it asserts.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import gpr_oracle as O
from test_loo_cpu import CRITS, data, loo_abs_sum, loo_from_matrices, loo_reference

G = pytest.importorskip("gpr_amd")

pytestmark = pytest.mark.gpu

_KINDS = {"SE+WN": (["SE", "WN"], lambda: G.SquaredExp() + G.WhiteNoise()),
          "SE+SE+WN": (["SE", "SE", "WN"],
                       lambda: G.SquaredExp() + G.SquaredExp() + G.WhiteNoise())}
_COSTS = {"LogPredictive": G.LogPredictive, "MSE": G.MSE, "ChiSq": G.ChiSq,
          "Mahalanobis": G.Mahalanobis}
assert tuple(_COSTS) == CRITS
# one partial tile; n no multiple of 16; odd n (the GEMM's unaligned path); five 128-tiles (the
# pipelined GEMM, the direct tile-DAG)
_SHAPES = [(2, 10), (2, 200), (3, 331), (3, 640)]


@functools.lru_cache(maxsize=None)
def _case(kname, d, n):
    kinds, _ = _KINDS[kname]
    x, y = data(d, n, 11 + d)
    hp = O.default_hp(kinds, d, length=2.0)
    assert np.linalg.cond(O.kernel(kinds, hp, x)) <= 4e4
    return x, y, hp


@functools.lru_cache(maxsize=None)
def _ref(kname, crit, d, n):
    """(value, grad, sum |f_i|) of the numpy identity: computed once, shared, never modified."""
    kinds, _ = _KINDS[kname]
    x, y, hp = _case(kname, d, n)
    v, g = loo_reference(kinds, hp, crit, x, y)
    g.setflags(write=False)
    return v, g, loo_abs_sum(kinds, hp, crit, x, y)


def _model(kname, d, n):
    x, y, hp = _case(kname, d, n)
    return G.GPRModel(_KINDS[kname][1](), hp, x, y), hp


def _check_value(tag, got, want, asum):
    print(tag, "value err / sum|f|", abs(got - want) / asum)
    np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-8 * asum, err_msg=tag)


def _check_grad(tag, got, want):
    print(tag, "grad max err / max|g|", np.max(np.abs(got - want)) / np.max(np.abs(want)))
    np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-8 * np.max(np.abs(want)), err_msg=tag)


@pytest.mark.parametrize("d,n", _SHAPES)
@pytest.mark.parametrize("kname", list(_KINDS))
def test_value_vs_reference(kname, d, n):
    md, hp = _model(kname, d, n)
    tl = G.LooLossCache(md)
    tg = G.MllGradCache(md)
    G.update_cache_(tg, hp, md)
    for crit, cost in _COSTS.items():
        want, _, asum = _ref(kname, crit, d, n)
        loo = G.LeaveOneOut(cost())
        tag = f"{kname} {(d, n)} {crit}"
        _check_value(tag + " LooLossCache", G.loss(loo, hp, md, tl), want, asum)
        _check_value(tag + " loss(md, tl)", G.loss(loo, md, tl), want, asum)
        _check_value(tag + " MllGradCache", G.loss(loo, md, tg), want, asum)
        _check_value(tag + " loss(md)", G.loss(loo, md), want, asum)


@pytest.mark.parametrize("d,n", _SHAPES)
@pytest.mark.parametrize("kname", list(_KINDS))
def test_gradient_vs_reference(kname, d, n):
    md, hp = _model(kname, d, n)
    tc = G.MllGradCache(md)
    for crit, cost in _COSTS.items():
        want_v, want_g, asum = _ref(kname, crit, d, n)
        loo = G.LeaveOneOut(cost())
        tag = f"{kname} {(d, n)} {crit}"
        _check_grad(tag + " grad", G.grad(loo, hp, md), want_g)
        g = np.zeros(len(hp))
        v = G.loss_grad_(loo, True, g, hp, md, tc)
        _check_grad(tag + " loss_grad_", g, want_g)
        _check_value(tag + " loss_grad_", v, want_v, asum)
        assert G.loss_grad_(loo, None, g, hp, md, tc) is None
        _check_value(tag + " loss_grad_(F only)", G.loss_grad_(loo, True, None, hp, md, tc), want_v,
                     asum)
        gl = np.zeros(len(hp))
        vl = G.log_loss_grad_(loo, True, gl, np.log(hp), md, tc)
        # (exp(log(hp)) is hp to an ulp; the identity's own sensitivity to that is far below the bar)
        _check_grad(tag + " log_loss_grad_", gl, want_g * hp)
        _check_value(tag + " log_loss_grad_", vl, want_v, asum)


# hyper-parameters per part at d = 2: [sigma, l_1, l_2], Periodic [sigma, l_1, l_2, p_1, p_2]
_OTHER = {
    "M52+WN": (lambda: G.Matern52() + G.WhiteNoise(), [1.1, 1.7, 2.3, 0.1]),
    "PER+WN": (lambda: G.Periodic() + G.WhiteNoise(), [1.1, 0.9, 0.7, 1.3, 1.9, 0.1]),
    "SE*PER+WN": (lambda: G.SquaredExp() * G.Periodic() + G.WhiteNoise(),
                  [1.1, 1.7, 2.3, 0.9, 0.8, 0.6, 1.3, 1.9, 0.1]),
    "SE+M32+WN": (lambda: G.SquaredExp() + G.Matern32() + G.WhiteNoise(),
                  [1.0, 2.0, 2.0, 0.6, 1.5, 2.5, 0.1]),
}


@pytest.mark.parametrize("kname", list(_OTHER))
def test_other_kinds_vs_identity_on_device_matrices(kname):
    """The LOO machinery independently of the fused pass: the reference is the numpy identity fed
    with the device's own K and dK matrices (tested against long double elsewhere)."""
    d, n = 2, 200
    make, hp = _OTHER[kname]
    hp = np.array(hp)
    x, y = data(d, n, 11 + d)
    cov = make()
    md = G.GPRModel(cov, hp, x, y)
    K = G.kernel(cov, hp, x)
    print(kname, "cond", np.linalg.cond(K))
    dKs = []
    for i in range(len(hp)):
        dK = G.grad(cov, i + 1, hp, x)
        dKs.append(("I", dK.lam) if isinstance(dK, G.UniformScaling) else dK)
    tc = G.MllGradCache(md)
    for crit, cost in _COSTS.items():
        want_v, want_g, f = loo_from_matrices(K, dKs, crit, y)
        loo = G.LeaveOneOut(cost())
        g = np.zeros(len(hp))
        v = G.loss_grad_(loo, True, g, hp, md, tc)
        _check_value(f"{kname} {crit}", v, want_v, np.abs(f).sum())
        _check_value(f"{kname} {crit} LooLossCache", G.loss(loo, hp, md), want_v, np.abs(f).sum())
        _check_grad(f"{kname} {crit}", g, want_g)


@pytest.mark.parametrize("d,n", [(2, 200), (3, 331)])
def test_agrees_with_cv_kfold(d, n):
    md, hp = _model("SE+WN", d, n)
    x, y, _ = _case("SE+WN", d, n)
    folds = [np.array([i]) for i in range(n)]
    for cost in (G.MSE, G.ChiSq):
        want = G.cv_kfold(md, cost(), x, y, folds).sum()
        got = G.loss(G.LeaveOneOut(cost()), hp, md)
        print(cost.__name__, (d, n), "rel", abs(got - want) / abs(want))
        np.testing.assert_allclose(got, want, rtol=1e-8)


def test_repeatable_bit_for_bit():
    md, hp = _model("SE+SE+WN", 3, 640)
    tc = G.MllGradCache(md)
    for cost in _COSTS.values():
        loo = G.LeaveOneOut(cost())
        out = []
        for _ in range(2):
            g = np.zeros(len(hp))
            v = G.loss_grad_(loo, True, g, hp, md, tc)
            out.append((v, g, G.loss(loo, hp, md)))
        assert out[0][0] == out[1][0] and out[0][2] == out[1][2]
        np.testing.assert_array_equal(out[0][1], out[1][1])


def test_cache_is_read_only_and_mll_untouched():
    md, hp = _model("SE+WN", 3, 331)
    mll = G.MarginalLikelihood()
    tc = G.MllGradCache(md)
    g_before = G.grad(mll, hp, md, tc=tc)
    v_before = G.loss(mll, md, tc)
    kinv, alpha = md.ctx.host(tc.Kinv), md.ctx.host(tc.alpha)
    for cost in _COSTS.values():
        G.core._loo_grad(md, tc, G.core._loo_crit(G.LeaveOneOut(cost())), want_value=True)
        np.testing.assert_array_equal(md.ctx.host(tc.Kinv), kinv)
        np.testing.assert_array_equal(md.ctx.host(tc.alpha), alpha)
    # the marginal likelihood on the same context and cache, after the LOO calls
    np.testing.assert_array_equal(G.core._mll_grad(md, tc), g_before)
    assert G.loss(mll, md, tc) == v_before
    np.testing.assert_array_equal(G.grad(mll, hp, md, tc=tc), g_before)


def test_c_abi_argument_errors():
    md, hp = _model("SE+WN", 2, 200)
    ctx, n = md.ctx, md.n
    lib, P = G._lib.lib, G.core._ptr
    tc = G.MllGradCache(md)
    G.update_cache_(tc, hp, md)
    kinds, nk = G.core._kinds_arr(md.covar)
    _, hpp = G.core._hp_arr(hp)
    dp = ctypes.POINTER(ctypes.c_double)
    sentinel = 123.25
    out = ctypes.c_double(sentinel)
    g = np.full(len(hp), sentinel)
    val = ctypes.c_double(sentinel)

    def err():
        return lib.gpr_last_error(ctx.h).decode()

    def loo(crit=4, p=None, incp=n + 1, a=None, nn=n, o=ctypes.byref(out)):
        return lib.gpr_loo(ctx.h, crit, P(tc.Kinv) if p is None else p, incp,
                           P(tc.alpha) if a is None else a, nn, o)

    for kw, name in (({"crit": 0}, "crit"), ({"crit": 5}, "crit"), ({"incp": 0}, "incp"),
                     ({"incp": -1}, "incp"), ({"p": ctypes.c_void_p(0)}, "dp"),
                     ({"a": ctypes.c_void_p(0)}, "dalpha"), ({"o": None}, "out"), ({"nn": 0}, "n")):
        assert loo(**kw) == -1, kw
        assert name in err() and "gpr_loo" in err(), (kw, err())
        assert out.value == sentinel

    def lg(k=kinds, h=hpp, x=None, kinv=None, ldk=n, a=None, crit=4, v=ctypes.byref(val), gr=None):
        return lib.gpr_loo_grad(ctx.h, k, nk, h, md.d, P(md.dx()) if x is None else x, n,
                                P(tc.Kinv) if kinv is None else kinv, ldk,
                                P(tc.alpha) if a is None else a, 1e-8, crit, 0, v,
                                g.ctypes.data_as(dp) if gr is None else gr)

    null = ctypes.c_void_p(0)
    for kw, name in (({"crit": 0}, "crit"), ({"crit": 7}, "crit"), ({"ldk": n - 1}, "ldk"),
                     ({"k": None}, "kinds"), ({"h": None}, "hp"), ({"x": null}, "dX"),
                     ({"kinv": null}, "dKinv"), ({"a": null}, "dalpha"),
                     ({"gr": ctypes.cast(null, dp)}, "grad")):
        assert lg(**kw) == -1, kw
        assert name in err() and "gpr_loo_grad" in err(), (kw, err())
        assert val.value == sentinel and np.all(g == sentinel)

    K = ctx.empty(n, n)
    al, pd = ctx.zeros(n), ctx.zeros(n)
    info = ctypes.c_int(77)

    def fl(k=kinds, h=hpp, x=None, y=None, dk=None, ldk=n, a=None, p=None):
        return lib.gpr_fit_loo(ctx.h, k, nk, h, md.d, P(md.dx()) if x is None else x, n,
                               P(md.dsample()) if y is None else y, 1e-8,
                               P(K) if dk is None else dk, ldk, P(al) if a is None else a,
                               P(pd) if p is None else p, ctypes.byref(info))

    for kw, name in (({"ldk": n - 1}, "ldk"), ({"k": None}, "kinds"), ({"h": None}, "hp"),
                     ({"x": null}, "dX"), ({"y": null}, "dy"), ({"dk": null}, "dK"),
                     ({"a": null}, "dalpha"), ({"p": null}, "dpdiag")):
        assert fl(**kw) == -1, kw
        assert name in err() and "gpr_fit_loo" in err(), (kw, err())
        assert info.value == 77
        assert not ctx.host(al).any() and not ctx.host(pd).any()
    # and the same calls with good arguments succeed (value NULL is allowed)
    assert loo() == 0 and lg(v=None) == 0 and fl() == 0 and info.value == 0
    want, want_g, asum = _ref("SE+WN", "LogPredictive", 2, 200)
    _check_value("C ABI", out.value, want, asum)
    _check_grad("C ABI", g, want_g)
    assert val.value == sentinel


@functools.lru_cache(maxsize=None)
def _train_problem():
    rng = np.random.default_rng(63)
    x = rng.random((1, 60))
    y = np.sin(6.0 * x[0]) + 0.1 * rng.standard_normal(60)
    return x, y


@pytest.mark.parametrize("method", ["LBFGS", "NelderMead"])
def test_train(method):
    x, y = _train_problem()
    hp0 = np.array([1.0, 1.0, 0.3])
    md = G.GPRModel(G.SquaredExp() + G.WhiteNoise(), hp0, x, y)
    loo = G.LeaveOneOut()
    hp_tr, res = G.train(md, loo, hp0, method=getattr(G, method)())
    # (LogScale: train takes hp0 as given for the optimisation variable, so it starts at exp(hp0))
    l_tr = G.loss(loo, hp_tr, md)
    l_0, l_start = G.loss(loo, hp0, md), G.loss(loo, np.exp(hp0), md)
    print(method, "hp", hp_tr, "loss", l_tr, "at hp0", l_0, "at exp(hp0)", l_start, "g_residual",
          res.g_residual, "iterations", res.iterations)
    assert np.isfinite(l_tr) and l_tr == res.minimum
    assert l_tr < l_0 and l_tr < l_start
    v, _ = loo_reference(["SE", "WN"], hp_tr, "LogPredictive", x, y)
    np.testing.assert_allclose(l_tr, v, rtol=1e-8)
    if method == "LBFGS":
        assert res.g_residual < 1e-4
