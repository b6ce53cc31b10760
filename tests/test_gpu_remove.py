"""GPU: gpr_fit_remove and the Python layer on it (remove_) -- taking observations out of a fitted
model without refactoring it.

The reference is always the full fit of the kept points (tests/test_remove_cpu.py builds it and
shows that the rank-r Givens update meets these tolerances on the same inputs).  Tolerances: the
project's own for the same quantities from gpr_fit, as tests/test_gpu_append.py -- U's upper
triangle and alpha rtol 1e-8 / atol 1e-12, mu rtol 1e-8 / atol 1e-10, the diagonal variance
rtol 1e-8 / atol 1e-8 diag_prior, the strict lower triangle against K rtol 1e-13, the MLL value
rtol 1e-10.  The two routes of the update (GPR_REMOVE_SWEEP) run the same arithmetic on every
element: they are compared bit for bit, which is also the check of the sweep's hand-off.
"""
import ctypes
import functools

import numpy as np
import pytest

import test_append_cpu as A
import test_periodic_cpu as R
import test_remove_cpu as RM
from oracle import gpr_oracle as O
from test_append_cpu import TOL_K, TOL_MLL, TOL_MU, TOL_U
from test_periodic_cpu import M52, PER, SE, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

GPR_E_ARG = -1
EPS = 1e-8
PAD = 7.25  # what both buffers are filled with before anything is written
KINDS, D_IN = RM.KINDS, RM.D_IN


def karr(kinds):
    return (ctypes.c_int * len(kinds))(*[R.KIND_CODE[k] for k in kinds])


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dp(a):
    return np.ascontiguousarray(a).ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ia(idx):
    return (ctypes.c_int * len(idx))(*[int(v) for v in idx])


class Fit:
    """n points fitted by gpr_fit into a PAD-filled buffer of leading dimension ld"""

    def __init__(self, kinds, hp, x, y, ld=None):
        self.ctx = ctx = G.default_context()
        self.L = G._lib.lib
        self.kinds, self.hp = kinds, np.ascontiguousarray(hp, dtype=np.float64)
        self.d, self.n = x.shape
        self.x, self.y = x, y
        self.ny = 1 if y.ndim == 1 else y.shape[1]
        self.ld = ld or self.n
        self.dx = ctx.colmajor(x)
        self.dy = ctx.colmajor(np.array(y))   # (a writable copy: the shared case arrays are read-only)
        self.dK = ctx.empty(self.n, self.ld)
        self.dK.fill_(PAD)
        self.alpha = ctx.empty(self.ny, self.n)
        info = ctypes.c_int(-1)
        rc = self.L.gpr_fit(ctx.h, karr(kinds), len(kinds), _dp(self.hp), self.d, _P(self.dx), self.n,
                            _P(self.dy), self.ny, self.n, EPS, _P(self.dK), self.ld, _P(self.alpha),
                            ctypes.byref(info))
        assert rc == 0 and info.value == 0, self.L.gpr_last_error(ctx.h)

    def K(self):
        self.ctx.sync()
        return self.dK.cpu().numpy().T.copy()

    def a(self):
        self.ctx.sync()
        h = self.alpha.cpu().numpy()
        return h[0].copy() if self.ny == 1 else h.T.copy()


class Removed:
    """gpr_fit_remove of idx from a fitted buffer into a PAD-filled one of leading dimension ldo; y of
    the kept points with leading dimension n' + ldy_pad; room: further columns of the buffer, for a
    following append.  Has the attributes of a Fit."""

    def __init__(self, src, idx, ldo=None, ldy_pad=0, room=0):
        self.ctx, self.L, self.kinds, self.hp, self.d = src.ctx, src.L, src.kinds, src.hp, src.d
        ctx = self.ctx
        keep = RM.keep_of(src.n, idx)
        self.n, self.ny = len(keep), src.ny
        self.x, self.y = src.x[:, keep], src.y[keep]
        self.ld = ldo or self.n
        self.dx = ctx.colmajor(self.x)
        ldy = self.n + ldy_pad
        Y = np.full((ldy, self.ny), PAD)
        Y[:self.n] = self.y.reshape(self.n, self.ny)
        self.dy = ctx.colmajor(Y)
        self.dK = ctx.empty(self.n + room, self.ld)
        self.dK.fill_(PAD)
        self.alpha = ctx.empty(self.ny, self.n)
        rc = self.L.gpr_fit_remove(ctx.h, _P(src.dK), src.n, src.ld, _ia(idx), len(idx), _P(self.dy),
                                   self.ny, ldy, _P(self.dK), self.ld, _P(self.alpha))
        assert rc == 0, self.L.gpr_last_error(ctx.h)

    K, a = Fit.K, Fit.a


@functools.lru_cache(maxsize=None)
def reference(n0, idx, ny=1):
    """(x, y, hp) of the n0 points and the kept points' (K, U, alpha); shared, kept unchanged"""
    x, y, hp, K, U, alpha = A.make_case(KINDS, n0, 0, D_IN, ny)
    out = RM.kept_fit(K, y, RM.keep_of(n0, list(idx)))
    for a in out:
        a.setflags(write=False)
    return (x, y, hp) + out


def check_factor(dev, K_ref, U_ref, alpha_ref, what=""):
    n = dev.n
    buf = dev.K()
    Kd = buf[:n, :n]
    err_u = np.max(np.abs(np.triu(Kd) - np.triu(U_ref)) / (1e-12 + 1e-8 * np.abs(np.triu(U_ref))))
    low = np.tril_indices(n, -1)
    err_k = np.max(np.abs(Kd[low] - K_ref[low]) / np.abs(K_ref[low])) if n > 1 else 0.0
    a = dev.a()
    err_a = np.max(np.abs(a - alpha_ref) / (1e-12 + 1e-8 * np.abs(alpha_ref)))
    print(f"  {what} n'={n} ldo={dev.ld}: U {err_u:.2e}  alpha {err_a:.2e} of the tolerance; "
          f"lower K rel {err_k:.2e}")
    assert np.all(np.isfinite(np.triu(Kd))) and np.all(np.isfinite(a))
    np.testing.assert_allclose(np.triu(Kd), np.triu(U_ref), **TOL_U)
    np.testing.assert_allclose(Kd[low], K_ref[low], **TOL_K)
    np.testing.assert_allclose(a, alpha_ref, **TOL_U)
    assert np.all(buf[n:] == PAD) and np.all(buf[:n, n:] == PAD), "wrote outside (n0 - r)^2"


def run_case(n0, idx, pad=0, pado=0, ny=1, ldy_pad=0):
    x, y, hp, Kk, Uk, ak = reference(n0, tuple(idx), ny)
    src = Fit(KINDS, hp, x, y, ld=n0 + pad)
    before = src.K()
    out = Removed(src, idx, ldo=n0 - len(idx) + pado, ldy_pad=ldy_pad)
    assert np.array_equal(src.K(), before), "dK was written"
    check_factor(out, Kk, Uk, ak, f"({n0}, r={len(idx)})")
    return src, out


# ---------------------------------------------------------------------------------------
# shapes, routes, repeatability
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("pad,pado", [(0, 0), (7, 3)])
@pytest.mark.parametrize("case", RM.GPU_SHAPES, ids=RM.shape_id)
def test_shapes(case, pad, pado, route, knobs):
    knobs("GPR_REMOVE_SWEEP", route)
    assert G.default_context().get_knob("GPR_REMOVE_SWEEP") == route
    run_case(*case, pad=pad, pado=pado)


@pytest.mark.parametrize("case", RM.GPU_SHAPES, ids=RM.shape_id)
def test_routes_and_calls_agree_bit_for_bit(case, knobs):
    n0, idx = case
    x, y, hp, Kk, Uk, ak = reference(n0, tuple(idx))
    src = Fit(KINDS, hp, x, y, ld=n0 + 1)
    outs = []
    for route in (0, 1, 1, 0):
        knobs("GPR_REMOVE_SWEEP", route)
        o = Removed(src, idx, ldo=n0 - len(idx) + 2)
        outs.append((o.K(), o.a()))
    for K1, a1 in outs[1:]:
        assert np.array_equal(outs[0][0], K1) and np.array_equal(outs[0][1], a1)


def test_long_chain_of_hops_route_1_against_route_0(knobs):
    """65 column blocks: more hops of the hand-off than the small shapes give; compared on the
    device, no CPU reference at this size"""
    import torch
    n0, idx = RM.LONG_CHAIN["n0"], RM.LONG_CHAIN["idx"]
    rng = np.random.default_rng(17)
    x = rng.random((D_IN, n0))
    hp = R.model_hp(KINDS, D_IN, rng, lscale=0.3, noise=0.1)
    src = Fit(KINDS, hp, x, np.cos(x.sum(0)))
    outs = []
    for route in (0, 1):
        knobs("GPR_REMOVE_SWEEP", route)
        outs.append(Removed(src, idx))
    src.ctx.sync()
    assert torch.equal(outs[0].dK, outs[1].dK) and torch.equal(outs[0].alpha, outs[1].alpha)
    n = n0 - len(idx)
    diag = torch.diagonal(outs[1].dK[:, :n])
    assert bool(torch.all(torch.isfinite(outs[1].dK))) and bool(torch.all(diag > 0))


def test_two_columns_of_y_with_a_padded_ldy():
    c = RM.NRHS_CASE
    run_case(c["n0"], c["idx"], ny=c["ny"], ldy_pad=c["ldy_pad"])


# ---------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------
def test_chained_removals():
    n = RM.CHAIN["n0"]
    x, y, hp, K, U, alpha = A.make_case(KINDS, n, 0, D_IN)
    dev, alive = Fit(KINDS, hp, x, y), np.arange(n)
    for idx in RM.CHAIN["steps"]:
        dev = Removed(dev, idx)
        alive = alive[RM.keep_of(len(alive), idx)]
        check_factor(dev, *RM.kept_fit(K, y, alive), f"chain -{len(idx)}")
    assert dev.n == 400 - 137


def test_sliding_window():
    """12 rounds at window 256: gpr_fit_remove of the oldest point, gpr_fit_append of a new one (in
    the removal's output buffer, which has the room), against the full fit of the final window"""
    w, rounds = RM.SLIDE["window"], RM.SLIDE["rounds_gpu"]
    x, y, hp, K, U, alpha = A.make_case(KINDS, w, RM.SLIDE["rounds_cpu"], D_IN)
    dev = Fit(KINDS, hp, x[:, :w], y[:w])
    ctx, L = dev.ctx, dev.L
    for lo in range(1, rounds + 1):
        out = Removed(dev, [0], ldo=w, room=1)
        xw, yw = x[:, lo:lo + w], y[lo:lo + w]
        dxw, dyw = ctx.colmajor(xw), ctx.colmajor(yw)
        new = ctx.empty(1, w)
        info = ctypes.c_int(-1)
        rc = L.gpr_fit_append(ctx.h, karr(KINDS), len(KINDS), _dp(hp), D_IN, _P(dxw), w - 1, 1,
                              _P(dyw), 1, w, EPS, _P(out.dK), w, _P(out.alpha), _P(new),
                              ctypes.byref(info))
        assert rc == 0 and info.value == 0, L.gpr_last_error(ctx.h)
        out.n, out.alpha, out.x, out.y, out.dx, out.dy = w, new, xw, yw, dxw, dyw
        dev = out
    keep = np.arange(rounds, rounds + w)
    Kk, Uk, ak = RM.kept_fit(K, y, keep)
    buf = dev.K()
    np.testing.assert_allclose(np.triu(buf), np.triu(Uk), **TOL_U)
    low = np.tril_indices(w, -1)
    np.testing.assert_allclose(buf[low], Kk[low], **TOL_K)
    np.testing.assert_allclose(dev.a(), ak, **TOL_U)


# ---------------------------------------------------------------------------------------
# the calls that follow, on the context's factor cache as the removal left it
# ---------------------------------------------------------------------------------------
def test_predict_and_mll_follow_with_no_forget_factor():
    n0, idx = 300, [5, 127, 128, 129, 299]
    x, y, hp, Kk, Uk, ak = reference(n0, tuple(idx))
    src = Fit(KINDS, hp, x, y)
    dev = Removed(src, idx, ldo=n0)
    ctx, L = dev.ctx, dev.L
    m = 19
    xp = np.random.default_rng(3).random((D_IN, m))
    dxp = ctx.colmajor(xp)
    mu, var = ctx.empty(1, m), ctx.empty(m)
    rc = L.gpr_predict(ctx.h, karr(KINDS), len(KINDS), _dp(hp), D_IN, _P(dev.dx), dev.n, _P(dev.dK),
                       dev.ld, _P(dev.alpha), 1, _P(dxp), m, G.GPR_PREDICT_DIAG, EPS, _P(mu), _P(var),
                       m, _P(None))
    assert rc == 0, L.gpr_last_error(ctx.h)
    out = ctypes.c_double(0.0)
    rc = L.gpr_mll(ctx.h, _P(dev.dK), dev.n, dev.ld, _P(dev.dy), _P(dev.alpha), ctypes.byref(out))
    assert rc == 0, L.gpr_last_error(ctx.h)
    ctx.sync()
    mu_o, var_o = R.predict(KINDS, hp, dev.x, dev.y, xp, diagonal_var=True)
    np.testing.assert_allclose(mu.cpu().numpy()[0], mu_o, **TOL_MU)
    np.testing.assert_allclose(var.cpu().numpy(), var_o, rtol=1e-8,
                               atol=1e-8 * R.diag_prior(KINDS, hp, D_IN))
    assert out.value == pytest.approx(O.mll_value(Uk, dev.y, ak), rel=TOL_MLL)


# ---------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------
def test_argument_errors_write_nothing():
    n0, idx = 100, [3, 50]
    x, y, hp, Kk, Uk, ak = reference(n0, tuple(idx))
    src = Fit(KINDS, hp, x, y)
    ctx, L = src.ctx, src.L
    n = n0 - len(idx)
    dy = ctx.colmajor(y[RM.keep_of(n0, idx)])
    dKo, da = ctx.empty(n, n), ctx.empty(1, n)
    dKo.fill_(PAD)
    da.fill_(PAD)
    snap = src.K()
    inside = src.dK.view(-1)[n0 * 10:]  # a window of dK itself: overlaps it

    def call(dK=src.dK, n0_=n0, ldk=n0, ix=idx, r=None, dy_=dy, nrhs=1, ldy=n, out=dKo, ldo=n, a=da,
             null_idx=False):
        ip = ctypes.POINTER(ctypes.c_int)() if null_idx else _ia(ix)
        return L.gpr_fit_remove(ctx.h, _P(dK), n0_, ldk, ip, len(ix) if r is None else r, _P(dy_),
                                nrhs, ldy, _P(out), ldo, _P(a))

    cases = {
        "r=0": ("r=", dict(r=0)), "r>=n0": ("r=", dict(ix=list(range(n0)), ldo=n0, ldy=n0)),
        "nrhs": ("nrhs", dict(nrhs=0)), "ldk": ("ldk", dict(ldk=n0 - 1)), "ldo": ("ldo", dict(ldo=n - 1)),
        "ldy": ("ldy", dict(ldy=n - 1)), "dK": ("dK", dict(dK=None)), "idx": ("idx", dict(null_idx=True)),
        "dy": ("dy", dict(dy_=None)), "dKout": ("dKout", dict(out=None)), "dalpha": ("dalpha", dict(a=None)),
        "descending": ("idx", dict(ix=[50, 3])), "repeated": ("idx", dict(ix=[3, 3])),
        "negative": ("idx", dict(ix=[-1, 3])), "too large": ("idx", dict(ix=[3, n0])),
        "overlap": ("overlaps", dict(out=inside)), "same": ("overlaps", dict(out=src.dK)),
    }
    for name, (word, kw) in cases.items():
        assert call(**kw) == GPR_E_ARG, name
        msg = L.gpr_last_error(ctx.h).decode()
        assert word in msg, (name, msg)
    assert np.array_equal(src.K(), snap)
    ctx.sync()
    assert np.all(dKo.cpu().numpy() == PAD) and np.all(da.cpu().numpy() == PAD)
    assert call() == 0   # and the call with the right arguments still works
    ctx.sync()
    np.testing.assert_allclose(np.triu(dKo.cpu().numpy().T), np.triu(Uk), **TOL_U)
    np.testing.assert_allclose(da.cpu().numpy()[0], ak, **TOL_U)


# ---------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------
def _cov(name):
    if name == "SE+M52+WN":
        return G.SquaredExp() + G.Matern52() + G.WhiteNoise(), [SE, M52, WN]
    return G.SquaredExp() * G.Periodic() + G.WhiteNoise(), None


def _py_model(name, n=220, d=3, ny=1):
    cov, kinds = _cov(name)
    rng = np.random.default_rng(23)
    x = rng.random((d, n))
    s = x.sum(0)
    y = np.cos(s)
    if ny > 1:
        y = np.stack([y, 0.25 * np.sin(2.0 * s) ** 2], axis=1)
    if kinds is not None:
        hp = R.model_hp(kinds, d, rng, lscale=0.3, noise=0.1)
    else:  # SE * PER + WN: sigma, l (d), then the Periodic factor's sigma, l (d), p (d), then sigma_n
        hp = np.concatenate([[1.0], np.full(d, 0.5), [1.0], np.full(d, 1.0), np.full(d, 2.0), [0.1]])
    assert hp.size == G.dim_hp(cov, d)
    return cov, hp, x, y


def _removal(form, n):
    idx = [150, 3, 128, 127, 77, 219, 0, 64, 65, 201, 13]
    if form == "list":
        return sorted(idx), idx
    if form == "unsorted":
        return idx, idx
    mask = np.zeros(n, dtype=bool)
    mask[idx] = True
    return mask, idx


@pytest.mark.parametrize("form", ["list", "unsorted", "mask"])
@pytest.mark.parametrize("name", ["SE+M52+WN", "SE*PER+WN"])
def test_remove_python_layer(name, form):
    cov, hp, x, y = _py_model(name, ny=2)
    n, d = x.shape[1], x.shape[0]
    arg, idx = _removal(form, n)
    keep = RM.keep_of(n, idx)
    md = G.GPRModel(cov, hp, x.copy(), y.copy())
    pc = G.GPRPredictCache(md, 0, capacity=n + 4)
    G.update_predict_cache_(pc, md)
    G.remove_(pc, md, arg)
    assert md.n == len(keep) and pc.ld == n + 4 and md._x_obj is md.x
    np.testing.assert_array_equal(md.x, x[:, keep])
    np.testing.assert_array_equal(md.y, y[keep])
    fresh = G.GPRModel(cov, hp, x[:, keep].copy(), y[keep].copy())
    fc = G.GPRPredictCache(fresh)
    G.update_predict_cache_(fc, fresh)
    ctx = md.ctx
    nk = len(keep)
    np.testing.assert_allclose(ctx.host(pc.wt), ctx.host(fc.wt), **TOL_U)
    np.testing.assert_allclose(np.triu(ctx.host(pc.Kxx)[:nk, :nk]), np.triu(ctx.host(fc.Kxx)),
                               **TOL_U)
    m = 17
    xp = np.random.default_rng(6).random((d, m))
    prior = float(np.max(G.predict(fresh, xp, diagonal_var=True)[1])) + 1.0
    mu, var = ctx.empty(2, m), ctx.empty(m)
    mu_f, var_f = ctx.empty(2, m), ctx.empty(m)
    G.predict_(mu, var, md, xp, pc, True)
    G.predict_(mu_f, var_f, fresh, xp, fc, True)
    np.testing.assert_allclose(ctx.host(mu), ctx.host(mu_f), **TOL_MU)
    np.testing.assert_allclose(ctx.host(var), ctx.host(var_f), rtol=1e-8, atol=1e-8 * prior)
    # predict(md, md.x): the compacted x is the model's own object (the same-object branch)
    mu_s, var_s = G.predict(md, md.x, diagonal_var=True)
    mu_o, var_o = G.predict(fresh, fresh.x, diagonal_var=True)
    np.testing.assert_allclose(mu_s, mu_o, **TOL_MU)
    np.testing.assert_allclose(var_s, var_o, rtol=1e-8, atol=1e-8 * prior)
    # remove_ then append_ within the kept capacity: the removed points come back at the end
    back = sorted(idx)
    G.append_(pc, md, x[:, back].copy(), y[back].copy())
    assert pc.ld == n + 4 and md.n == n
    order = np.concatenate([keep, back])
    full = G.GPRModel(cov, hp, x[:, order].copy(), y[order].copy())
    flc = G.GPRPredictCache(full)
    G.update_predict_cache_(flc, full)
    np.testing.assert_allclose(ctx.host(pc.wt), ctx.host(flc.wt), **TOL_U)


@pytest.mark.parametrize("name", ["SE+M52+WN", "SE*PER+WN"])
def test_remove_mll_cache(name):
    cov, hp, x, y = _py_model(name)
    n = x.shape[1]
    arg, idx = _removal("unsorted", n)
    keep = RM.keep_of(n, idx)
    md = G.GPRModel(cov, hp, x.copy(), y.copy())
    tc = G.MllLossCache(md)
    G.update_cache_(tc, hp, md)
    G.remove_(tc, md, arg)
    fresh = G.GPRModel(cov, hp, x[:, keep].copy(), y[keep].copy())
    want = G.loss(G.MarginalLikelihood(), hp, fresh)
    got = G.loss(G.MarginalLikelihood(), md, tc)   # (the cache's value: nothing refitted)
    assert got == pytest.approx(want, rel=TOL_MLL)
    ft = G.MllLossCache(fresh)
    G.update_cache_(ft, hp, fresh)
    np.testing.assert_allclose(md.ctx.host(tc.alpha), md.ctx.host(ft.alpha), **TOL_U)


def test_remove_refusals_touch_nothing():
    cov, hp, x, y = _py_model("SE+M52+WN")
    n, d = x.shape[1], x.shape[0]
    md = G.GPRModel(cov, hp, x.copy(), y.copy())
    pc = G.GPRPredictCache(md)
    G.update_predict_cache_(pc, md)
    x_before, wt_before, buf_before = md.x, pc.wt, pc.Kxx
    for bad in ([3, 3], [n], [-1], [], list(range(n)), np.zeros(n, dtype=bool), np.ones(n, dtype=bool),
                np.zeros(n - 1, dtype=bool), [1.5]):
        with pytest.raises(ValueError):
            G.remove_(pc, md, bad)
    with pytest.raises(TypeError):
        G.remove_(pc, md, G.Cmap("+", np.zeros((d, 2)), np.zeros((d, 2))))
    with pytest.raises(TypeError, match="MllGradCache"):
        G.remove_(G.MllGradCache(md), md, [0])
    with pytest.raises(TypeError):
        G.remove_(object(), md, [0])
    assert md.n == n and md.x is x_before and pc.wt is wt_before and pc.Kxx is buf_before
    G.remove_(pc, md, 5)   # a plain int
    assert md.n == n - 1
    np.testing.assert_array_equal(md.x, np.delete(x, 5, axis=1))
