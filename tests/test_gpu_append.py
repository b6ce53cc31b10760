"""GPU: gpr_fit_append and the Python layer on it (append_) -- conditioning a fitted model on new
observations without refactoring it.

The reference is always the full fit of all n0 + m points (tests/test_append_cpu.py builds it
and shows that the block formulas meet these tolerances on the same inputs).  Tolerances: the
project's own for the same quantities from gpr_fit (tests/test_gpu_parity.py) -- U's upper
triangle and alpha rtol 1e-8 / atol 1e-12, mu rtol 1e-8 / atol 1e-10, the diagonal variance
rtol 1e-8 / atol 1e-8 diag_prior, the strict lower triangle against K rtol 1e-13, the MLL value
rtol 1e-10.
"""
import ctypes

import numpy as np
import pytest

import test_append_cpu as A
import test_periodic_cpu as R
from oracle import gpr_oracle as O
from test_append_cpu import TOL_K, TOL_MLL, TOL_MU, TOL_U
from test_periodic_cpu import M32, M52, PER, SE, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

GPR_E_ARG = -1
EPS = 1e-8
PAD = 7.25  # what the rows of a padded buffer beyond n0 + m are filled with


def cov_of(kinds):
    cls = {SE: G.SquaredExp, WN: G.WhiteNoise, M32: G.Matern32, M52: G.Matern52, PER: G.Periodic}
    c = None
    for k in kinds:
        c = cls[k]() if c is None else c + cls[k]()
    return c


def karr(kinds):
    return (ctypes.c_int * len(kinds))(*[R.KIND_CODE[k] for k in kinds])


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dp(a):
    return np.ascontiguousarray(a).ctypes.data_as(ctypes.POINTER(ctypes.c_double))


class Dev:
    """All N points on the device, a factor buffer of leading dimension ld (N columns, the rows
    beyond N filled with PAD) and y with leading dimension ldy."""

    def __init__(self, kinds, hp, x, y, ld=None, ldy=None):
        self.ctx = ctx = G.default_context()
        self.L = G._lib.lib
        self.kinds, self.hp = kinds, np.ascontiguousarray(hp, dtype=np.float64)
        self.d, self.N = x.shape
        self.ny = 1 if y.ndim == 1 else y.shape[1]
        self.ld = ld or self.N
        self.ldy = ldy or self.N
        self.dx = ctx.colmajor(x)
        Y = np.full((self.ldy, self.ny), PAD)
        Y[:self.N] = y.reshape(self.N, self.ny)
        self.dy = ctx.colmajor(Y)
        self.dK = ctx.empty(self.N, self.ld)
        self.dK.fill_(PAD)
        self.alpha = None
        self.n = 0

    def fit(self, n0, eps=EPS):
        self.alpha = self.ctx.empty(self.ny, n0)
        info = ctypes.c_int(-1)
        rc = self.L.gpr_fit(self.ctx.h, karr(self.kinds), len(self.kinds), _dp(self.hp), self.d,
                            _P(self.dx), n0, _P(self.dy), self.ny, self.ldy, eps, _P(self.dK),
                            self.ld, _P(self.alpha), ctypes.byref(info))
        assert rc == 0 and info.value == 0, self.L.gpr_last_error(self.ctx.h)
        self.n = n0
        return self

    def append(self, m, eps=EPS, expect_ok=True):
        """gpr_fit_append of the next m points; (rc, info)"""
        n0, Nn = self.n, self.n + m
        new = self.ctx.empty(self.ny, Nn)
        info = ctypes.c_int(-1)
        rc = self.L.gpr_fit_append(self.ctx.h, karr(self.kinds), len(self.kinds), _dp(self.hp),
                                   self.d, _P(self.dx), n0, m, _P(self.dy), self.ny, self.ldy, eps,
                                   _P(self.dK), self.ld, _P(self.alpha), _P(new),
                                   ctypes.byref(info))
        if expect_ok:
            assert rc == 0 and info.value == 0, (rc, info.value, self.L.gpr_last_error(self.ctx.h))
        if rc == 0:
            self.alpha, self.n = new, Nn
        return rc, info.value

    def K(self):
        """the whole buffer as a (ld, N) host array"""
        self.ctx.sync()
        return self.dK.cpu().numpy().T.copy()

    def a(self):
        self.ctx.sync()
        h = self.alpha.cpu().numpy()
        return h[0].copy() if self.ny == 1 else h.T.copy()


def check_factor(dev, K_ref, U_ref, alpha_ref, what=""):
    n = dev.n
    buf = dev.K()
    Kd = buf[:n, :n]
    err_u = np.max(np.abs(np.triu(Kd) - np.triu(U_ref)) / (1e-12 + 1e-8 * np.abs(np.triu(U_ref))))
    low = np.tril_indices(n, -1)
    err_k = np.max(np.abs(Kd[low] - K_ref[low]) / np.abs(K_ref[low])) if n > 1 else 0.0
    a = dev.a()
    err_a = np.max(np.abs(a - alpha_ref) / (1e-12 + 1e-8 * np.abs(alpha_ref)))
    print(f"  {what} n={n} ld={dev.ld}: U {err_u:.2e}  alpha {err_a:.2e} of the tolerance; "
          f"lower K rel {err_k:.2e}")
    assert np.all(np.isfinite(np.triu(Kd))) and np.all(np.isfinite(a))
    np.testing.assert_allclose(np.triu(Kd), np.triu(U_ref), **TOL_U)
    np.testing.assert_allclose(Kd[low], K_ref[low], **TOL_K)
    np.testing.assert_allclose(a, alpha_ref, **TOL_U)
    assert np.all(buf[n:dev.N] == PAD) and np.all(buf[dev.N:] == PAD), "wrote outside (n0 + m)^2"
    assert np.all(buf[:n, n:] == PAD)


def posterior_and_mll(dev, x, y, xp):
    """gpr_predict (DIAG) and gpr_mll from the device's factor, no gpr_forget_factor before"""
    ctx, L = dev.ctx, dev.L
    m = xp.shape[1]
    dxp = ctx.colmajor(xp)
    mu, var = ctx.empty(dev.ny, m), ctx.empty(m)
    rc = L.gpr_predict(ctx.h, karr(dev.kinds), len(dev.kinds), _dp(dev.hp), dev.d, _P(dev.dx),
                       dev.n, _P(dev.dK), dev.ld, _P(dev.alpha), dev.ny, _P(dxp), m,
                       G.GPR_PREDICT_DIAG, EPS, _P(mu), _P(var), m, _P(None))
    assert rc == 0, L.gpr_last_error(ctx.h)
    out = ctypes.c_double(0.0)
    rc = L.gpr_mll(ctx.h, _P(dev.dK), dev.n, dev.ld, _P(dev.dy), _P(dev.alpha), ctypes.byref(out))
    assert rc == 0, L.gpr_last_error(ctx.h)
    ctx.sync()
    hm = mu.cpu().numpy()
    return (hm[0].copy() if dev.ny == 1 else hm.T.copy()), var.cpu().numpy().copy(), out.value


def check_posterior(dev, kinds, hp, x, y, U_ref, alpha_ref, seed=3):
    xp = np.random.default_rng(seed).random((x.shape[0], 19))
    mu, var, mll = posterior_and_mll(dev, x, y, xp)
    mu_o, var_o = R.predict(kinds, hp, x, y, xp, diagonal_var=True)
    np.testing.assert_allclose(mu, mu_o, **TOL_MU)
    np.testing.assert_allclose(var, var_o, rtol=1e-8, atol=1e-8 * R.diag_prior(kinds, hp, x.shape[0]))
    y1 = y if y.ndim == 1 else y[:, 0]
    a1 = alpha_ref if alpha_ref.ndim == 1 else alpha_ref[:, 0]
    assert mll == pytest.approx(O.mll_value(U_ref, y1, a1), rel=TOL_MLL)


def run_case(kinds, n0, m, d, ny=1, pad=0, ldy_pad=0, posterior=True):
    x, y, hp, K, U, alpha = A.make_case(kinds, n0, m, d, ny)
    N = n0 + m
    dev = Dev(kinds, hp, x, y, ld=N + pad, ldy=N + ldy_pad).fit(n0)
    before = dev.K()[:n0, :n0]
    a0 = dev.alpha
    a0_before = a0.cpu().numpy().copy()
    dev.append(m)
    assert np.array_equal(dev.K()[:n0, :n0], before), "the old n0 x n0 block was rewritten"
    assert np.array_equal(a0.cpu().numpy(), a0_before), "dalpha0 was written"
    check_factor(dev, K, U, alpha, f"({n0}, {m})")
    if posterior:
        check_posterior(dev, kinds, hp, x, y, U, alpha)
    return dev


# ---------------------------------------------------------------------------------------
# block-edge shapes, kinds, nrhs
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("n0,m", A.SHAPES)
def test_block_edge_shapes(n0, m, pad):
    run_case(A.SHAPE_KINDS, n0, m, A.SHAPE_D, pad=pad)


@pytest.mark.parametrize("d", A.KIND_DS)
@pytest.mark.parametrize("name", list(A.KIND_SETS))
def test_kinds(name, d):
    run_case(A.KIND_SETS[name], *A.KIND_SHAPE, d)


def test_two_columns_of_y_with_a_padded_ldy():
    c = A.NRHS_CASE
    run_case(c["kinds"], c["n0"], c["m"], c["d"], ny=c["ny"], ldy_pad=c["ldy_pad"])


# ---------------------------------------------------------------------------------------
# chained appends, then every consumer of the factor cache
# ---------------------------------------------------------------------------------------
def test_chained_appends_then_the_consumers():
    kinds, d, n = A.CHAIN["kinds"], A.CHAIN["d"], A.CHAIN["n0"]
    total = n + sum(A.CHAIN["steps"])
    x, y, hp, K, U, alpha = A.make_case(kinds, n, total - n, d)
    dev = Dev(kinds, hp, x, y).fit(n)
    for m in A.CHAIN["steps"]:
        dev.append(m)
        n += m
        Kf = A.kernel(kinds, hp, x[:, :n])
        Uf = O.chol_upper(Kf)
        buf = dev.K()[:n, :n]
        np.testing.assert_allclose(np.triu(buf), Uf, **TOL_U)
        low = np.tril_indices(n, -1)
        np.testing.assert_allclose(buf[low], Kf[low], **TOL_K)
        np.testing.assert_allclose(dev.a(), O.cho_solve_upper(Uf, y[:n]), **TOL_U)
    assert n == total
    ctx, L = dev.ctx, dev.L
    xp = np.random.default_rng(8).random((d, 23))
    dxp = ctx.colmajor(xp)
    rng = np.random.default_rng(9)
    B = rng.standard_normal((total, 3))

    def consumers(dv):
        mu, var, mll = posterior_and_mll(dv, x, y, xp)
        gm, gv = ctx.empty(1, 23, d), ctx.empty(23, d)
        rc = L.gpr_predict_grad(ctx.h, karr(kinds), len(kinds), _dp(hp), d, _P(dv.dx), total,
                                _P(dv.dK), dv.ld, _P(dv.alpha), 1, _P(dxp), 23, 1, EPS, _P(gm),
                                _P(gv), _P(None))
        assert rc == 0, L.gpr_last_error(ctx.h)
        dB = ctx.colmajor(B)
        rc = L.gpr_potrs_upper(ctx.h, _P(dv.dK), total, dv.ld, _P(dB), 3, total)
        assert rc == 0, L.gpr_last_error(ctx.h)
        ctx.sync()
        return mu, var, mll, gm.cpu().numpy(), gv.cpu().numpy(), dB.cpu().numpy()

    got = consumers(dev)      # (the context's cache: left by the last append)
    fresh = Dev(kinds, hp, x, y).fit(total)   # the same calls on a fresh gpr_fit of all points
    want = consumers(fresh)
    prior = O.diag_prior([O.SE, O.WN], hp, d)
    np.testing.assert_allclose(got[0], want[0], **TOL_MU)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-8, atol=1e-8 * prior)
    assert got[2] == pytest.approx(want[2], rel=TOL_MLL)
    for g, w in zip(got[3:5], want[3:5]):
        assert np.linalg.norm(g - w) <= 1e-8 * np.linalg.norm(w)
    np.testing.assert_allclose(got[5], want[5], rtol=1e-8, atol=1e-8 * np.abs(want[5]).max())
    mu_o, var_o = O.predict([O.SE, O.WN], hp, x, y, xp, diagonal_var=True)
    np.testing.assert_allclose(got[0], mu_o, **TOL_MU)
    np.testing.assert_allclose(got[1], var_o, rtol=1e-8, atol=1e-8 * prior)
    # and back on the appended buffer after the fresh one took the cache
    mu2, var2, mll2 = posterior_and_mll(dev, x, y, xp)
    np.testing.assert_allclose(var2, var_o, rtol=1e-8, atol=1e-8 * prior)


# ---------------------------------------------------------------------------------------
# knob, determinism
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("n0,m", A.KNOB_SHAPES)
def test_both_routes_of_the_skinny_solve(n0, m, route, knobs):
    knobs("GPR_APPEND_SWEEP", route)
    assert G.default_context().get_knob("GPR_APPEND_SWEEP") == route
    run_case(A.SHAPE_KINDS, n0, m, A.SHAPE_D, posterior=False)


def test_two_appends_agree_bit_for_bit(knobs):
    kinds, (n0, m), d = [SE, M52, WN], (1037, 21), 3
    x, y, hp, K, U, alpha = A.make_case(kinds, n0, m, d)
    outs = []
    for _ in range(2):
        dev = Dev(kinds, hp, x, y).fit(n0)
        dev.append(m)
        outs.append((dev.K(), dev.a()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    check_factor(dev, K, U, alpha, "determinism case")


# ---------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------
def test_not_positive_definite_leaves_the_old_model_usable():
    c = A.NOT_PD
    x, y, hp = A.not_pd_case()
    n0 = c["n0"]
    dev = Dev(c["kinds"], hp, x, y).fit(n0)
    before = dev.K()[:n0, :n0]
    a0 = dev.alpha
    a0_before = a0.cpu().numpy().copy()
    rc, info = dev.append(1, eps=c["eps_append"], expect_ok=False)
    assert info == n0 + 1 and rc == n0 + 1
    assert np.array_equal(dev.K()[:n0, :n0], before)
    assert dev.alpha is a0 and np.array_equal(a0.cpu().numpy(), a0_before)
    # the old model still predicts, and a correct append of the same point succeeds
    xo, yo = x[:, :n0], y[:n0]
    dev_n = dev.n
    assert dev_n == n0
    xp = np.random.default_rng(4).random((c["d"], 11))
    dxp = dev.ctx.colmajor(xp)
    mu, var = dev.ctx.empty(1, 11), dev.ctx.empty(11)
    rcp = dev.L.gpr_predict(dev.ctx.h, karr(dev.kinds), len(dev.kinds), _dp(hp), dev.d, _P(dev.dx),
                            n0, _P(dev.dK), dev.ld, _P(dev.alpha), 1, _P(dxp), 11,
                            G.GPR_PREDICT_DIAG, EPS, _P(mu), _P(var), 11, _P(None))
    assert rcp == 0
    dev.ctx.sync()
    mu_o, var_o = O.predict([O.SE, O.WN], hp, xo, yo, xp, diagonal_var=True)
    np.testing.assert_allclose(mu.cpu().numpy()[0], mu_o, **TOL_MU)
    dev.append(1)
    Kf = A.kernel(c["kinds"], hp, x)
    Uf = O.chol_upper(Kf)
    check_factor(dev, Kf, Uf, O.cho_solve_upper(Uf, y), "after the failed append")


def test_argument_errors_write_nothing():
    kinds, n0, m, d = [SE, WN], 100, 4, 2
    x, y, hp, K, U, alpha = A.make_case(kinds, n0, m, d)
    dev = Dev(kinds, hp, x, y).fit(n0)
    ctx, L = dev.ctx, dev.L
    N = n0 + m
    new = ctx.empty(1, N)
    new.fill_(PAD)
    snap = dev.K()
    info = ctypes.c_int(-7)

    def call(n0_=n0, m_=m, ldk=N, dX=dev.dx, dy=dev.dy, dK=dev.dK, a0=dev.alpha, a1=new, nrhs=1):
        return L.gpr_fit_append(ctx.h, karr(kinds), len(kinds), _dp(hp), d, _P(dX), n0_, m_, _P(dy),
                                nrhs, N, EPS, _P(dK), ldk, _P(a0), _P(a1), ctypes.byref(info))

    cases = {
        "m": dict(m_=0), "n0": dict(n0_=0), "ldk": dict(ldk=N - 1), "dX": dict(dX=None),
        "dy": dict(dy=None), "dK": dict(dK=None), "dalpha0": dict(a0=None), "dalpha": dict(a1=None),
        "distinct": dict(a1=dev.alpha),
    }
    for name, kw in cases.items():
        assert call(**kw) == GPR_E_ARG, name
        msg = L.gpr_last_error(ctx.h).decode()
        assert name in msg, (name, msg)
        assert info.value == -7, "info written on an argument error"
    assert np.array_equal(dev.K(), snap)
    ctx.sync()
    assert np.all(new.cpu().numpy() == PAD)
    dev.append(m)   # and the call with the right arguments still works
    check_factor(dev, K, U, alpha, "after the refused calls")


# ---------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------
def _py_case(ny, n0=200, steps=(3, 60), d=2):
    kinds = [SE, WN]
    total = n0 + sum(steps)
    x, y, hp, K, U, alpha = A.make_case(kinds, n0, total - n0, d, ny)
    return kinds, x, y, hp, n0, steps, U, alpha


@pytest.mark.parametrize("ny", [1, 2])
@pytest.mark.parametrize("capacity", [True, False])
def test_append_python_layer(ny, capacity):
    kinds, x, y, hp, n0, steps, U, alpha = _py_case(ny)
    d, total = x.shape
    md = G.GPRModel(cov_of(kinds), hp, x[:, :n0].copy(), y[:n0].copy())
    pc = G.GPRPredictCache(md, 0, capacity=total + 5) if capacity else G.GPRPredictCache(md)
    assert pc.ld == (total + 5 if capacity else n0)
    G.update_predict_cache_(pc, md)
    n, lds = n0, [pc.ld]
    for m in steps:
        G.append_(pc, md, x[:, n:n + m].copy(), y[n:n + m].copy())
        n += m
        lds.append(pc.ld)
        assert md.n == n and md.y.shape[0] == n
    if capacity:
        assert lds == [total + 5] * 3
    else:  # two regrowths (200 -> 256 for 203 points, -> 384 for 263), multiples of 16
        assert lds[0] < lds[1] < lds[2] and all(v % 16 == 0 for v in lds[1:]) and lds[2] >= total
    np.testing.assert_array_equal(md.x, x)
    np.testing.assert_array_equal(md.y, y)
    ctx = md.ctx
    wt = ctx.host(pc.wt)
    np.testing.assert_allclose(wt, alpha, **TOL_U)
    np.testing.assert_allclose(np.triu(ctx.host(pc.Kxx)[:total, :total]), U, **TOL_U)
    # predict_ (diag and full), predict_mean_, predict_grad_ from the appended cache
    okinds = [O.SE, O.WN]
    m = 17
    xp = np.random.default_rng(6).random((d, m))
    prior = O.diag_prior(okinds, hp, d)
    mu = ctx.empty(ny, m) if ny > 1 else ctx.empty(m)
    var, Sig = ctx.empty(m), ctx.empty(m, m)
    mu_o, var_o = O.predict(okinds, hp, x, y, xp, diagonal_var=True)
    _, Sig_o = O.predict(okinds, hp, x, y, xp, diagonal_var=False)
    G.predict_(mu, var, md, xp, pc, True)
    np.testing.assert_allclose(ctx.host(mu), mu_o, **TOL_MU)
    np.testing.assert_allclose(ctx.host(var), var_o, rtol=1e-8, atol=1e-8 * prior)
    G.predict_(mu, Sig, md, xp, pc, False)
    np.testing.assert_allclose(ctx.host(Sig), Sig_o, rtol=1e-8, atol=1e-8 * prior)
    mu.zero_()
    G.predict_mean_(mu, md, xp, pc)
    np.testing.assert_allclose(ctx.host(mu), mu_o, **TOL_MU)
    import test_predict_grad_cpu as PG
    gm_o, gv_o = PG.posterior_grad(kinds, hp, x, y, xp)
    dmu = ctx.empty(ny, m, d) if ny > 1 else ctx.empty(m, d)
    dvar = ctx.empty(m, d)
    G.predict_grad_(dmu, dvar, md, xp, pc)
    ctx.sync()
    gm = dmu.cpu().numpy()
    gm = gm.transpose(0, 2, 1) if ny > 1 else gm.T[None]
    gm_o = gm_o if gm_o.ndim == 3 else gm_o[None]
    assert np.linalg.norm(gm - gm_o) <= 1e-8 * np.linalg.norm(gm_o)
    assert np.linalg.norm(dvar.cpu().numpy().T - gv_o) <= 1e-8 * np.linalg.norm(gv_o)
    # predict(md, md.x) takes the same-object branch: the appended x is the model's own object
    assert md._x_obj is md.x
    mu_s, var_s = G.predict(md, md.x, diagonal_var=True)
    mu_so, var_so = O.predict(okinds, hp, x, y, x, diagonal_var=True)   # (`x is x`: same object)
    np.testing.assert_allclose(mu_s, mu_so, **TOL_MU)
    np.testing.assert_allclose(var_s, var_so, rtol=1e-8, atol=1e-8 * prior)


def test_append_mll_cache_and_grad_cache():
    kinds, x, y, hp, n0, steps, U, alpha = _py_case(1)
    md = G.GPRModel(cov_of(kinds), hp, x[:, :n0].copy(), y[:n0].copy())
    tc = G.MllLossCache(md)
    G.update_cache_(tc, hp, md)
    n = n0
    for m in steps:
        G.append_(tc, md, x[:, n:n + m].copy(), y[n:n + m].copy())
        n += m
    L = G.loss(G.MarginalLikelihood(), md, tc)   # (the cache's value: nothing refitted)
    assert L == pytest.approx(O.mll([O.SE, O.WN], hp, x, y), rel=TOL_MLL)
    np.testing.assert_allclose(md.ctx.host(tc.alpha), alpha, **TOL_U)
    gc = G.MllGradCache(md)
    with pytest.raises(TypeError):
        G.append_(gc, md, x[:, :1], y[:1])


def test_append_validation_and_failed_append():
    c = A.NOT_PD
    x, y, hp = A.not_pd_case()
    n0, d = c["n0"], c["d"]
    md = G.GPRModel(cov_of(c["kinds"]), hp, x[:, :n0].copy(), y[:n0].copy())
    pc = G.GPRPredictCache(md, 0, capacity=n0 + 8)
    G.update_predict_cache_(pc, md)
    x_before, wt_before = md.x, pc.wt
    wt_host = md.ctx.host(pc.wt)
    with pytest.raises(ValueError):
        G.append_(pc, md, np.zeros((d + 1, 2)), np.zeros(2))
    with pytest.raises(ValueError):
        G.append_(pc, md, np.zeros((d, 2)), np.zeros(3))
    with pytest.raises(ValueError):
        G.append_(pc, md, np.zeros((d, 2)), np.zeros((2, 2)))
    with pytest.raises(TypeError):
        G.append_(pc, md, G.Cmap("+", np.zeros((d, 2)), np.zeros((d, 2))), np.zeros(4))
    with pytest.raises(G.PosDefException) as e:
        G.append_(pc, md, x[:, n0:], y[n0:], eps=c["eps_append"])
    assert e.value.info == n0 + 1
    assert md.n == n0 and md.x is x_before and pc.wt is wt_before
    assert np.array_equal(md.ctx.host(pc.wt), wt_host)
    G.append_(pc, md, x[:, n0:], y[n0:])
    Uf = O.chol_upper(A.kernel(c["kinds"], hp, x))
    np.testing.assert_allclose(md.ctx.host(pc.wt), O.cho_solve_upper(Uf, y), **TOL_U)
