"""What a context remembers between calls -- its workspaces and the factor caches keyed on the
caller's pointers -- must never show in a result: every sequence below equals, bit for bit, the
same calls on a fresh context.  Through the C ABI (ctypes), SE + WN, d = 2, at n = 300 (two full
128-blocks and a ragged one; the tile-DAG takes it through a padded copy) and n = 384 (taken
directly).  No tolerances: the comparator is always the library itself.

The leak bound of test_no_leak_over_context_cycles was measured with the library as it was
before the workspaces had one owner: PARENT_LEAK_BYTES, from
profiles/r18_ctx_leak_parent.txt."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gpr_oracle as O

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

lib = G._lib.lib
D = 2
KINDS = [O.SE, O.WN]
KARR = (ctypes.c_int * 2)(1, 2)
EPS = 1e-8
SIZES = [300, 384]
DIAG = G.GPR_PREDICT_DIAG
# free device memory after context cycle 2 minus that after cycle 6, measured on the parent of
# the change that introduced this test (profiles/r18_ctx_leak_parent.txt): the bound
PARENT_LEAK_BYTES = 0


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def hpp(hp):
    return hp.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def make_hp(sigma, length, noise):
    return np.array([sigma, length, 0.8 * length, noise])


HP1 = make_hp(1.0, 1.5, 0.3)
HP2 = make_hp(1.3, 2.2, 0.2)


def data(n, m=0, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    x = rng.random((D, n))
    y = np.sin(3.0 * x.sum(0)) + 0.1 * rng.standard_normal(n)
    return x, y, rng.random((D, m))


def fit(ctx, hp, dx, dy, n, dK, dalpha, ldk=None):
    info = ctypes.c_int(-7)
    rc = lib.gpr_fit(ctx.h, KARR, 2, hpp(hp), D, P(dx), n, P(dy), 1, n, EPS, P(dK), ldk or n,
                     P(dalpha), ctypes.byref(info))
    assert rc == 0 and info.value == 0, lib.gpr_last_error(ctx.h)


def predict(ctx, hp, dx, n, dK, dalpha, dxp, m):
    mu, var = ctx.empty(m), ctx.empty(m)
    rc = lib.gpr_predict(ctx.h, KARR, 2, hpp(hp), D, P(dx), n, P(dK), n, P(dalpha), 1, P(dxp), m,
                         DIAG, EPS, P(mu), P(var), m, None)
    assert rc == 0, lib.gpr_last_error(ctx.h)
    return ctx.host(mu), ctx.host(var)


def fit_predict(ctx, hp, dx, dy, n, dxp, m):
    dK, mu, var = ctx.empty(n, n), ctx.empty(m), ctx.empty(m)
    info = ctypes.c_int(-7)
    rc = lib.gpr_fit_predict(ctx.h, KARR, 2, hpp(hp), D, P(dx), n, P(dy), 1, n, EPS, P(dK), n, None,
                             P(dxp), m, DIAG, P(mu), P(var), m, None, ctypes.byref(info))
    assert rc == 0 and info.value == 0, lib.gpr_last_error(ctx.h)
    return ctx.host(dK), ctx.host(mu), ctx.host(var)


def spd(n, seed):
    x, _, _ = data(n, seed=seed)
    return O.kernel(KINDS, make_hp(1.0, 1.5 + 0.1 * seed, 0.3), x)


def potrf(ctx, dA, n):
    info = ctypes.c_int(-7)
    rc = lib.gpr_potrf_upper(ctx.h, P(dA), n, n, ctypes.byref(info))
    assert rc >= 0, lib.gpr_last_error(ctx.h)
    return info.value


def potrs(ctx, dU, n, b):
    dB = ctx.colmajor(b)
    assert lib.gpr_potrs_upper(ctx.h, P(dU), n, n, P(dB), 1, n) == 0, lib.gpr_last_error(ctx.h)
    return ctx.host(dB)


def fresh_solve(U, b, nb=128):
    """K^{-1} b on a new context that is handed the factor's bits."""
    ctx = G.Context(0, nb=nb)
    return potrs(ctx, ctx.colmajor(U), U.shape[0], b)


@pytest.mark.parametrize("n", SIZES)
def test_refit_in_place(n):
    """gpr_fit with hp1, a posterior, gpr_fit with hp2 into the same buffer, a posterior: as a
    fresh context given only hp2."""
    m = 40
    x, y, xp = data(n, m)

    def run(hps):
        ctx = G.Context(0)
        dx, dy, dxp = ctx.colmajor(x), ctx.colmajor(y), ctx.colmajor(xp)
        dK, dalpha = ctx.empty(n, n), ctx.empty(n)
        for hp in hps:
            fit(ctx, hp, dx, dy, n, dK, dalpha)
            mu, var = predict(ctx, hp, dx, n, dK, dalpha, dxp, m)
        return ctx.host(dK), ctx.host(dalpha), mu, var

    for got, want in zip(run([HP1, HP2]), run([HP2])):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("n", SIZES)
def test_two_live_factors(n):
    """Two buffers factored on one context, solves on A, then B, then A: each as a fresh
    context's solve from that factor."""
    ctx = G.Context(0)
    dA, dB = ctx.colmajor(spd(n, 1)), ctx.colmajor(spd(n, 2))
    assert potrf(ctx, dA, n) == 0 and potrf(ctx, dB, n) == 0
    UA, UB = ctx.host(dA), ctx.host(dB)
    rng = np.random.default_rng(n)
    for dU, U in ((dA, UA), (dB, UB), (dA, UA)):
        b = rng.standard_normal(n)
        assert np.array_equal(potrs(ctx, dU, n, b), fresh_solve(U, b))


@pytest.mark.parametrize("n", SIZES)
def test_failed_factorisation_leaves_no_cache(n):
    """A matrix that is not positive definite returns info > 0 (a normal return); the caller
    then copies a valid factor into the same buffer (same n and ld) and solves from it."""
    ctx = G.Context(0)
    A = spd(n, 3)
    dU = ctx.colmajor(A)
    assert potrf(ctx, dU, n) == 0
    U = ctx.host(dU)
    bad = A.copy()
    bad[200, 200] = -1.0
    dP = ctx.colmajor(bad)
    assert potrf(ctx, dP, n) == 201
    with torch.cuda.stream(ctx.stream):
        dP.copy_(dU)
    ctx.sync()
    b = np.random.default_rng(n + 1).standard_normal(n)
    assert np.array_equal(potrs(ctx, dP, n, b), fresh_solve(U, b))


@pytest.mark.parametrize("n", SIZES)
def test_block_width_between_solves(n):
    """gpr_set_block(64) between two solves on one factor: the second as a fresh context created
    with nb = 64 (the launch-per-block sweeps), the first as a fresh context's own
    factorisation and solve."""
    A = spd(n, 4)
    rng = np.random.default_rng(n + 2)
    b1, b2 = rng.standard_normal(n), rng.standard_normal(n)
    ctx = G.Context(0)
    dU = ctx.colmajor(A)
    assert potrf(ctx, dU, n) == 0
    x1 = potrs(ctx, dU, n, b1)
    assert lib.gpr_set_block(ctx.h, 64) == 0
    x2 = potrs(ctx, dU, n, b2)
    ref = G.Context(0)
    dR = ref.colmajor(A)
    assert potrf(ref, dR, n) == 0
    assert np.array_equal(x1, potrs(ref, dR, n, b1))
    assert np.array_equal(x2, fresh_solve(ctx.host(dU), b2, nb=64))


@pytest.mark.parametrize("n", SIZES)
def test_block_width_there_and_back(n):
    """gpr_set_block(64) then gpr_set_block(128) between two posteriors from one factor (the
    variance solve goes through the outer-square inverses): the second posterior is the first,
    and a fresh context's."""
    m = 40
    x, y, xp = data(n, m, seed=3)

    def run(toggle):
        ctx = G.Context(0)
        dx, dy, dxp = ctx.colmajor(x), ctx.colmajor(y), ctx.colmajor(xp)
        dK, dalpha = ctx.empty(n, n), ctx.empty(n)
        fit(ctx, HP1, dx, dy, n, dK, dalpha)
        first = predict(ctx, HP1, dx, n, dK, dalpha, dxp, m)
        if toggle:
            assert lib.gpr_set_block(ctx.h, 64) == 0 and lib.gpr_set_block(ctx.h, 128) == 0
        return first, predict(ctx, HP1, dx, n, dK, dalpha, dxp, m)

    first, second = run(True)
    ref_first, ref_second = run(False)
    for got, want in zip(first + second + second, ref_first + ref_second + first):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("n", SIZES)
def test_workspace_regrow(n):
    """gpr_predict without dwork at m = 16, 400, 16 (the context's workspace grows, then serves
    the smaller call): each as a fresh context's."""
    x, y, xp = data(n, 400)

    def run(ms):
        ctx = G.Context(0)
        dx, dy = ctx.colmajor(x), ctx.colmajor(y)
        dK, dalpha = ctx.empty(n, n), ctx.empty(n)
        fit(ctx, HP1, dx, dy, n, dK, dalpha)
        return [predict(ctx, HP1, dx, n, dK, dalpha, ctx.colmajor(xp[:, :m]), m) for m in ms]

    got = run([16, 400, 16])
    for (mu, var), m in zip(got, [16, 400, 16]):
        (mu_f, var_f), = run([m])
        assert np.array_equal(mu, mu_f) and np.array_equal(var, var_f)


def cv_batch(ctx, hp, dx, dy, ntot, ntrn, nfold=3):
    ntst = ntot - ntrn
    idx = np.arange(ntot)
    tst = np.stack([idx[f::nfold] for f in range(nfold)]).astype(np.int32)
    trn = np.stack([np.setdiff1d(idx, t) for t in tst]).astype(np.int32)
    assert trn.shape == (nfold, ntrn) and tst.shape == (nfold, ntst)
    lss = np.zeros(nfold)
    ip = ctypes.POINTER(ctypes.c_int)
    rc = lib.gpr_cv_batch(ctx.h, KARR, 2, hpp(hp), D, P(dx), ntot, P(dy), trn.ctypes.data_as(ip),
                          ntrn, tst.ctypes.data_as(ip), ntst, nfold,
                          G._lib.GPR_COST_MAHALANOBIS, EPS,
                          lss.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc == 0, lib.gpr_last_error(ctx.h)
    return lss


@pytest.mark.parametrize("n", SIZES)
def test_released_child_workspaces(n):
    """gpr_cv_batch fold by fold on child contexts (GPR_CV_BATCH=0), whose workspaces are
    released after every call: two runs give identical losses, and a gpr_fit_predict on the
    parent context afterwards is a fresh context's."""
    ntot, m = n * 3 // 2, 40  # 3 folds: n training points each
    x, y, _ = data(ntot, seed=5)
    xf, yf, xp = data(n, m, seed=6)
    ctx = G.Context(0)
    ctx.set_knob("GPR_CV_BATCH", 0)
    dx, dy = ctx.colmajor(x), ctx.colmajor(y)
    l1 = cv_batch(ctx, HP1, dx, dy, ntot, n)
    l2 = cv_batch(ctx, HP1, dx, dy, ntot, n)
    assert np.all(np.isfinite(l1)) and np.array_equal(l1, l2)
    got = fit_predict(ctx, HP2, ctx.colmajor(xf), ctx.colmajor(yf), n, ctx.colmajor(xp), m)
    ref = G.Context(0)
    want = fit_predict(ref, HP2, ref.colmajor(xf), ref.colmajor(yf), n, ref.colmajor(xp), m)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_no_leak_over_context_cycles():
    """Six times: create a context, one call of each family (fit_predict, potri, cv_batch,
    integrate_noise, fit_append, fit_remove, predict_grad, mvn_sample), destroy it.  The device
    memory free after cycle 6 is not below that after cycle 2 by more than the library lost
    before its workspaces had one owner (PARENT_LEAK_BYTES, measured: see the module text)."""
    n0, madd, m, ny = 300, 84, 40, 3
    N = n0 + madd  # 384
    dev = torch.device("cuda", 0)
    x, y, xp = data(N, m, seed=7)
    Y = np.stack([y[:n0] * (1.0 + 0.1 * j) for j in range(ny)], axis=1)
    x3, y3, _ = data(450, seed=8)
    rng = np.random.default_rng(9)
    # every device buffer the calls use, allocated once on the current stream (the framework's
    # allocator caches per stream: nothing it does may move between cycles)
    def up(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)).to(dev)

    def new(*s):
        return torch.empty(*s, dtype=torch.float64, device=dev)

    dx, dy, dxp, dY = up(x), up(y), up(xp), up(Y)
    dx3, dy3 = up(x3), up(y3)
    dZ = up(rng.standard_normal((N, 4)))
    dK, dKinv, dKout = new(N, N), new(n0, n0), new(N, N)
    da0, da1, da2 = new(n0), new(N), new(N)
    mu, var, gmu, gvar, dS = new(m), new(m), new(m, D), new(m, D), new(4, N)
    ridx = (ctypes.c_int * 2)(5, 200)
    lo, hi = (ctypes.c_double * D)(0.0, 0.0), (ctypes.c_double * D)(1.0, 1.0)
    noise = (ctypes.c_double * ny)(0.05, 0.1, 0.2)
    Iout, ivar = (ctypes.c_double * ny)(), (ctypes.c_double * ny)()
    torch.cuda.synchronize()
    free = []
    for _ in range(6):
        ctx = G.Context(0)
        info = ctypes.c_int(-7)
        assert lib.gpr_fit_predict(ctx.h, KARR, 2, hpp(HP1), D, P(dx), n0, P(dy), 1, n0, EPS, P(dK),
                                   N, P(da0), P(dxp), m, DIAG, P(mu), P(var), m, None,
                                   ctypes.byref(info)) == 0 and info.value == 0
        assert lib.gpr_potri_upper(ctx.h, P(dK), n0, N, P(dKinv), n0) == 0
        ctx.set_knob("GPR_CV_BATCH", 0)
        cv_batch(ctx, HP1, dx3, dy3, 450, 300)
        assert lib.gpr_integrate_noise(ctx.h, KARR, 2, hpp(HP1), D, P(dx), n0, P(dY), ny, n0, lo,
                                       hi, noise, EPS, Iout, ivar) == 0, lib.gpr_last_error(ctx.h)
        assert lib.gpr_predict_grad(ctx.h, KARR, 2, hpp(HP1), D, P(dx), n0, P(dK), N, P(da0), 1,
                                    P(dxp), m, 1, EPS, P(gmu), P(gvar), None) == 0
        assert lib.gpr_fit_append(ctx.h, KARR, 2, hpp(HP1), D, P(dx), n0, madd, P(dy), 1, N, EPS,
                                  P(dK), N, P(da0), P(da1), ctypes.byref(info)) == 0
        assert info.value == 0
        assert lib.gpr_mvn_sample(ctx.h, P(dK), N, N, None, P(dZ), 4, N, P(dS), N) == 0
        assert lib.gpr_fit_remove(ctx.h, P(dK), N, N, ridx, 2, P(dy), 1, N, P(dKout), N,
                                  P(da2)) == 0, lib.gpr_last_error(ctx.h)
        ctx.sync()
        ctx.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(dev)[0])
    lost = free[1] - free[5]
    print(f"free device memory after each cycle: {free}; cycle 2 - cycle 6 = {lost} bytes")
    assert lost <= PARENT_LEAK_BYTES
