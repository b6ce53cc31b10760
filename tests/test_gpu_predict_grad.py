"""GPU: gradients of the posterior with respect to the test inputs (gpr_predict_grad and the Python
layer on it) for every kind of part, every feature-width path of the fused pass, the slab
reduction and its determinism.

Expected values: the NumPy restatement of tests/test_predict_grad_cpu.py, which that file pins to
central differences of the restated and of the oracle's predict.  Every accuracy case carries a
WhiteNoise part sigma_n = 0.1 and l_k ~ 0.3 sqrt(8/d), and asserts on the restatement's K that it
is far from diagonal and factorable.

Tolerance: the project's posterior tolerance 1e-8 (tests/test_gpu_parity.py), normwise per output
array, ||g - g_ref||_2 <= 1e-8 ||g_ref||_2 -- gradient entries pass through zero, so an
element-wise rtol has no meaning for them.
"""
import ctypes
import functools

import numpy as np
import pytest

import test_periodic_cpu as R
import test_predict_grad_cpu as PG
from oracle import gpr_oracle as O
from test_periodic_cpu import M32, M52, PER, SE, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

GPR_E_ARG = -1
TOL = 1e-8


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
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def relnorm(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def assert_well_conditioned(K):
    """the restatement's K: far from diagonal (as tests/test_gpu_periodic.py; a single point has
    no off-diagonal), and factorable"""
    n = K.shape[0]
    if n > 1:
        off = K[~np.eye(n, dtype=bool)]
        assert np.median(off) > 0.05, f"median off-diagonal {np.median(off):.3g}: K is nearly diagonal"
    return O.chol_upper(K)


def make_case(kinds, n, m, d, seed, coincident=0):
    rng = np.random.default_rng(seed)
    x, xp = rng.random((d, n)), rng.random((d, m))
    if coincident:
        xp[:, :coincident] = x[:, rng.permutation(n)[:coincident]]
    hp = R.model_hp(kinds, d, rng, lscale=0.3, noise=0.1)
    y = np.sin(3.0 * x.sum(0)) + 0.1 * rng.standard_normal(n)
    assert_well_conditioned(R.kernel(kinds, hp, x))
    return x, y, xp, hp


def fit(ctx, kinds, hp, x, y):
    """gpr_fit: (dx, dU, dalpha, nrhs)"""
    L = G._lib.lib
    d, n = x.shape
    nrhs = 1 if y.ndim == 1 else y.shape[1]
    dx, dy = ctx.colmajor(x), ctx.colmajor(y)
    dU, alpha = ctx.empty(n, n), ctx.empty(nrhs, n)
    info = ctypes.c_int(-1)
    rc = L.gpr_fit(ctx.h, karr(kinds), len(kinds), _dp(hp), d, _P(dx), n, _P(dy), nrhs, n, 1e-8,
                   _P(dU), n, _P(alpha), ctypes.byref(info))
    assert rc == 0 and info.value == 0, L.gpr_last_error(ctx.h)
    return dx, dU, alpha, nrhs


def grad_call(ctx, kinds, hp, d, dx, n, dU, alpha, nrhs, dxp, m, want_var=1, dgvar="new"):
    """gpr_predict_grad into fresh buffers: (gm (nrhs, d, m), gv (d, m) or None)"""
    L = G._lib.lib
    gm = ctx.empty(nrhs, m, d)
    gv = (ctx.empty(m, d) if want_var else None) if isinstance(dgvar, str) else dgvar
    rc = L.gpr_predict_grad(ctx.h, karr(kinds), len(kinds), _dp(hp), d, _P(dx), n, _P(dU), n,
                            _P(alpha), nrhs, _P(dxp), m, want_var, 1e-8, _P(gm), _P(gv), _P(None))
    assert rc == 0, L.gpr_last_error(ctx.h)
    ctx.sync()
    hm = gm.cpu().numpy().transpose(0, 2, 1).copy()
    return hm, (gv.cpu().numpy().T.copy() if gv is not None else None)


def c_abi(kinds, hp, x, y, xp, want_var=1):
    ctx = G.default_context()
    d, n = x.shape
    dx, dU, alpha, nrhs = fit(ctx, kinds, hp, x, y)
    return grad_call(ctx, kinds, hp, d, dx, n, dU, alpha, nrhs, ctx.colmajor(xp), xp.shape[1], want_var)


def check(name, got, want):
    err = relnorm(got, want)
    print(f"  {name}: ||g - ref|| / ||ref|| = {err:.2e}")
    assert np.all(np.isfinite(got))
    assert err <= TOL, f"{name}: {err:.3e} > {TOL}"


# ---------------------------------------------------------------------------------------
# 1. C ABI parity
# ---------------------------------------------------------------------------------------
KSETS = {
    "SE+WN": [SE, WN],
    "WN+SE": [WN, SE],
    "M32+WN": [M32, WN],
    "M52+WN": [M52, WN],
    "PER+WN": [PER, WN],
    "SE+PER+M52+WN": [SE, PER, M52, WN],
    "SEx4+PER+WN": [SE, SE, SE, SE, PER, WN],   # a part beyond the group of four
}
# ragged and exact 64-tiles in both directions; every compile-time feature width (2, 4, 8, 16,
# 32), each both exact and padded; the chunked path for raw d > 32 and for a Periodic part's 16
# dimensions at a time; the degenerate single point
SHAPES = [(1, 1, 1), (63, 2, 2), (65, 37, 3), (130, 64, 8), (98, 65, 10), (70, 9, 11), (66, 5, 17),
          (66, 3, 33)]


@pytest.mark.parametrize("name", list(KSETS))
@pytest.mark.parametrize("n,m,d", SHAPES)
def test_c_abi_parity(name, n, m, d):
    kinds = KSETS[name]
    x, y, xp, hp = make_case(kinds, n, m, d, 1000 * n + 10 * d + len(kinds))
    gm_o, gv_o = PG.posterior_grad(kinds, hp, x, y, xp)
    gm, gv = c_abi(kinds, hp, x, y, xp)
    print(f"{name} n={n} m={m} d={d}")
    assert gm.shape == (1, d, m) and gv.shape == (d, m)
    check("mean", gm[0], gm_o)
    check("variance", gv, gv_o)


# ---------------------------------------------------------------------------------------
# 2. slab boundary, 6. determinism
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _slab_case(S):
    kinds = [SE, M52, WN]
    n, m, d = 2 * S + 37, 5, 2
    x, y, xp, hp = make_case(kinds, n, m, d, 77)
    gm_o, gv_o = PG.posterior_grad(kinds, hp, x, y, xp)
    for a in (gm_o, gv_o):  # (shared between runs of the test: kept unchanged)
        a.setflags(write=False)
    return kinds, x, y, xp, hp, gm_o, gv_o


def test_slab_boundary_and_determinism():
    """n = 2 S + 37 with S the pass's slab length along n (the knob GPR_PGRAD_SLAB): two full slabs
    and a ragged third; and the same call twice into fresh buffers, bit for bit."""
    ctx = G.default_context()
    S = int(ctx.get_knob("GPR_PGRAD_SLAB"))
    assert 64 <= S <= 4096 and S % 64 == 0
    kinds, x, y, xp, hp, gm_o, gv_o = _slab_case(S)
    d, n = x.shape
    m = xp.shape[1]
    dx, dU, alpha, nrhs = fit(ctx, kinds, hp, x, y)
    dxp = ctx.colmajor(xp)
    gm, gv = grad_call(ctx, kinds, hp, d, dx, n, dU, alpha, nrhs, dxp, m)
    print(f"S={S} n={n}")
    check("mean", gm[0], gm_o)
    check("variance", gv, gv_o)
    gm2, gv2 = grad_call(ctx, kinds, hp, d, dx, n, dU, alpha, nrhs, dxp, m)
    assert np.array_equal(gm, gm2) and np.array_equal(gv, gv2)


def test_slab_length_only_cuts_the_sum(knobs):
    """A shorter slab (the knob's floor, 64: three slabs at n = 165) gives the same gradients
    within the tolerance; the knob rounds up to a multiple of 64."""
    kinds = [SE, M52, WN]
    x, y, xp, hp = make_case(kinds, 165, 5, 2, 78)
    gm_o, gv_o = PG.posterior_grad(kinds, hp, x, y, xp)
    knobs("GPR_PGRAD_SLAB", 1)
    assert G.default_context().get_knob("GPR_PGRAD_SLAB") == 64
    gm, gv = c_abi(kinds, hp, x, y, xp)
    check("mean", gm[0], gm_o)
    check("variance", gv, gv_o)
    knobs("GPR_PGRAD_SLAB", 100)
    assert G.default_context().get_knob("GPR_PGRAD_SLAB") == 128


@pytest.mark.parametrize("n,m", [(130, 37), (66, 5)])
def test_both_solves_behind_the_variance_gradient(n, m, knobs):
    """Q = K^-1 K(x, xp) by the sweeps (GPR_PGRAD_SOLVE=0) and by Z = U^-T and two products (1):
    both within the tolerance, each bit for bit the same when repeated; auto takes the products
    for m > max(16, n / 512), the sweeps below."""
    kinds = [SE, M52, WN]
    d = 3
    x, y, xp, hp = make_case(kinds, n, m, d, 21)
    gm_o, gv_o = PG.posterior_grad(kinds, hp, x, y, xp)
    ctx = G.default_context()
    dx, dU, alpha, nrhs = fit(ctx, kinds, hp, x, y)
    dxp = ctx.colmajor(xp)
    got = {}
    for route in (0, 1, -1):
        knobs("GPR_PGRAD_SOLVE", route)
        gm, gv = grad_call(ctx, kinds, hp, d, dx, n, dU, alpha, nrhs, dxp, m)
        check(f"variance, solve {route}", gv, gv_o)
        gm2, gv2 = grad_call(ctx, kinds, hp, d, dx, n, dU, alpha, nrhs, dxp, m)
        assert np.array_equal(gv, gv2) and np.array_equal(gm, gm2)
        got[route] = gv
    assert np.array_equal(got[-1], got[1 if m > 16 else 0])


def test_both_solves_agree_where_the_tile_dag_solves():
    """n = 8192: Z = U^-T has n right-hand sides, which the library solves as a solve-only tile-DAG
    launch from this size on (GPR_DAG_SOLVE's auto rule) -- another path than every small case
    above.  The restatement would need an 8192^2 Cholesky on the host, so here the two routes,
    which share nothing but the factor, check each other: 1e-8 normwise, as everywhere."""
    kinds = [SE, WN]
    n, m, d = 8192, 24, 2
    rng = np.random.default_rng(8)
    x, xp = rng.random((d, n)), rng.random((d, m))
    hp = R.model_hp(kinds, d, rng, lscale=0.3, noise=0.1)
    y = np.sin(3.0 * x.sum(0)) + 0.1 * rng.standard_normal(n)
    ctx = G.Context(0)
    dx, dU, alpha, nrhs = fit(ctx, kinds, hp, x, y)
    dxp = ctx.colmajor(xp)
    got = {}
    for route in (0, 1):
        ctx.set_knob("GPR_PGRAD_SOLVE", route)
        got[route] = grad_call(ctx, kinds, hp, d, dx, n, dU, alpha, nrhs, dxp, m)
    ctx.close()
    assert np.array_equal(got[0][0], got[1][0])  # (the mean pass does not depend on the solve)
    check("variance, products against sweeps", got[1][1], got[0][1])


# ---------------------------------------------------------------------------------------
# 3. coincident points
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [M32, M52])
def test_coincident_points(kind):
    """xp = 9 columns copied from x, then 9 random ones: r = 0 under the square root."""
    kinds = [kind, WN]
    x, y, xp, hp = make_case(kinds, 70, 18, 3, 5, coincident=9)
    assert all(np.any(np.all(x == xp[:, [j]], axis=0)) for j in range(9))
    gm_o, gv_o = PG.posterior_grad(kinds, hp, x, y, xp)
    gm, gv = c_abi(kinds, hp, x, y, xp)
    check("mean", gm[0], gm_o)
    check("variance", gv, gv_o)


# ---------------------------------------------------------------------------------------
# 4. same pointer: always the cross kernel
# ---------------------------------------------------------------------------------------
def test_same_pointer_is_the_cross_kernel():
    kinds = [SE, WN]
    n, d = 66, 3
    x, y, _, hp = make_case(kinds, n, 1, d, 9)
    ctx = G.default_context()
    dx, dU, alpha, nrhs = fit(ctx, kinds, hp, x, y)
    same = grad_call(ctx, kinds, hp, d, dx, n, dU, alpha, nrhs, dx, n)
    import torch
    with torch.cuda.stream(ctx.stream):
        dcopy = dx.clone()
    assert dcopy.data_ptr() != dx.data_ptr()
    copy = grad_call(ctx, kinds, hp, d, dx, n, dU, alpha, nrhs, dcopy, n)
    assert np.array_equal(same[0], copy[0]) and np.array_equal(same[1], copy[1])
    gm_o, gv_o = PG.posterior_grad(kinds, hp, x, y, x)
    check("mean", same[0][0], gm_o)
    check("variance", same[1], gv_o)


# ---------------------------------------------------------------------------------------
# 5. nrhs = 2, want_var = 0
# ---------------------------------------------------------------------------------------
def test_two_columns_and_no_variance():
    kinds = [SE, M32, WN]
    n, m, d = 97, 20, 3
    x, y, xp, hp = make_case(kinds, n, m, d, 3)
    Y = np.stack([y, 2.0 * y - 1.0], axis=1)
    gm_o, gv_o = PG.posterior_grad(kinds, hp, x, Y, xp)
    ctx = G.default_context()
    dx, dU, alpha, nrhs = fit(ctx, kinds, hp, x, Y)
    assert nrhs == 2
    dxp = ctx.colmajor(xp)
    gm, gv = grad_call(ctx, kinds, hp, d, dx, n, dU, alpha, 2, dxp, m)
    assert gm.shape == (2, d, m)
    check("mean, column 1", gm[0], gm_o[0])
    check("mean, column 2", gm[1], gm_o[1])
    check("variance", gv, gv_o)
    # want_var = 0: a NULL dgvar is fine, and a buffer that is passed stays as it was
    gm0, none = grad_call(ctx, kinds, hp, d, dx, n, dU, alpha, 2, dxp, m, want_var=0, dgvar=None)
    assert none is None and np.array_equal(gm0, gm)
    sentinel = ctx.colmajor(np.full((d, m), -7.0))
    gm1, kept = grad_call(ctx, kinds, hp, d, dx, n, dU, alpha, 2, dxp, m, want_var=0, dgvar=sentinel)
    assert np.array_equal(gm1, gm) and np.all(kept == -7.0)


# ---------------------------------------------------------------------------------------
# 7. the Python layer
# ---------------------------------------------------------------------------------------
def test_python_layer():
    kinds = [SE, PER, WN]
    n, m, d = 130, 37, 3
    x, y, xp, hp = make_case(kinds, n, m, d, 12)
    gm_o, gv_o = PG.posterior_grad(kinds, hp, x, y, xp)
    md = G.GPRModel(cov_of(kinds), hp.copy(), x, y)
    gm, gv = G.predict_grad(md, xp)
    assert gm.shape == (d, m) and gv.shape == (d, m)
    check("mean", gm, gm_o)
    check("variance", gv, gv_o)
    # from an updated cache, on device buffers: the same call, bit for bit
    ctx = md.ctx
    pc = G.GPRPredictCache(md, m)
    G.update_predict_cache_(pc, md)
    dm, dv = ctx.empty(m, d), ctx.empty(m, d)
    G.predict_grad_(dm, dv, md, xp, pc)
    assert np.array_equal(ctx.host(dm), gm) and np.array_equal(ctx.host(dv), gv)
    gm_only, none = G.predict_grad(md, xp, var=False)
    assert none is None and np.array_equal(gm_only, gm)
    # a 2-D y: (ny, d, m)
    Y = np.stack([y, 2.0 * y - 1.0], axis=1)
    gm2_o, _ = PG.posterior_grad(kinds, hp, x, Y, xp)
    gm2, gv2 = G.predict_grad(G.GPRModel(cov_of(kinds), hp.copy(), x, Y), xp)
    assert gm2.shape == (2, d, m) and gv2.shape == (d, m)
    check("mean, 2-D y", gm2, gm2_o)
    check("variance, 2-D y", gv2, gv_o)
    cm = G.Cmap("+", xp[:, :3], xp[:, 3:8])
    with pytest.raises(TypeError, match="Cmap"):
        G.predict_grad(md, cm)
    with pytest.raises(TypeError, match="Cmap"):
        G.predict_grad_(dm, dv, md, cm, pc)


# ---------------------------------------------------------------------------------------
# 8. argument errors
# ---------------------------------------------------------------------------------------
def test_argument_errors():
    kinds = [SE, WN]
    n, m, d = 40, 7, 2
    x, y, xp, hp = make_case(kinds, n, m, d, 4)
    ctx = G.default_context()
    L = G._lib.lib
    dx, dU, alpha, nrhs = fit(ctx, kinds, hp, x, y)
    dxp = ctx.colmajor(xp)
    gm, gv = ctx.colmajor(np.full((d, m), -7.0)), ctx.colmajor(np.full((d, m), -7.0))

    def call(m_=m, gm_=gm, gv_=gv, want=1, ldu=n):
        return L.gpr_predict_grad(ctx.h, karr(kinds), 2, _dp(hp), d, _P(dx), n, _P(dU), ldu, _P(alpha),
                                  1, _P(dxp), m_, want, 1e-8, _P(gm_), _P(gv_), _P(None))

    for kw, word in ((dict(m_=0), b"m=0"), (dict(gm_=None), b"dgmu"), (dict(gv_=None), b"dgvar"),
                     (dict(ldu=n - 1), b"ldu")):
        rc = call(**kw)
        msg = L.gpr_last_error(ctx.h)
        assert rc == GPR_E_ARG and word in msg, (kw, rc, msg)
        assert np.all(ctx.host(gm) == -7.0) and np.all(ctx.host(gv) == -7.0)
    assert call() == 0
    assert np.all(np.isfinite(ctx.host(gm))) and np.all(np.isfinite(ctx.host(gv)))
