"""The tile-DAG's ticket order with tile rows taken in groups (dag.hip dag_task_order;
GPR_DAG_RGROUP / GPR_DAG_RSKEW / GPR_DAG_RGROUP_MIN).

Host only, through gpr_debug_dag_task_order: every grouped list is a permutation of the row
order's and topological (every tile a task reads has an earlier ticket -- the launch's
deadlock-freedom argument), group = 1 is the row order itself, and lower-triangular / gram
launches do not see the knobs.

On the device: the order changes who runs when, never a tile's arithmetic (its accumulation runs
k ascending whatever the piece boundaries), so every result is bit for bit the row
order's.  n = 256 (one full pair), 384 (a partial group of 4, a full pair + partial pair), 640 (a
full group of 4 + 1), 1024 (two groups of 4), 592 (a ragged last tile row of 80); the skew of 2
exceeds the short rows.  Tolerances against the oracle are those of test_gpu_parity.py.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import scipy.linalg as sla

from oracle import gpr_oracle as O

G = pytest.importorskip("gpr_amd")

SE, WN = O.SE, O.WN
DAG_SOLVE, DAG_LOWER, DAG_GRAM = 1, 2, 4
_KNOBS = ("GPR_DAG_RGROUP", "GPR_DAG_RSKEW", "GPR_DAG_RGROUP_MIN")


def relnorm(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# ---- host only: the order itself ---------------------------------------------------------------
def _order(nt, ntr, flags, group, skew, gmin, zlag=4):
    f = G._lib.lib.gpr_debug_dag_task_order
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_uint), ctypes.c_int]
    cap = nt * (nt + 1) + nt * ntr + 1
    buf = (ctypes.c_uint * cap)()
    cnt = f(nt, ntr, flags, zlag, group, skew, gmin, buf, cap)
    assert 0 <= cnt < cap
    return np.frombuffer(buf, dtype=np.uint32, count=cnt).copy()


def _row_order(nt, ntr, solve):
    """Today's list, written out independently of the library."""
    out = []
    for i in range(nt):
        if not solve:
            out += [(i << 16) | j for j in range(i, nt)]
        out += [0x80000000 | (i << 16) | c for c in range(ntr)]
    return np.array(out, dtype=np.uint32)


def _assert_topological(codes, nt, ntr, solve):
    pos = np.argsort(codes, kind="stable")  # codes are distinct: position of each by lookup
    where = dict(zip(codes[pos].tolist(), pos.tolist()))
    big = len(codes)
    posA = np.full((nt, nt), -1 if solve else big)  # (solve-only: U is final from the start)
    posR = np.full((nt, max(ntr, 1)), big)
    for code, p in where.items():
        i, j = (code >> 16) & 0x7FFF, code & 0xFFFF
        if code >> 31:
            posR[i, j] = p
        else:
            posA[i, j] = p
    for code, p in where.items():
        i, j = (code >> 16) & 0x7FFF, code & 0xFFFF
        rhs = code >> 31
        deps = [posA[:i, i], (posR if rhs else posA)[:i, j]]
        if rhs or i != j:
            deps.append(posA[i:i + 1, i])
        latest = max((int(d.max()) for d in deps if d.size), default=-1)
        assert latest < p, (hex(code), latest, p)


@pytest.mark.parametrize("nt", [1, 2, 3, 4, 5, 8, 9, 33])
def test_grouped_order_is_a_topological_permutation(nt):
    for ntr, solve in itertools.product((0, 1, 3), (False, True)):
        flags = DAG_SOLVE if solve else 0
        rows = _row_order(nt, ntr, solve)
        for group, skew, gmin in itertools.product((1, 2, 4), (0, 1, 3, 40), (0, 3, 100)):
            codes = _order(nt, ntr, flags, group, skew, gmin)
            what = (nt, ntr, solve, group, skew, gmin)
            if group == 1:
                assert np.array_equal(codes, rows), what
                continue
            assert np.array_equal(np.sort(codes), np.sort(rows)), what
            _assert_topological(codes, nt, ntr, solve)
            if gmin >= nt:
                assert np.array_equal(codes, rows), what


def test_pair_order_is_the_documented_one():
    F = lambda i: (i << 16) | i  # noqa: E731
    T = lambda i, j: (i << 16) | j  # noqa: E731
    got = _order(4, 0, 0, 2, 0, 0)
    want = [F(0), T(0, 1), F(1), T(0, 2), T(1, 2), T(0, 3), T(1, 3),
            F(2), T(2, 3), F(3)]
    assert got.tolist() == want
    # skew 1: member 1 one column slot behind; gmin 1 rounds up to the pair at row 2
    got = _order(4, 1, 0, 2, 1, 1)
    R = lambda i, c: 0x80000000 | (i << 16) | c  # noqa: E731
    want = [F(0), T(0, 1), T(0, 2), T(0, 3), R(0, 0), F(1), T(1, 2), T(1, 3), R(1, 0),
            F(2), T(2, 3), F(3), R(2, 0), R(3, 0)]
    assert got.tolist() == want
    # the grouped part actually differs from row order where there is a full group
    assert not np.array_equal(_order(8, 3, 0, 4, 0, 0), _row_order(8, 3, False))
    assert not np.array_equal(_order(8, 3, DAG_SOLVE, 2, 1, 0), _row_order(8, 3, True))


@pytest.mark.parametrize("flags", [DAG_LOWER, DAG_LOWER | DAG_GRAM, DAG_SOLVE | DAG_LOWER])
def test_lower_and_gram_orders_ignore_the_knobs(flags):
    for nt in (1, 2, 5, 9, 33):
        base = _order(nt, nt, flags, 1, 0, 32)
        for group, skew, gmin in itertools.product((2, 4), (0, 1, 3, 40), (0, 3, 100)):
            assert np.array_equal(_order(nt, nt, flags, group, skew, gmin), base), (nt, group, skew, gmin)


# ---- on the device -----------------------------------------------------------------------------
_KINDS = [SE, WN]
_DIM = 3
_SETTINGS = [(2, 0), (2, 2), (4, 0), (4, 2)]  # (group, skew), gmin = 0


def _ctx(monkeypatch, group=None, skew=0, gmin=0, **env):
    monkeypatch.setenv("GPR_DAG", "1")
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    if group is not None:
        for k, v in zip(_KNOBS, (group, skew, gmin)):
            monkeypatch.setenv(k, str(v))
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    ctx = G.Context(0)
    if group is not None:
        assert [ctx.get_knob(k) for k in _KNOBS] == [group, skew, gmin]
    else:
        assert ctx.get_knob("GPR_DAG_RGROUP") in (1, 2, 4)
    return ctx


@functools.lru_cache(maxsize=None)
def _problem(n, npred):
    """Inputs and the oracle's results, computed once per shape (callers do not write to them)."""
    x, y, xp = O.synthetic(_DIM, n, npred, seed_train=n, seed_test=npred)
    hp = O.default_hp(_KINDS, _DIM, noise=0.05)
    K = O.kernel(_KINDS, hp, x)
    U = sla.cholesky(K, lower=False)
    alpha = O.cho_solve_upper(U, y)
    mu, var = O.predict(_KINDS, hp, x, y, xp, diagonal_var=True)
    B = np.random.default_rng(n).random((n, 130))
    return x, y, xp, hp, K, U, alpha, mu, var, B


_P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731


def _potrf_and_solves(ctx, K, B):
    """Factorisation alone (no right-hand side), then U^{-T} B for 1 and 130 columns from the
    finished factor."""
    lib = G._lib.lib
    n = K.shape[0]
    dA = ctx.colmajor(K)
    info = ctypes.c_int(-7)
    assert lib.gpr_potrf_upper(ctx.h, _P(dA), n, n, ctypes.byref(info)) >= 0 and info.value == 0
    out = [ctx.host(dA)]
    for nrhs in (1, 130):
        dB = ctx.colmajor(B[:, :nrhs])
        assert lib.gpr_trsm_upper_trans(ctx.h, _P(dA), n, n, _P(dB), nrhs, n) == 0, lib.gpr_last_error(ctx.h)
        out.append(ctx.host(dB))
    return out


def _fit(ctx, hp, x, y):
    """gpr_fit: z = U^{-T} y is the launch's one right-hand-side column."""
    d, n = x.shape
    dx, dy = ctx.colmajor(x), ctx.colmajor(y[:, None])
    K, alpha = ctx.empty(n, n), ctx.empty(n)
    karr = (ctypes.c_int * 2)(1, 2)
    info = ctypes.c_int(-1)
    rc = G._lib.lib.gpr_fit(ctx.h, karr, 2, hp.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), d,
                            _P(dx), n, _P(dy), 1, n, 1e-8, _P(K), n, _P(alpha), ctypes.byref(info))
    assert rc == 0 and info.value == 0, G._lib.lib.gpr_last_error(ctx.h)
    return ctx.host(K), ctx.host(alpha)


def _fit_predict(ctx, hp, x, y, xp):
    """gpr_fit_predict: [K(x, xp) | y], np + 1 right-hand-side columns inside the launch."""
    d, n = x.shape
    m = xp.shape[1]
    dx, dy, dxp = ctx.colmajor(x), ctx.colmajor(y[:, None]), ctx.colmajor(xp)
    K, alpha, mu, var = ctx.empty(n, n), ctx.empty(1, n), ctx.empty(1, m), ctx.empty(m)
    karr = (ctypes.c_int * 2)(1, 2)
    info = ctypes.c_int(-1)
    rc = G._lib.lib.gpr_fit_predict(ctx.h, karr, 2, hp.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                    d, _P(dx), n, _P(dy), 1, n, 1e-8, _P(K), n, _P(alpha), _P(dxp), m,
                                    G.GPR_PREDICT_DIAG, _P(mu), _P(var), m, None, ctypes.byref(info))
    assert rc == 0 and info.value == 0, G._lib.lib.gpr_last_error(ctx.h)
    return ctx.host(K), ctx.host(alpha).ravel(), ctx.host(mu).ravel(), ctx.host(var)


def _run_all(ctx, n, npred):
    x, y, xp, hp, K, _, _, _, _, B = _problem(n, npred)
    res = dict(zip(("U", "X1", "X130"), _potrf_and_solves(ctx, K, B)))
    res.update(zip(("fit_K", "fit_alpha"), _fit(ctx, hp, x, y)))
    res.update(zip(("fp_K", "fp_alpha", "fp_mu", "fp_var"), _fit_predict(ctx, hp, x, y, xp)))
    return res


def _check_oracle(res, n, npred):
    _, _, _, hp, K, U, alpha_o, mu_o, var_o, B = _problem(n, npred)
    assert relnorm(np.triu(res["U"]), U) < 1e-12
    assert np.array_equal(np.tril(res["U"], -1), np.tril(K, -1))
    for name, nrhs in (("X1", 1), ("X130", 130)):
        assert relnorm(res[name], sla.solve_triangular(U, B[:, :nrhs], trans="T")) < 1e-11
    for name in ("fit_K", "fp_K"):
        # the fits factor the K they assembled (strict lower triangle: K itself), which is the
        # oracle's to 1e-13: the factor against the Cholesky of that K (test_gpu_dag_ring.py)
        Kd = res[name]
        np.testing.assert_allclose(np.tril(Kd, -1), np.tril(K, -1), rtol=1e-13, atol=1e-15)
        Kdev = np.tril(Kd) + np.tril(Kd, -1).T
        np.fill_diagonal(Kdev, np.diag(K))
        assert relnorm(np.triu(Kd), sla.cholesky(Kdev, lower=False)) < 1e-11
    for name in ("fit_alpha", "fp_alpha"):
        np.testing.assert_allclose(res[name], alpha_o, rtol=1e-8, atol=1e-10 * np.abs(alpha_o).max())
    np.testing.assert_allclose(res["fp_mu"], mu_o, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(res["fp_var"], var_o, rtol=1e-8, atol=1e-8 * O.diag_prior(_KINDS, hp, _DIM))


# 129 prediction points + y: 130 right-hand-side columns, two column tiles, the second 2 wide;
# (640, 130): 131 columns
@pytest.mark.gpu
@pytest.mark.parametrize("dag_solve", ["auto", "1"])
@pytest.mark.parametrize("n,npred", [(256, 129), (384, 129), (640, 129), (1024, 129), (592, 129),
                                     (640, 130)])
def test_grouped_rows_bitwise_equal_row_order(n, npred, dag_solve, monkeypatch):
    """dag_solve = "1": the solves from the finished factor are solve-only DAG launches, whose
    right-hand-side rows are grouped too."""
    env = {"GPR_FUSED_RHS": "2"}
    if dag_solve == "1":
        env["GPR_DAG_SOLVE"] = "1"
    base = _run_all(_ctx(monkeypatch, 1, 0, 0, **env), n, npred)
    _check_oracle(base, n, npred)
    for group, skew in _SETTINGS:
        got = _run_all(_ctx(monkeypatch, group, skew, 0, **env), n, npred)
        for name in base:
            assert np.array_equal(got[name], base[name]), (name, group, skew)
        _check_oracle(got, n, npred)


@pytest.mark.gpu
def test_grouped_launch_repeats_bitwise(monkeypatch):
    ctx = _ctx(monkeypatch, 4, 2, 0, GPR_FUSED_RHS="2", GPR_DAG_SOLVE="1")
    a = _run_all(ctx, 640, 130)
    b = _run_all(ctx, 640, 130)
    for name in a:
        assert np.array_equal(a[name], b[name]), name


@pytest.mark.gpu
def test_set_knob_on_a_live_context_rebuilds_the_list(monkeypatch):
    """Same shape, same context: the cached list must follow the knobs (a stale list would still
    give the right numbers, so the check is that every setting runs and agrees)."""
    ctx = _ctx(monkeypatch, 1, 0, 0, GPR_FUSED_RHS="2")
    x, y, xp, hp = _problem(640, 130)[:4]
    base = _fit_predict(ctx, hp, x, y, xp)
    for group, skew, gmin in [(2, 0, 0), (4, 2, 0), (2, 1, 3), (1, 0, 0)]:
        for k, v in zip(_KNOBS, (group, skew, gmin)):
            ctx.set_knob(k, v)
        got = _fit_predict(ctx, hp, x, y, xp)
        for u, v in zip(got, base):
            assert np.array_equal(u, v), (group, skew, gmin)


def _fit_kinv(ctx, n):
    kinds, dim = [SE, WN], 4
    x, y, _ = O.synthetic(dim, n, 0, seed_train=n)
    hp = O.default_hp(kinds, dim, noise=0.1)
    dx, dy = ctx.colmajor(x), ctx.colmajor(y)
    K, Kinv, alpha = ctx.empty(n, n), ctx.empty(n, n), ctx.empty(n)
    karr = (ctypes.c_int * 2)(1, 2)
    info = ctypes.c_int(-1)
    rc = G._lib.lib.gpr_fit_kinv(ctx.h, karr, 2, hp.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                 dim, _P(dx), n, _P(dy), 1, n, 1e-8, _P(K), n, _P(alpha), _P(Kinv), n,
                                 ctypes.byref(info))
    assert rc == 0 and info.value == 0
    return ctx.host(K), ctx.host(alpha), ctx.host(Kinv)


@pytest.mark.gpu
def test_fit_kinv_unchanged_by_the_knobs(monkeypatch):
    """The lower-triangular / gram launch keeps its order: same results with the knobs set."""
    env = {"GPR_FUSE_KINV": "2", "GPR_DAG_GRAM": "1"}
    base = _fit_kinv(_ctx(monkeypatch, 1, 0, 0, **env), 384)
    got = _fit_kinv(_ctx(monkeypatch, 4, 2, 0, **env), 384)
    for name, u, v in zip(("K", "alpha", "Kinv"), got, base):
        assert np.array_equal(u, v), name


@pytest.mark.gpu
def test_cv_batch_unchanged_by_the_knobs(monkeypatch):
    """The batched launch keeps its order too (and its child contexts inherit the knobs)."""
    d, n, k = 3, 600, 100
    rng = np.random.default_rng(11 + d)
    x = rng.random((d, n))
    y = np.sin(x.sum(axis=0)) ** 2
    hp = O.default_hp(["SE", "WN"], d, length=2.0)
    cvset = G.kfoldcv(n, k, rng=np.random.default_rng(5))
    out = []
    for group in (1, 4):
        ctx = _ctx(monkeypatch, group, 2 if group > 1 else 0, 0)
        md = G.GPRModel(G.SquaredExp() + G.WhiteNoise(), hp, x, y, ctx=ctx)
        out.append(np.asarray(G.cv_batch(md, G.Mahalanobis(), x, y, cvset)))
    assert np.array_equal(out[0], out[1])
