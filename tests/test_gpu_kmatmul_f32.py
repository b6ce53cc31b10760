"""GPU: the matrix-free product with FP32 kernel evaluation (GPR_KMM_PREC; ``precision="fp32"``)
and the refined CG solve built on it (``precision="mixed"``).

Product bound, u32 = 2^-24, per stationary part with y = l o x - c, Delta = y_a - y_b:
    dD = 2 sum_k |Delta_k| (|y_ak| + |y_bk|) + (d + 4) D,   beta = u32 (W(D) dD + 8 k(D)),
    |out - ref|_ic <= sum_j beta_ij |V_jc| + (1e-13 + (nb + 8) u) sum_j |K_ij| |V_jc|
(the second term is test_gpu_kernel_matmul.py's bound of the FP64 product), ref the long-double
kernel times V.
"""
import numpy as np
import pytest
import torch

import kernel_ref_ld as R
import test_product_cpu as PR
from kernel_ref_ld import CROSS, LD, M32, M52, PER, SAME_OBJECT, SE, SELF, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")
from oracle import gpr_oracle as O  # noqa: E402

U32 = 2.0 ** -24
DESCS = {"SE": [SE], "M32": [M32], "SE+M52+WN": [SE, M52, WN], "5SE+WN": [SE] * 5 + [WN],
         "PER": [PER]}

# (description, d, na, nb, nv, same, GPR_KMM_SLABS, (ldv - nb, ldo - na))
CASES = [
    ("SE", 1, 1, 1, 1, SELF, 0, (0, 0)),
    ("SE", 8, 64, 64, 16, SELF, 0, (0, 0)),             # one tile
    ("SE", 8, 65, 65, 15, SAME_OBJECT, 0, (0, 0)),      # ragged
    ("SE", 21, 130, 130, 16, SELF, 0, (0, 0)),          # run-time k
    ("M32", 3, 200, 200, 1, SELF, 0, (0, 0)),
    ("SE+M52+WN", 8, 300, 300, 16, SELF, 3, (0, 0)),
    ("5SE+WN", 8, 300, 300, 16, SELF, 0, (0, 0)),       # two part groups, the noise on the last
    ("SE+M52+WN", 8, 130, 97, 16, CROSS, 0, (0, 0)),
    ("SE+M52+WN", 8, 200, 200, 65, SELF, 0, (0, 0)),    # a 64-column pass plus a 1-column pass
    ("SE+M52+WN", 8, 130, 130, 17, SELF, 0, (7, 5)),
]


def _inputs(name, d, na, nb, nv, same, seed):
    rng = np.random.default_rng(seed)
    desc = DESCS[name]
    hp = rng.uniform(0.3, 2.0, sum(R.width(k, d) for k in R.flat(desc)))
    xa = rng.random((d, na))
    return desc, hp, xa, rng.random((d, nb)) if same == CROSS else None, rng.standard_normal((nb, nv))


def _run(desc, hp, xa, xb, V, same, pad=(0, 0), **kw):
    """kernel_matmul on device buffers with padded leading dimensions: NaN in V's padding rows, a
    sentinel in Out's"""
    ctx = G.default_context()
    na, (nb, nv) = xa.shape[1], V.shape
    dV = torch.full((nv, nb + pad[0]), float("nan"), dtype=torch.float64, device=ctx.device)
    dV[:, :nb] = torch.from_numpy(np.ascontiguousarray(V.T)).to(ctx.device)
    out = torch.full((nv, na + pad[1]), -7.5, dtype=torch.float64, device=ctx.device)
    torch.cuda.synchronize()
    xp = None if same == SELF else xa if same == SAME_OBJECT else xb
    G.kernel_matmul(PR.cov_of(desc), hp, xa, dV, xp, out=out, **kw)
    ctx.sync()
    o = out.cpu().numpy()
    assert np.all(o[:, na:] == -7.5), "Out's padding was written"
    return o[:, :na].T.copy()


def _beta(desc, hp, xa, xb):
    """the element bound of the FP32 evaluation, summed over the stationary parts"""
    d = xa.shape[0]
    beta = LD(0)
    for kind, h in [kh for t in R.split_hp(desc, hp, d) for kh in t if kh[0] != WN]:
        sa = R.features(kind, h, xa)[0]
        sb = sa if xb is None else R.features(kind, h, xb)[0]
        c = R.centre(sa)[0][:, None]
        ya, yb = np.abs(sa - c), np.abs(sb - c)
        A = sum(np.abs(sa[k][:, None] - sb[k][None, :]) * (ya[k][:, None] + yb[k][None, :])
                for k in range(d))
        D = R.factor_dist_ld(kind, h, xa, xa if xb is None else xb)
        f, w = R.profile_ld(kind, D)[:2]
        beta = beta + LD(U32) * LD(h[0]) ** 2 * (w * (2 * A + (d + 4) * D) + 8 * f)
    return beta


@pytest.mark.parametrize("name,d,na,nb,nv,same,slabs,pad", CASES)
def test_product_against_long_double(knobs, name, d, na, nb, nv, same, slabs, pad):
    knobs("GPR_KMM_SLABS", slabs)
    desc, hp, xa, xb, V = _inputs(name, d, na, nb, nv, same, 1000 * na + nb + nv)
    out = _run(desc, hp, xa, xb, V, same, pad, precision="fp32")
    K = R.kernel_ld(desc, hp, xa, xb, same=same)
    ref = K @ V.astype(LD)
    aV = np.abs(V).astype(LD)
    bound = _beta(desc, hp, xa, xb) @ aV + (1e-13 + (nb + 8) * R.U) * (np.abs(K) @ aV)
    err = np.abs(out.astype(LD) - ref)
    print(f"max |err| / bound = {float(np.max(err / bound)):.3g}")
    assert np.all(np.isfinite(out))
    assert np.all(err <= bound)
    if na == 300:  # the FP32 kernel really ran
        f64 = _run(desc, hp, xa, xb, V, same, pad)
        assert np.max(np.abs(out - f64) / np.abs(f64)) > 2.0 ** -30


def test_identity_columns_keep_the_fp64_diagonal():
    n = 65
    desc, hp, x, _, _ = _inputs("SE+M52+WN", 8, n, n, 1, SELF, 77)
    eye = np.eye(n)
    lo, hi = (np.hstack([_run(desc, hp, x, None, eye[:, c:c + 16], SELF, precision=p)
                         for c in range(0, n, 16)]) for p in ("fp32", "fp64"))
    assert np.array_equal(np.diag(lo), np.diag(hi))
    assert not np.array_equal(lo, hi)


def test_repeatability_and_the_knob(knobs):
    ctx = G.default_context()
    desc, hp, x, _, V = _inputs("SE+M52+WN", 8, 300, 300, 16, SELF, 5)
    a = _run(desc, hp, x, None, V, SELF, precision="fp32")
    assert ctx.get_knob("GPR_KMM_PREC") == 0
    assert np.array_equal(a, _run(desc, hp, x, None, V, SELF, precision="fp32"))
    plain = _run(desc, hp, x, None, V, SELF)
    assert np.array_equal(plain, _run(desc, hp, x, None, V, SELF, precision="fp64"))
    assert not np.array_equal(a, plain)
    pdesc, php, px, _, pV = _inputs("PER", 3, 130, 130, 4, SELF, 6)
    with pytest.raises(ValueError, match="Periodic"):
        _run(pdesc, php, px, None, pV, SELF, precision="fp32")
    with pytest.raises(ValueError, match="precision"):
        _run(desc, hp, x, None, V, SELF, precision="fp16")
    # the C knob at 1 with a Periodic part: the library itself keeps the FP64 kernels.  (The
    # Python wrapper would set the knob to 0 for its call: go to the C ABI.)
    from gpr_amd import core

    def c_call(kdesc, khp, kx, kV):
        kinds, nk = core._kinds_arr(PR.cov_of(kdesc))
        dx, dV = ctx.colmajor(kx), ctx.colmajor(kV)
        n, out = dx.shape[0], ctx.empty(dV.shape[0], dx.shape[0])
        ctx.check(G._lib.lib.gpr_kernel_matmul(ctx.h, kinds, nk, core._hp_arr(khp)[1], dx.shape[1],
                                               core._ptr(dx), n, None, n, SELF, R.EPS, core._ptr(dV),
                                               dV.shape[0], n, core._ptr(out), n), "gpr_kernel_matmul")
        return ctx.host(out)

    pplain, splain = c_call(pdesc, php, px, pV), c_call(desc, hp, x, V)
    knobs("GPR_KMM_PREC", 1)
    pknob, sknob = c_call(pdesc, php, px, pV), c_call(desc, hp, x, V)
    assert ctx.get_knob("GPR_KMM_PREC") == 1
    assert np.array_equal(pknob, pplain)
    assert np.array_equal(sknob, a) and not np.array_equal(sknob, splain)  # (the knob was live)


def _solve_problem(n, noise, nrhs):
    x, y, _ = O.synthetic(3, n, 0)
    hp = O.default_hp([O.SE, O.WN], 3, sigma=1.0, noise=noise)
    B = y if nrhs == 1 else np.column_stack(
        [y] + [np.random.default_rng(c).standard_normal(n) for c in range(1, nrhs)])
    md = G.GPRModel(G.SquaredExp() + G.WhiteNoise(), hp, x, B)
    return md, O.kernel([O.SE, O.WN], hp, x), B.reshape(n, -1)


def _true_residual(K, X, B):
    """(||b - K x|| / ||b|| per column in NumPy, its own uncertainty): the device's K is within the
    project's 1e-13 of this K entry by entry, and the product rounds n times"""
    X = X.reshape(B.shape)
    nb = np.linalg.norm(B, axis=0)
    slack = (1e-13 + B.shape[0] * R.U) * np.linalg.norm(np.abs(K) @ np.abs(X), axis=0) / nb
    return np.linalg.norm(B - K @ X, axis=0) / nb, slack


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("noise", [0.3, 0.05])
@pytest.mark.parametrize("n", [130, 300])
def test_mixed_solve_meets_the_fp64_contract(n, noise, nrhs):
    """test_gpu_solve_cg.py's acceptance: the residual recomputed from the dense K is the returned
    relres (its rtol 1e-6, beside the recomputation's own uncertainty) and meets tol"""
    tol = 1e-10
    md, K, B = _solve_problem(n, noise, nrhs)
    X, iters, relres = G.solve_cg(md, tol=tol, maxit=20 * n, precision="mixed")
    true, slack = _true_residual(K, X, B)
    print(f"iters {iters}, relres {relres}, true {true}, slack {slack}, "
          f"outer {md.ctx.get_knob('GPR_CG_STAT_OUTER')}, fp64 {md.ctx.get_knob('GPR_CG_STAT_F64')}")
    assert iters < 20 * n and relres.shape == (nrhs,)
    assert np.all(true <= relres * (1 + 1e-6) + slack)
    assert np.all(true <= tol + slack) and np.all(relres <= tol * (1 + 4 * R.U))
    assert md.ctx.get_knob("GPR_KMM_PREC") == 0


@pytest.mark.parametrize("tol", [1e-8, 1e-14])
def test_mixed_solve_ill_conditioned(tol):
    """sigma_n = 1e-4: cond_2(K) ~ 1e10, far past 1 / u32; the second column is random.  At tol =
    1e-8 the call must meet the contract by whichever products it takes (measured: three outer steps,
    no fallback -- K~ - K is a smooth relative perturbation with an exact diagonal).  tol = 1e-14
    is below what FP64 residuals of this system reach (n u ||K| |x|| / ||b|| ~ 1e-13): an outer step
    gains less than 4 x, the rest of the call runs on FP64 products and ends at maxit as the plain
    solve does"""
    n, maxit = 300, 4000
    md, K, B = _solve_problem(n, 1e-4, 2)
    X, iters, relres = G.solve_cg(md, tol=tol, maxit=maxit, precision="mixed")
    true, slack = _true_residual(K, X, B)
    print(f"iters {iters}, relres {relres}, true {true}, slack {slack}, "
          f"outer {md.ctx.get_knob('GPR_CG_STAT_OUTER')}, fp64 {md.ctx.get_knob('GPR_CG_STAT_F64')}")
    if tol < 1e-13:
        assert md.ctx.get_knob("GPR_CG_STAT_F64") > md.ctx.get_knob("GPR_CG_STAT_OUTER")
    if iters == maxit:
        assert relres.max() > tol
        np.testing.assert_allclose(relres, true, rtol=1e-6, atol=slack.max())
    else:
        assert np.all(relres <= tol * (1 + 4 * R.U)) and np.all(true <= relres * (1 + 1e-6) + slack)


@pytest.mark.parametrize("desc", [[SE, WN], [SE, M52, WN]], ids=["SE+WN", "SE+M52+WN"])
def test_mixed_mll_grad_free_reproduces_the_dense_gradient(desc):
    """test_gpu_mll_grad_free.py's exact-probe acceptance, the solve by the refined route"""
    import test_gpu_grad_form as GF
    import test_gpu_mll_grad_free as MF
    n = 130
    hp, x, y, md = MF._model(desc, n, n + len(desc))
    g, iters, relres = G.mll_grad_free(md, Z=np.sqrt(n) * np.eye(n), tol=1e-12, maxit=20 * n,
                                       precision="mixed")
    K = R.kernel_ld(desc, hp, x).astype(np.float64)
    Kinv = np.linalg.inv(K).astype(LD)
    a = Kinv @ y.astype(LD)
    ref, T, S = GF.form_ref(desc, hp, x, np.outer(a, a) - Kinv,
                            np.outer(np.abs(a), np.abs(a)) + np.abs(Kinv))
    kappa = np.linalg.cond(K, 2)
    bound = 4 * kappa * relres.max() * S + (1e-13 + (n + (n + 1) + 2 * MF.D + 16) * R.U) * T
    err = np.abs(g.astype(LD) - LD(-0.5) * ref)
    print(f"iters {iters}, max relres {relres.max():.3g}, max |err| / bound = "
          f"{float(np.max(err / bound)):.3g}")
    assert relres.shape == (n + 1,) and np.all(err <= bound)
