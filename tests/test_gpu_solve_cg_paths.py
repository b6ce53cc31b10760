"""GPU: the paths of the matrix-free conjugate-gradient solve (gpr_solve_cg) that
tests/test_gpu_solve_cg.py does not reach, on the problems of tests/cg_ref.py (their preconditions
are asserted on the CPU by tests/test_cg_ref_cpu.py):

  n > 1024           two and three blocks in the two-stage sums, the last one ragged (P1, P2)
  the product        grouped launches adding into Q (P3), a product term with a Periodic factor
                     (P4), the run-time-S tile (P5), 64 staged columns of V (nrhs = 17)
  frozen columns     a column that has met the stop test keeps x, r and p while the others go on
  zero columns       frozen at once; B = 0 ends before the first product
  ldb > n, ldx > n   through the C ABI (the Python wrapper passes ldx = n)
  maxit = 0, exact power-of-two scalings of B, two calls bit for bit, GPR_KMM_SLABS
  argument errors    GPR_E_ARG naming the argument, nothing written

Bounds: relres <= 10 tol and ||x - x_ref|| / ||x_ref|| <= cond_2 relres as in
tests/test_gpu_solve_cg.py, x_ref = solve(K_ref, B) in float64 on the long-double reference
kernel; everything else is exact equality, argued from cg.hip and kmatmul.hip where it is asserted.
Every call goes through the C ABI with X pre-filled with a sentinel, its padding rows included.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cg_ref as C
import kernel_ref_ld as R
import test_product_cpu as PR

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

SENT = -7.5
GPR_E_ARG = -1


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _karr(desc):
    c = PR.codes(desc)
    return (ctypes.c_int * len(c))(*c), len(c)


def _solve(name, B, tol=C.TOL, maxit=None, pad=(0, 0)):
    """(X, iters, relres) of gpr_solve_cg on a problem of cg_ref: B with ldb = n + pad[0], its
    padding rows NaN; X with ldx = n + pad[1], pre-filled with the sentinel, which must be gone
    from every element of the solution and still stand in the padding."""
    desc, hp, x = C.inputs(name)
    ctx = G.default_context()
    d, n = x.shape
    B = np.asarray(B, dtype=np.float64).reshape(n, -1)
    nrhs = B.shape[1]
    dB = torch.full((nrhs, n + pad[0]), float("nan"), dtype=torch.float64, device=ctx.device)
    dB[:, :n] = torch.from_numpy(np.ascontiguousarray(B.T)).to(ctx.device)
    dX = torch.full((nrhs, n + pad[1]), SENT, dtype=torch.float64, device=ctx.device)
    torch.cuda.synchronize()
    dx = ctx.colmajor(x)
    ka, nk = _karr(desc)
    hpa = np.array(hp)  # (held: the pointer does not own it)
    iters, relres = ctypes.c_int(-7), np.full(nrhs, SENT)
    rc = G._lib.lib.gpr_solve_cg(ctx.h, ka, nk, _dp(hpa), d, _P(dx), n, _P(dB), nrhs, n + pad[0],
                                 R.EPS, tol, C.reference(name)[3] if maxit is None else maxit,
                                 _P(dX), n + pad[1], ctypes.byref(iters), _dp(relres))
    assert rc == 0, G._lib.lib.gpr_last_error(ctx.h)
    ctx.sync()
    o = dX.cpu().numpy()
    assert np.all(o[:, n:] == SENT), "X's padding was written"
    assert not np.any(o[:, :n] == SENT), "an element of X was not written"
    return o[:, :n].T.copy(), iters.value, relres


@functools.lru_cache(maxsize=None)
def _rhs_and_solution(name, nrhs):
    """(B, x_ref): computed once per case, never written"""
    B = C.rhs(name, nrhs)
    Xs = np.linalg.solve(C.reference(name)[0], B)
    B.setflags(write=False)
    Xs.setflags(write=False)
    return B, Xs


def _check_accuracy(name, X, iters, relres, B, Xs, tol=C.TOL):
    _, cond, _, maxit = C.reference(name)
    err = np.linalg.norm(X - Xs, axis=0) / np.linalg.norm(Xs, axis=0)
    print(f"{name} nrhs={B.shape[1]}: iters {iters} (maxit {maxit}), max relres {relres.max():.3g}, "
          f"max err / (cond relres) {np.max(err / (cond * relres)):.3g}, cond {cond:.1f}")
    assert iters < maxit
    assert relres.shape == (B.shape[1],) and np.all(relres <= 10 * tol)
    assert np.all(err <= cond * relres)
    return err


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("name", list(C.PROBLEMS))
def test_converges_to_the_dense_solution(name, nrhs):
    B, Xs = _rhs_and_solution(name, nrhs)
    X, iters, relres = _solve(name, B)
    _check_accuracy(name, X, iters, relres, B, Xs)


def test_wide_right_hand_side():
    """nrhs = 17: the product stages 64 columns of V (NVB = 4), on grouped launches"""
    B, Xs = _rhs_and_solution("P3", 17)
    X, iters, relres = _solve("P3", B)
    _check_accuracy("P3", X, iters, relres, B, Xs)


def test_a_converged_column_freezes():
    """[b_fast | b_slow | b_fast] jointly against b_fast and b_slow alone: every joint column is
    the solo column bit for bit, and the call runs as long as the slow column needs.
    Why the bits agree: nrhs = 1 and 3 both take the NVB = 1 instance of the product; its slab
    count (kmm_launch) depends on na and nb, not on nv; the MFMA forms row vcol of Out^T from row
    vcol of V^T alone, and kmm_reduce_kernel and every cg_* kernel index a column by blockIdx.y or
    t / na and read no other column.  A frozen column's x, r and p are not touched again
    (cg_step_xr_kernel and cg_step_p_kernel return on the flag), and relres comes from one more
    product of the same x."""
    b_fast, b_slow = C.fast_and_slow()
    tol = C.FAST_SLOW_TOL
    Xj, itj, rrj = _solve("P1", np.column_stack([b_fast, b_slow, b_fast]), tol=tol)
    Xf, itf, rrf = _solve("P1", b_fast, tol=tol)
    Xs, its, rrs = _solve("P1", b_slow, tol=tol)
    print(f"iters: joint {itj}, fast {itf}, slow {its}; relres joint {rrj}")
    assert np.all(rrj <= 10 * tol)
    assert itf + 5 <= its and itj == its
    assert np.array_equal(Xj[:, 0], Xf[:, 0]) and np.array_equal(Xj[:, 2], Xf[:, 0])
    assert np.array_equal(Xj[:, 1], Xs[:, 0])
    assert rrj[0] == rrf[0] == rrj[2] and rrj[1] == rrs[0]


def test_zero_columns():
    b = C.rhs("P1", 1)[:, 0]
    z = np.zeros_like(b)
    X1, it1, rr1 = _solve("P1", b)
    X, it, rr = _solve("P1", np.column_stack([b, z, b]))
    assert np.all(X[:, 1] == 0.0) and rr[1] == 0.0
    assert np.array_equal(X[:, 0], X1[:, 0]) and np.array_equal(X[:, 2], X1[:, 0])
    assert it == it1 and rr[0] == rr1[0] == rr[2]
    X, it, rr = _solve("P1", np.column_stack([z, z]))
    assert it == 0 and np.all(X == 0.0) and np.all(rr == 0.0)


@pytest.mark.parametrize("name", ["P1", "P4"])
def test_padded_leading_dimensions(name):
    B = C.rhs(name, 3)
    X, it, rr = _solve(name, B)
    Xp, itp, rrp = _solve(name, B, pad=(7, 5))
    assert np.array_equal(X, Xp) and it == itp and np.array_equal(rr, rrp)


def test_maxit_zero():
    """x = 0 and relres = 1.0 exactly: cg_resid_kernel forms b - 0 = b and sums its squares by the
    fused multiply-adds, the strides and the two trees cg_init_kernel and cg_init_scalars_kernel
    sum b.b by (cg_sum_kernel's tree is cg_init_scalars_kernel's), so the quotient is 1.0."""
    X, it, rr = _solve("P1", C.rhs("P1", 3), maxit=0)
    assert it == 0 and np.all(X == 0.0) and np.all(rr == 1.0)


def test_power_of_two_scaling_is_exact():
    """B 2^100 and B 2^-100: no operation of the recurrence or of the product rounds differently
    under an exact scaling that stays in range (the stop test compares r.r with tol^2 b.b, both
    scaled by its square; alpha and beta are quotients of equally scaled sums)."""
    B = C.rhs("P1", 3)
    X, it, rr = _solve("P1", B)
    for s in (2.0 ** 100, 2.0 ** -100):
        Xs, its, rrs = _solve("P1", B * s)
        assert its == it and np.array_equal(rrs, rr)
        assert np.array_equal(Xs, X * s)


def test_two_calls_agree_bit_for_bit():
    B = C.rhs("P2", 3)
    X, it, rr = _solve("P2", B)
    X2, it2, rr2 = _solve("P2", B)
    assert it == it2 and np.array_equal(rr, rr2) and np.array_equal(X, X2)


def test_slab_count_changes_the_summation_order_only(knobs):
    B, Xs = _rhs_and_solution("P1", 3)
    cond = C.reference("P1")[1]
    out = []
    for slabs in (1, 3):
        knobs("GPR_KMM_SLABS", slabs)
        X, iters, relres = _solve("P1", B)
        _check_accuracy("P1", X, iters, relres, B, Xs)
        out.append((X, relres))
    diff = np.linalg.norm(out[0][0] - out[1][0], axis=0) / np.linalg.norm(Xs, axis=0)
    bound = 2 * cond * max(out[0][1].max(), out[1][1].max())
    print(f"slabs 1 against 3: max difference / bound = {diff.max() / bound:.3g}")
    assert np.all(diff <= bound)


# ---------------------------------------------------------------------------------------
# argument errors: GPR_E_ARG naming the argument, before anything is written
# ---------------------------------------------------------------------------------------
# (what changes, the word the message must carry)
BAD_ARGS = [
    (dict(dX=None), "dX is"), (dict(dB=None), "dB is"), (dict(dXout=None), "dXout is"),
    (dict(n=0), "n="), (dict(nrhs=0), "nrhs"), (dict(nrhs=-1), "nrhs"),
    (dict(ldb=-1), "ldb"), (dict(ldx=-1), "ldx"),
    (dict(tol=0.0), "tol"), (dict(tol=-1e-8), "tol"), (dict(tol=float("nan")), "tol"),
    (dict(maxit=-1), "maxit"),
]


@pytest.mark.parametrize("change,word", BAD_ARGS, ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in BAD_ARGS])
def test_argument_errors(change, word):
    desc, hp, x = C.inputs("P4")
    ctx = G.default_context()
    d, n = x.shape
    nrhs = 2
    dx = ctx.colmajor(x)
    dB = ctx.colmajor(C.rhs("P4", nrhs))
    dX = torch.full((nrhs, n), SENT, dtype=torch.float64, device=ctx.device)
    torch.cuda.synchronize()
    a = dict(dX=dx, n=n, dB=dB, nrhs=nrhs, ldb=n, tol=1e-8, maxit=10, dXout=dX, ldx=n)
    a.update(change)
    for k in ("ldb", "ldx"):  # -1: one short of n
        if a[k] == -1:
            a[k] = n - 1
    ka, nk = _karr(desc)
    hpa = np.array(hp)
    iters, relres = ctypes.c_int(-7), np.full(nrhs, SENT)
    rc = G._lib.lib.gpr_solve_cg(ctx.h, ka, nk, _dp(hpa), d, _P(a["dX"]), a["n"], _P(a["dB"]),
                                 a["nrhs"], a["ldb"], R.EPS, a["tol"], a["maxit"], _P(a["dXout"]),
                                 a["ldx"], ctypes.byref(iters), _dp(relres))
    msg = G._lib.lib.gpr_last_error(ctx.h).decode()
    assert rc == GPR_E_ARG, (rc, msg)
    assert word in msg, msg
    ctx.sync()
    assert torch.all(dX == SENT).item() and iters.value == -7 and np.all(relres == SENT)
