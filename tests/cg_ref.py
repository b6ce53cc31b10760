"""The recurrence of csrc/cg.hip restated in NumPy float64 on a dense K, and the problem families
of tests/test_gpu_solve_cg_paths.py with their preconditions (asserted here, on the CPU, by
tests/test_cg_ref_cpu.py).  A helper module: nothing here is collected as a test.

A model of the algorithm, not of its bits: the dot products and the dense products K p are
NumPy's.  What it restates, line by line of gpr_solve_cg:
    x = 0, r = b, p = b / diag, rho = b.b                     (cg_init_kernel)
    a column is frozen at once when b.b <= tol^2 b.b           (cg_init_scalars_kernel: b = 0)
    alpha = (rho / diag) / p.q,  x += alpha p,  r -= alpha q   (cg_step_xr_kernel)
    beta = r.r / rho,  p = r / diag + beta p,  rho = r.r       (cg_step_p_kernel)
    frozen when r.r <= tol^2 b.b, per column; a frozen column keeps x, r, p and rho
    the call ends when every column is frozen, or after maxit iterations
diag is K's constant diagonal as cg_diagonal forms it from the description: the first WhiteNoise's
sigma_n^2 plus, per term, the product of its factors' sigma^2 and eps.

K is kernel_ref_ld.kernel_ld(...).astype(float64), the GPR_SELF matrix.

Problems (inputs in the unit cube, hp in [0.3, 2], sigma_n in [0.3, 1], as
test_gpu_mll_grad_free._model; seeds fixed):
    P1  SE+WN      d = 3   n = 1100   two blocks of the two-stage sums, the second ragged
    P2  SE+M52+WN  d = 8   n = 2100   three blocks
    P3  5SE+WN     d = 8   n = 200    two part groups: the second launch adds into Q
    P4  SE*PER+WN  d = 3   n = 130    a product term and the Periodic embedding
    P5  SE+WN      d = 21  n = 129    the run-time-S tile
Preconditions: the NumPy recurrence converges at tol = 1e-10 within the textbook count
0.5 sqrt(cond_2) ln(2 sqrt(cond_2) / tol) (the formula of tests/test_gpu_solve_cg.py); the GPU
tests' maxit is that count times 400 / 231, that test's margin, rounded up.
"""
import functools
import math

import numpy as np

import kernel_ref_ld as R
from kernel_ref_ld import M52, PER, SE, WN

TOL = 1e-10
MARGIN = 400.0 / 231.0

PROBLEMS = {
    "P1": ([SE, WN], 3, 1100, 28),  # (a seed whose b_slow count clears the 20 below by a margin)
    "P2": ([SE, M52, WN], 8, 2100, 12),
    "P3": ([SE, SE, SE, SE, SE, WN], 8, 200, 13),
    "P4": ([[SE, PER], WN], 3, 130, 14),
    "P5": ([SE, WN], 21, 129, 15),
}


def diagonal(desc, hp, d, eps=R.EPS):
    """K's constant diagonal in the GPR_SELF form, in cg_diagonal's order of operations"""
    dg = None
    for t in R.split_hp(desc, hp, d):
        if t[0][0] == WN and dg is None:
            dg = float(t[0][1][0]) * float(t[0][1][0])
    dg = 0.0 if dg is None else dg
    for t in R.split_hp(desc, hp, d):
        if t[0][0] == WN:
            continue
        term = 1.0
        for _, h in t:
            term *= float(h[0]) * float(h[0])
        dg += term + eps
    return dg


def cg(K, B, diag, tol, maxit):
    """(X, iters, col_iters): the recurrence above on the n x nrhs columns of B; col_iters[c] is the
    iteration after which column c froze (0: at once; maxit + 1: never)"""
    # (column-major, so that a column is the same contiguous vector whatever nrhs is)
    B = np.asfortranarray(np.asarray(B, dtype=np.float64).reshape(K.shape[0], -1))
    dinv, tol2 = 1.0 / diag, tol * tol
    X = np.zeros_like(B)
    Rr, P = B.copy(order="F"), np.asfortranarray(B * dinv)
    bb = np.einsum("ic,ic->c", B, B)
    rho = bb.copy()
    frozen = bb <= tol2 * bb
    col_iters = np.where(frozen, 0, maxit + 1)
    it = 0
    while not frozen.all() and it < maxit:
        for c in np.flatnonzero(~frozen):
            q = K @ P[:, c]  # (column by column: a column's arithmetic does not depend on nrhs)
            alpha = (rho[c] * dinv) / (P[:, c] @ q)
            X[:, c] += alpha * P[:, c]
            Rr[:, c] -= alpha * q
            num = Rr[:, c] @ Rr[:, c]
            P[:, c] = Rr[:, c] * dinv + (num / rho[c]) * P[:, c]
            rho[c] = num
            if num <= tol2 * bb[c]:
                frozen[c] = True
                col_iters[c] = it + 1
        it += 1
    return X, it, col_iters


def textbook_count(cond, tol):
    return 0.5 * math.sqrt(cond) * math.log(2.0 * math.sqrt(cond) / tol)


def rhs(name, nrhs):
    """the seeded right-hand side of a problem: sin^2 of the coordinate sum, then standard normals"""
    _, _, x = inputs(name)
    n = x.shape[1]
    cols = [np.sin(np.sum(x, axis=0)) ** 2]
    cols += [np.random.default_rng(1000 + c).standard_normal(n) for c in range(1, nrhs)]
    return np.column_stack(cols)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(desc, hp, x), never written"""
    desc, d, n, seed = PROBLEMS[name]
    rng = np.random.default_rng(seed)
    hp = rng.uniform(0.3, 2.0, sum(R.width(k, d) for k in R.flat(desc)))
    hp[-1] = rng.uniform(0.3, 1.0)
    x = rng.random((d, n))
    hp.setflags(write=False)
    return desc, hp, x


@functools.lru_cache(maxsize=None)
def reference(name):
    """(K, cond_2, diag, maxit): the float64 reference matrix (read-only), its condition number, the
    Jacobi factor's diagonal and the GPU tests' iteration cap"""
    desc, hp, x = inputs(name)
    K = R.kernel_ld(desc, hp, x).astype(np.float64)
    K.setflags(write=False)
    ev = np.linalg.eigvalsh(K)
    assert ev[0] > 0.0
    cond = float(ev[-1] / ev[0])
    return K, cond, diagonal(desc, hp, x.shape[0]), int(math.ceil(MARGIN * textbook_count(cond, TOL)))


def assert_problem(name):
    """the preconditions of a problem; returns (cond_2, allowed count, the recurrence's count)"""
    desc, hp, x = inputs(name)
    K, cond, diag, maxit = reference(name)
    d, n = x.shape
    assert np.all((x >= 0.0) & (x < 1.0)) and np.all((hp >= 0.3) & (hp <= 2.0)) and hp[-1] <= 1.0
    assert np.allclose(np.diag(K), diag, rtol=1e-14, atol=0.0), "cg_diagonal restated wrongly"
    allowed = textbook_count(cond, TOL)
    B = rhs(name, 3)
    X, iters, _ = cg(K, B, diag, TOL, int(math.ceil(allowed)))
    assert iters < allowed, f"{name}: {iters} iterations, the bound allows {allowed:.1f}"
    res = np.linalg.norm(B - K @ X, axis=0) / np.linalg.norm(B, axis=0)
    assert np.all(res <= 10 * TOL), res
    assert maxit >= iters
    return cond, allowed, iters


@functools.lru_cache(maxsize=None)
def fast_and_slow():
    """(b_fast, b_slow) on P1: the sum of the two leading eigenvectors of the reference K (a Krylov
    space of dimension two: two iterations in exact arithmetic) and a seeded standard-normal vector"""
    K = reference("P1")[0]
    _, vec = np.linalg.eigh(K)
    b_fast = vec[:, -1] + vec[:, -2]
    b_slow = np.random.default_rng(77).standard_normal(K.shape[0])
    for b in (b_fast, b_slow):
        b.setflags(write=False)
    return b_fast, b_slow


FAST_SLOW_TOL = 1e-8


def assert_fast_and_slow():
    """at most 4 iterations for b_fast, at least 20 for b_slow at tol = 1e-8; returns the counts"""
    K, _, diag, _ = reference("P1")
    b_fast, b_slow = fast_and_slow()
    _, _, ci = cg(K, np.column_stack([b_fast, b_slow]), diag, FAST_SLOW_TOL, K.shape[0])
    assert ci[0] <= 4 and ci[1] >= 20, ci
    return int(ci[0]), int(ci[1])
