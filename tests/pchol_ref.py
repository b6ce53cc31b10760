"""csrc/pchol.hip's factorisation and csrc/cg.hip's preconditioned recurrence restated in NumPy on a
dense matrix, and the problems of tests/test_gpu_pchol.py (x in the unit cube, hp in [0.3, 2],
sigma_n = 0.05, seeds fixed).  A helper module: nothing here is collected as a test.
Kc is kernel_ref_ld's cross-form kernel of x with itself (no eps, no noise), K the GPR_SELF matrix,
delta = sigma_n^2 + eps per term, so that K = Kc + delta I.
"""
import functools

import numpy as np

import kernel_ref_ld as R
from kernel_ref_ld import M52, PER, SE, WN

SIGMA_N = 0.05
TOL = 1e-10
RANKS = (1, 5, 17, 64)

PROBLEMS = {
    "a": ([SE, WN], 3, 130, 1),
    "b": ([SE, M52, WN], 8, 1100, 2),
    "c": ([[SE, PER], WN], 3, 130, 3),
    "d": ([SE, SE, SE, SE, SE, WN], 8, 200, 4),
    "e": ([SE, WN], 21, 129, 5),
}


def pchol(Kc, rank, rtol=0.0):
    """(L, piv, gap) in Kc's dtype.  Step m: pivot i = the first largest residual diagonal d_i; stop
    with rank m when d_i <= rtol n c; L[:, m] = (Kc[:, i] - L[:, :m] L[i, :m]) / sqrt(d_i); d -=
    L[:, m]^2 clamped at 0, a chosen pivot marked -1.  gap: the least difference between the largest
    and the second-largest residual diagonal over the steps, in units of c."""
    n, c = Kc.shape[0], Kc[0, 0]
    one = Kc.dtype.type
    L = np.zeros((n, rank), dtype=Kc.dtype)
    dres = np.full(n, c, dtype=Kc.dtype)
    piv, gap = [], np.inf
    for m in range(rank):
        i = int(np.argmax(dres))  # (the first of equal maxima)
        di = dres[i]
        if not di > one(rtol) * one(n) * c:
            break
        if m > 0:  # (step 0: every diagonal is c, the first point wins the tie)
            gap = min(gap, float((di - np.max(np.delete(dres, i))) / c))
        col = (Kc[:, i] - L[:, :m] @ L[i, :m]) / np.sqrt(di)
        L[:, m] = col
        new = np.maximum(dres - col * col, one(0))
        new[dres < 0] = one(-1)
        new[i] = one(-1)
        dres = new
        piv.append(i)
    return L[:, :len(piv)], np.array(piv, dtype=np.int64), gap


def pcg(K, B, L, delta, tol, maxit):
    """(X, iters, col_iters): z = (r - L C^-1 L'r) / delta, C = delta I + L'L; rho = r.z, alpha = rho /
    p.q, x += alpha p, r -= alpha q, beta = rho_new / rho, p = z + beta p; a column freezes at r.r <=
    tol^2 b.b, col_iters[c] the iteration after which it did (independent of nrhs)"""
    B = np.asarray(B, dtype=np.float64).reshape(K.shape[0], -1)
    C = delta * np.eye(L.shape[1]) + L.T @ L
    prec = lambda r: (r - L @ np.linalg.solve(C, L.T @ r)) / delta  # noqa: E731
    X, it = np.zeros_like(B), 0
    Rr, Z = B.copy(), prec(B)
    P, rho = Z.copy(), np.einsum("ic,ic->c", B, Z)
    bb = np.einsum("ic,ic->c", B, B)
    frozen = bb <= tol * tol * bb
    col_iters = np.where(frozen, 0, maxit + 1)
    while not frozen.all() and it < maxit:
        for c in np.flatnonzero(~frozen):
            q = K @ P[:, c]
            alpha = rho[c] / (P[:, c] @ q)
            X[:, c] += alpha * P[:, c]
            Rr[:, c] -= alpha * q
            z = prec(Rr[:, c])
            new = Rr[:, c] @ z
            P[:, c] = z + (new / rho[c]) * P[:, c]
            rho[c] = new
            if Rr[:, c] @ Rr[:, c] <= tol * tol * bb[c]:
                frozen[c], col_iters[c] = True, it + 1
        it += 1
    return X, it, col_iters


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(desc, hp, x), never written"""
    desc, d, n, seed = PROBLEMS[name]
    rng = np.random.default_rng(seed)
    hp = rng.uniform(0.3, 2.0, sum(R.width(k, d) for k in R.flat(desc)))
    hp[-1] = SIGMA_N
    x = rng.random((d, n))
    hp.setflags(write=False)
    x.setflags(write=False)
    return desc, hp, x


@functools.lru_cache(maxsize=None)
def reference(name):
    """(Kc float64, Kc long double, K float64, c, delta), read-only"""
    desc, hp, x = inputs(name)
    Kld = R.kernel_ld(desc, hp, x, xp=x, same=R.CROSS)
    nterms = sum(1 for t in R.split_hp(desc, hp, x.shape[0]) if t[0][0] != WN)
    c, delta = float(Kld[0, 0]), SIGMA_N ** 2 + R.EPS * nterms
    K = R.kernel_ld(desc, hp, x).astype(np.float64)
    Kc = Kld.astype(np.float64)
    for a in (Kc, Kld, K):
        a.setflags(write=False)
    return Kc, Kld, K, c, delta


@functools.lru_cache(maxsize=None)
def factor(name, rank):
    """(L, piv, gap / c, max |L - L_longdouble| / sqrt(c)) of the float64 restatement"""
    Kc, Kld, _, c, _ = reference(name)
    L, piv, gap = pchol(Kc, rank)
    Ll, pivl, _ = pchol(Kld, rank)
    assert np.array_equal(piv, pivl)
    L.setflags(write=False)
    return L, piv, gap, float(np.max(np.abs(L - Ll))) / np.sqrt(c)


def rhs(name, nrhs):
    """sin^2 of the coordinate sum, then seeded standard normals"""
    x = inputs(name)[2]
    cols = [np.sin(np.sum(x, axis=0)) ** 2]
    cols += [np.random.default_rng(1000 + c).standard_normal(x.shape[1]) for c in range(1, nrhs)]
    return np.column_stack(cols)
