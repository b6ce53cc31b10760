"""CPU: the rank-r update behind gpr_fit_remove restated in NumPy, and the case tables that
tests/test_gpu_remove.py runs on the device.

A fitted buffer holds U above the diagonal (K = U^T U) and K strictly below.  With D the removed
indices, keep the others in ascending order,

    T = U[keep, keep]        (upper triangular, positive diagonal)
    W = U[D, keep]           (W[s, j'] = 0 wherever keep[j'] < p_s: the buffer holds K there)
    K[keep, keep] = T^T T + W^T W

so the factor of the kept points is T after a rank-r positive update by Givens rotations: for each
row i' in ascending order and each s in ascending order rho = hypot(T[i',i'], W[s,i']),
c = T[i',i'] / rho, sg = W[s,i'] / rho, and every pair (T[i',j'], W[s,j']), j' >= i', becomes
(c t + sg w, -sg t + c w).  The library takes the removed points GROUP at a time (one pass over T
per group, the later groups' W rows from the untouched buffer): that grouped evaluation is
restated too and held to the same tolerances.

The reference is always the full fit of the kept points (O.chol_upper / O.cho_solve_upper on
K[keep, keep]).  Inputs, targets and tolerances are tests/test_append_cpu.py's: SE + WhiteNoise,
sigma_n = 0.1, d = 2, y = cos(sum_k x_k), the project's gpr_fit tolerances.  Measured here: U' within
0.04 and alpha' within 0.31 of those tolerances over the table (each case prints its own figures).
"""
import numpy as np
import pytest

import test_append_cpu as A
from oracle import gpr_oracle as O
from test_append_cpu import TOL_U

GROUP = 8  # removed points per pass of the library's update (RM_R of csrc/remove.hip)
KINDS, D_IN = A.SHAPE_KINDS, A.SHAPE_D


def _scattered(n0, r, seed):
    return sorted(int(v) for v in np.random.default_rng(seed).choice(n0, size=r, replace=False))


# ---- the case tables (shared with the GPU file) -----------------------------------------------
# (n0, removed indices): the oldest / the newest point (a pure copy), points at and around the
# edges of the 128-column blocks, a ragged last block, a full group, one more than two groups,
# many groups, all but one point, one block more than 16
GPU_SHAPES = [
    (100, [0]), (128, [127]), (129, [128]), (129, [0]), (257, [127, 128]),
    (300, [5, 127, 128, 129, 299]), (513, [256]), (1037, [0, 500, 1036]), (1000, list(range(16))),
    (640, list(range(100, 117))), (700, _scattered(700, 130, 41)), (5, [0, 1, 2, 3]), (2081, [0]),
]
SHAPES = GPU_SHAPES + [(300, [0, 1, 2])]
NRHS_CASE = dict(n0=300, idx=[7, 128, 200], ny=2, ldy_pad=5)
CHAIN = dict(n0=400, steps=[[0], _scattered(399, 5, 42), [393], _scattered(393, 130, 43)])
SLIDE = dict(window=256, rounds_cpu=44, rounds_gpu=12)
LONG_CHAIN = dict(n0=8320, idx=[0, 4000])


def shape_id(case):
    n0, idx = case
    return f"{n0}-{len(idx)}@{idx[0]}"


def keep_of(n0, idx):
    return np.setdiff1d(np.arange(n0), np.asarray(idx))


def fitted_buffer(K, U):
    """what gpr_fit leaves: U above the diagonal, K strictly below"""
    return np.triu(U) + np.tril(K, -1)


# ---- the restatement ----------------------------------------------------------------------------
def givens_remove(buf, idx, group=None):
    """U' (upper) of the kept points from the fitted buffer; group: removed points per pass (None:
    all of them in one pass)"""
    n0 = buf.shape[0]
    idx = np.asarray(idx)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n0
    keep = keep_of(n0, idx)
    T = np.triu(buf[np.ix_(keep, keep)])
    W = np.where(keep[None, :] > idx[:, None], buf[np.ix_(idx, keep)], 0.0)
    r, n = len(idx), len(keep)
    group = group or r
    for s0 in range(0, r, group):
        for i in range(n):
            for s in range(s0, min(r, s0 + group)):
                w = W[s, i]
                if w == 0.0:      # c = 1, sg = 0: the pair is reproduced exactly
                    continue
                t = T[i, i]
                rho = np.hypot(t, w)
                c, sg = t / rho, w / rho
                ti = T[i, i:].copy()
                T[i, i:] = c * ti + sg * W[s, i:]
                W[s, i:] = -sg * ti + c * W[s, i:]
    return T


def remove_fit(buf, idx, y_kept, group=None):
    Un = givens_remove(buf, idx, group)
    return Un, O.cho_solve_upper(Un, y_kept)


def kept_fit(K, y, keep):
    Kk = K[np.ix_(keep, keep)]
    Uk = A.assert_well_conditioned(Kk) if len(keep) > 1 else O.chol_upper(Kk)
    return Kk, Uk, O.cho_solve_upper(Uk, y[keep])


def tol_fraction(got, want):
    return float(np.max(np.abs(got - want) / (TOL_U["atol"] + TOL_U["rtol"] * np.abs(want))))


def check_against_kept_fit(n0, idx, ny=1, group=None):
    x, y, hp, K, U, alpha = A.make_case(KINDS, n0, 0, D_IN, ny)
    keep = keep_of(n0, idx)
    Kk, Uk, ak = kept_fit(K, y, keep)
    Un, an = remove_fit(fitted_buffer(K, U), idx, y[keep], group)
    print(f"  ({n0}, r={len(idx)}, group={group}): U {tol_fraction(np.triu(Un), np.triu(Uk)):.3f} "
          f"alpha {tol_fraction(an, ak):.3f} of the tolerance")
    assert np.all(np.diag(Un) > 0.0) and np.all(np.tril(Un, -1) == 0.0)
    np.testing.assert_allclose(Un, np.triu(Uk), **TOL_U)
    np.testing.assert_allclose(an, ak, **TOL_U)
    return Un, an


@pytest.mark.parametrize("case", SHAPES, ids=shape_id)
def test_shapes(case):
    check_against_kept_fit(*case)


@pytest.mark.parametrize("case", [c for c in SHAPES if len(c[1]) > GROUP], ids=shape_id)
def test_grouped_evaluation(case):
    """groups of GROUP removed points, each a pass of its own, against the kept fit and against the
    single pass"""
    n0, idx = case
    Ug, ag = check_against_kept_fit(n0, idx, group=GROUP)
    U1, a1 = check_against_kept_fit(n0, idx)
    np.testing.assert_allclose(Ug, U1, **TOL_U)
    np.testing.assert_allclose(ag, a1, **TOL_U)


def test_rows_above_the_first_removed_point_are_reproduced_exactly():
    n0, idx = 300, [140, 141, 290]
    x, y, hp, K, U, alpha = A.make_case(KINDS, n0, 0, D_IN)
    Un = givens_remove(fitted_buffer(K, U), idx)
    keep = keep_of(n0, idx)
    assert np.array_equal(Un[:140], np.triu(U)[np.ix_(keep, keep)][:140])
    # and removing only the newest points is a pure copy
    Un = givens_remove(fitted_buffer(K, U), [298, 299])
    assert np.array_equal(Un, np.triu(U)[:298, :298])


def test_the_mask_matters():
    """the buffer holds K, not zero, below the diagonal: W loaded without the mask gives another
    matrix"""
    n0, idx = 129, [64]
    x, y, hp, K, U, alpha = A.make_case(KINDS, n0, 0, D_IN)
    buf = fitted_buffer(K, U)
    keep = keep_of(n0, idx)
    assert np.all(np.abs(buf[64, :64]) > 0.0)
    Un = givens_remove(buf, idx)
    np.testing.assert_allclose(Un.T @ Un, K[np.ix_(keep, keep)], rtol=1e-12, atol=1e-14)


def test_two_columns_of_y():
    c = NRHS_CASE
    Un, an = check_against_kept_fit(c["n0"], c["idx"], ny=c["ny"])
    assert an.shape == (c["n0"] - len(c["idx"]), 2)


def test_chained_removals():
    """400 -> -1 -> -5 -> -1 -> -130, each step from the previous step's buffer"""
    n = CHAIN["n0"]
    x, y, hp, K, U, alpha = A.make_case(KINDS, n, 0, D_IN)
    buf, alive = fitted_buffer(K, U), np.arange(n)
    for idx in CHAIN["steps"]:
        Un = givens_remove(buf, idx, GROUP)
        alive = alive[keep_of(len(alive), idx)]
        Kk, Uk, ak = kept_fit(K, y, alive)
        np.testing.assert_allclose(Un, np.triu(Uk), **TOL_U)
        np.testing.assert_allclose(O.cho_solve_upper(Un, y[alive]), ak, **TOL_U)
        buf = fitted_buffer(Kk, Un)
    assert len(alive) == 400 - 137


def test_sliding_window():
    """a window of 256: remove the oldest point, append the next by the block formulas, 44 rounds;
    the factor and alpha against the full fit of the final window"""
    w, rounds = SLIDE["window"], SLIDE["rounds_cpu"]
    x, y, hp, K, U, alpha = A.make_case(KINDS, w, rounds, D_IN)
    lo = 0
    Uc, ac = A.old_fit(KINDS, hp, x, y, w)
    for _ in range(rounds):
        Kw = K[lo:lo + w, lo:lo + w]
        Un, an = remove_fit(fitted_buffer(Kw, Uc), [0], y[lo + 1:lo + w])
        lo += 1
        info, Uc, ac, _ = A.block_append(KINDS, hp, x[:, lo:lo + w], y[lo:lo + w], w - 1, Un, an)
        assert info == 0
    Kk, Uk, ak = kept_fit(K, y, np.arange(lo, lo + w))
    np.testing.assert_allclose(np.triu(Uc), np.triu(Uk), **TOL_U)
    np.testing.assert_allclose(ac, ak, **TOL_U)


def test_header_and_binding():
    import gpr_amd as G
    from gpr_amd import _lib as L
    assert "gpr_fit_remove" in L.header_exports()
    assert "gpr_fit_remove" in L._SIGS and hasattr(L.lib, "gpr_fit_remove")
    assert len(L._SIGS["gpr_fit_remove"][1]) == 12
    assert hasattr(G, "remove_") and "remove_" in G.__all__
