"""CPU: the NumPy restatement of cg.hip's recurrence (tests/cg_ref.py) and the preconditions of the
problem families the GPU tests of the matrix-free solve use -- an ill-posed family fails here,
without a GPU.
"""
import numpy as np
import pytest

import cg_ref as C


@pytest.mark.parametrize("name", list(C.PROBLEMS))
def test_problem_preconditions(name):
    cond, allowed, iters = C.assert_problem(name)
    print(f"{name}: cond_2 {cond:.1f}, the bound allows {allowed:.1f} iterations, the recurrence "
          f"takes {iters}; maxit {C.reference(name)[3]}")


def test_fast_and_slow_right_hand_sides():
    fast, slow = C.assert_fast_and_slow()
    print(f"P1 at tol {C.FAST_SLOW_TOL}: b_fast {fast} iterations, b_slow {slow}")


def test_recurrence_solves_and_freezes():
    """Against numpy.linalg.solve on P3; a joint solve's columns are the solo solves' (a column
    reads no other column), a zero column is frozen at once at x = 0, maxit = 0 leaves x = 0."""
    K, cond, diag, maxit = C.reference("P3")
    B = C.rhs("P3", 3)
    B[:, 1] = 0.0
    X, iters, ci = C.cg(K, B, diag, C.TOL, maxit)
    assert ci[1] == 0 and np.all(X[:, 1] == 0.0) and iters == max(ci) < maxit
    for c in (0, 2):
        xs = np.linalg.solve(K, B[:, c])
        res = np.linalg.norm(B[:, c] - K @ X[:, c]) / np.linalg.norm(B[:, c])
        assert res <= 10 * C.TOL
        assert np.linalg.norm(X[:, c] - xs) <= cond * res * np.linalg.norm(xs)
        solo, it1, ci1 = C.cg(K, B[:, c], diag, C.TOL, maxit)
        assert np.array_equal(solo[:, 0], X[:, c]) and it1 == ci1[0] == ci[c]
    X0, it0, _ = C.cg(K, B, diag, C.TOL, 0)
    assert it0 == 0 and np.all(X0 == 0.0)


def test_diagonal_follows_the_description():
    from kernel_ref_ld import PER, SE, WN
    hp = np.array([2.0, 1.0, 3.0, 1.0, 0.9, 0.5, 0.125])  # SE * PER + WN + WN at d = 1
    got = C.diagonal([[SE, PER], WN, WN], hp, 1, eps=1e-8)
    assert got == 0.25 + (4.0 * 9.0 + 1e-8)  # the first WhiteNoise only, eps once per term
