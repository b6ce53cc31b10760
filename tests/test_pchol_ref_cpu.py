"""CPU: the preconditions of tests/test_gpu_pchol.py.  For every (problem, rank) each step of the NumPy
factorisation keeps a gap of >= 1e-9 c between the two largest residual diagonals and long double
picks the same pivots, so comparing the device's pivots is meaningful.
"""
import numpy as np
import pytest

import pchol_ref as PC


@pytest.mark.parametrize("name", sorted(PC.PROBLEMS))
def test_pivot_gaps(name):
    Kc, _, K, c, delta = PC.reference(name)
    assert np.allclose(np.diag(Kc), c, rtol=1e-14, atol=0.0)
    assert np.allclose(K - Kc, delta * np.eye(K.shape[0]), rtol=0.0, atol=1e-15 * c)
    for rank in PC.RANKS:
        L, piv, gap, err = PC.factor(name, rank)  # (asserts the long-double pivots are the same)
        assert len(piv) == rank == len(set(piv.tolist())) and gap >= 1e-9, (rank, gap)
        assert np.max(np.abs((Kc - L @ L.T)[piv])) <= 1e-10 * c
