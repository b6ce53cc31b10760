"""GPU: the matrix-free gradient of the negative log marginal likelihood (gpr_mll_grad_free).

Exact probes.  With Z = sqrt(n) I and m = n, (1/m) Z Z' = I and Hutchinson's estimator is the
trace itself, so the call must reproduce the dense gradient -0.5 sum (alpha alpha' - K^-1) o dK_j up
to its solves and the form's rounding (this also takes r = n + 1 through the whole stack):
    |g_j - ref_j| <= 4 kappa max(relres) sum_ab (|alpha| |alpha|' + |K^-1|)_ab |dK_j,ab|
                     + the form's bound of test_gpu_grad_form.py, whose |M| is that same matrix,
kappa = cond_2(K): CG's normwise error kappa relres in each of [alpha | K^-1 Z], carried through the
form, which is bilinear in them.  The reference is the oracle's mll_grad where the oracle has the
kernel (SE + WN); with a Matern part it is the same formula on kernel_ref_ld's K and dK.
"""
import numpy as np
import pytest

import kernel_ref_ld as R
import test_gpu_grad_form as GF
import test_product_cpu as PR
from kernel_ref_ld import LD, M52, SE, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")
from oracle import gpr_oracle as O  # noqa: E402

D = 8


def _model(desc, n, seed):
    rng = np.random.default_rng(seed)
    hp = rng.uniform(0.3, 2.0, sum(R.width(k, D) for k in R.flat(desc)))
    hp[-1] = rng.uniform(0.3, 1.0)  # sigma_n >= 0.3: cond_2(K) stays in the thousands
    x = rng.random((D, n))
    y = np.sin(np.sum(x, axis=0)) ** 2
    return hp, x, y, G.GPRModel(PR.cov_of(desc), hp, x, y)


@pytest.mark.parametrize("n", [96, 130])
@pytest.mark.parametrize("desc", [[SE, WN], [SE, M52, WN]], ids=["SE+WN", "SE+M52+WN"])
def test_exact_probes_reproduce_the_dense_gradient(desc, n):
    hp, x, y, md = _model(desc, n, n + len(desc))
    g, iters, relres = G.mll_grad_free(md, Z=np.sqrt(n) * np.eye(n), tol=1e-12, maxit=20 * n)
    K = R.kernel_ld(desc, hp, x).astype(np.float64) if M52 in desc else O.kernel(desc, hp, x)
    Kinv = np.linalg.inv(K).astype(LD)
    a = Kinv @ y.astype(LD)
    ref, T, S = GF.form_ref(desc, hp, x, np.outer(a, a) - Kinv,
                            np.outer(np.abs(a), np.abs(a)) + np.abs(Kinv))
    ref = -0.5 * ref if M52 in desc else O.mll_grad(desc, hp, x, y)
    kappa = np.linalg.cond(K, 2)
    bound = 4 * kappa * relres.max() * S + (1e-13 + (n + (n + 1) + 2 * D + 16) * R.U) * T
    err = np.abs(g.astype(LD) - ref)
    print(f"iters {iters}, max relres {relres.max():.3g}, cond {kappa:.1f}, "
          f"max |err| / bound = {float(np.max(err / bound)):.3g}")
    assert relres.shape == (n + 1,)
    assert np.all(err <= bound)


def test_seed_reproduces_and_matters():
    hp, x, y, md = _model([SE, WN], 130, 3)
    a = G.mll_grad_free(md, seed=11)[0]
    b = G.mll_grad_free(md, seed=11)[0]
    c = G.mll_grad_free(md, seed=12)[0]
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    assert not np.array_equal(a, c)
