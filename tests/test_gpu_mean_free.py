"""GPU: the posterior mean by the matrix-free route (GPR_MEAN_FREE = 1) and predict_mean_from,
against the posterior mean mu = K(xp, x) K^{-1} y of the CPU oracle (SquaredExp + WhiteNoise)
or, for a description the oracle and the split path do not have, of the same formula on the
long-double reference kernel.  Tolerance: the parity tests' for mu (rtol 1e-8, atol 1e-10).
"""
import numpy as np
import pytest

import kernel_ref_ld as R
import test_product_cpu as PR
from kernel_ref_ld import M52, PER, SE, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")
from oracle import gpr_oracle as O  # noqa: E402

TOL = dict(rtol=1e-8, atol=1e-10)
DESCS = {"SE+WN": [SE, WN], "M52+PER+WN": [M52, PER, WN]}


def _model(name, n, m, d=3):
    x, y, xp = O.synthetic(d, n, m)
    desc = DESCS[name]
    rng = np.random.default_rng(n + m)
    hp = rng.uniform(0.5, 1.5, sum(R.width(k, d) for k in R.flat(desc)))
    hp[-1] = 0.3  # sigma_n
    return desc, hp, x, y, xp, G.GPRModel(PR.cov_of(desc), hp, x, y)


def _mean_ref(desc, hp, x, y, xp):
    if desc == [SE, WN]:
        return O.predict([O.SE, O.WN], hp, x, y, xp, diagonal_var=True)[0]
    K = R.kernel_ld(desc, hp, x).astype(np.float64)
    Kpx = R.kernel_ld(desc, hp, xp, x).astype(np.float64)
    return Kpx @ np.linalg.solve(K, y)


@pytest.mark.parametrize("name", list(DESCS))
@pytest.mark.parametrize("n,m", [(300, 257), (129, 1)])
def test_mean_free_route_matches_the_oracle(knobs, name, n, m):
    desc, hp, x, y, xp, md = _model(name, n, m)
    knobs("GPR_MEAN_FREE", 1)
    np.testing.assert_allclose(G.predict_mean(md, xp), _mean_ref(desc, hp, x, y, xp), **TOL)


def test_same_object_rule(knobs):
    """xp is md.x: eps on the diagonal of K(xp, x), no noise -- as the dense route"""
    desc, hp, x, y, _, md = _model("SE+WN", 200, 1)
    knobs("GPR_MEAN_FREE", 0)
    dense = G.predict_mean(md, md.x)
    knobs("GPR_MEAN_FREE", 1)
    free = G.predict_mean(md, md.x)
    np.testing.assert_allclose(free, dense, **TOL)
    K5 = R.kernel_ld(desc, hp, x, x).astype(np.float64)
    alpha = np.linalg.solve(R.kernel_ld(desc, hp, x).astype(np.float64), y)
    np.testing.assert_allclose(free, K5 @ alpha, **TOL)


def test_predict_mean_from_several_columns():
    """an N x 3 alpha: mu = K(xp, x) alpha column by column, against the long-double kernel"""
    desc, hp, x, y, xp, md = _model("M52+PER+WN", 300, 257)
    alpha = np.random.default_rng(3).standard_normal((300, 3))
    mu = G.predict_mean_from(md, alpha, xp)
    assert mu.shape == (257, 3)
    np.testing.assert_allclose(mu, R.kernel_ld(desc, hp, xp, x).astype(np.float64) @ alpha, **TOL)


def test_predict_mean_from_given_weights(knobs):
    desc, hp, x, y, xp, md = _model("M52+PER+WN", 300, 257)
    knobs("GPR_MEAN_FREE", 0)
    dense = G.predict_mean(md, xp)
    pc = G.predict_cache(md, xp)(md, 0)
    G.update_predict_cache_(pc, md)
    alpha = md.ctx.host(pc.wt)
    np.testing.assert_allclose(G.predict_mean_from(md, alpha, xp), dense, **TOL)
