"""GPU: the symmetric matrix-free product (GPR_KMM_SYM; ``symmetric=True``), which evaluates only
the tiles I <= J of K(x, x) and uses each off-diagonal tile twice.

The product is held to test_gpu_kernel_matmul.py's componentwise bound against the long-double
kernel (it holds for any summation order); with identity columns the route returns K(x, x), each
element bit for bit the Gram route's (an element is symmetric in its two points and the in-register
transposition is exact); CG and the free gradient are held to their own files' acceptance.
"""
import numpy as np
import pytest
import torch

import kernel_ref_ld as R
import test_gpu_grad_form as GF
import test_product_cpu as PR
from kernel_ref_ld import LD, M52, PER, SAME_OBJECT, SE, SELF, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")
from oracle import gpr_oracle as O  # noqa: E402

DESCS = {"SE": [SE], "SE+M52+WN": [SE, M52, WN], "PER": [PER], "SE*PER+WN": [[SE, PER], WN],
         "5SE+WN": [SE, SE, SE, SE, SE, WN]}

# (description, d, n, nv, same, GPR_KMM_SLABS, (ldv - n, ldo - n)).  Bands are 4 blocks of 64 points
# for a sum of SE parts at d <= 8, 2 for the other descriptions there, 1 above d = 8.
CASES = [
    ("SE", 1, 1, 1, SELF, 0, (0, 0)),                 # a single point
    ("SE", 8, 64, 16, SELF, 0, (0, 0)),               # one diagonal tile only
    ("SE", 8, 65, 15, SAME_OBJECT, 0, (0, 0)),        # the first off-diagonal pair, ragged
    ("SE", 8, 128, 16, SELF, 0, (0, 0)),              # ... and full: the transposed layout
    ("SE", 1, 200, 1, SELF, 0, (0, 0)),               # 4 blocks, one band, ragged
    ("SE", 8, 300, 16, SELF, 0, (0, 0)),              # 5 blocks, a second band shorter than G
    ("SE", 8, 600, 15, SELF, 3, (0, 0)),              # 3 bands, each walk in 3 slabs
    ("SE", 21, 128, 16, SAME_OBJECT, 0, (0, 0)),      # k-steps at run time: bands of one block
    ("SE", 21, 300, 1, SELF, 2, (0, 0)),
    ("SE+M52+WN", 8, 128, 15, SELF, 0, (0, 0)),
    ("SE+M52+WN", 1, 300, 16, SAME_OBJECT, 2, (0, 0)),
    ("SE+M52+WN", 21, 200, 1, SELF, 0, (0, 0)),
    ("PER", 1, 65, 16, SELF, 0, (0, 0)),
    ("PER", 8, 300, 1, SAME_OBJECT, 0, (0, 0)),
    ("SE*PER+WN", 8, 200, 15, SELF, 3, (0, 0)),
    ("SE*PER+WN", 21, 130, 16, SAME_OBJECT, 0, (0, 0)),
    ("5SE+WN", 8, 300, 16, SELF, 0, (0, 0)),          # two part groups, the noise on the last
    ("5SE+WN", 1, 128, 1, SAME_OBJECT, 0, (0, 0)),
    ("SE+M52+WN", 8, 200, 65, SELF, 0, (0, 0)),       # a 64-column full pass, a 1-column symmetric
    ("SE", 8, 300, 16, SELF, 0, (7, 5)),
    ("SE*PER+WN", 8, 130, 15, SAME_OBJECT, 0, (6, 3)),
]


def _inputs(name, d, n, nv, seed):
    rng = np.random.default_rng(seed)
    desc = DESCS[name]
    hp = rng.uniform(0.3, 2.0, sum(R.width(k, d) for k in R.flat(desc)))
    return desc, hp, rng.random((d, n)), rng.standard_normal((n, nv))


def _run(desc, hp, x, V, same, pad=(0, 0), symmetric=True):
    """kernel_matmul on device buffers with padded leading dimensions: NaN in V's padding rows, a
    sentinel in Out's"""
    ctx = G.default_context()
    n, nv = V.shape
    dV = torch.full((nv, n + pad[0]), float("nan"), dtype=torch.float64, device=ctx.device)
    dV[:, :n] = torch.from_numpy(np.ascontiguousarray(V.T)).to(ctx.device)
    out = torch.full((nv, n + pad[1]), -7.5, dtype=torch.float64, device=ctx.device)
    torch.cuda.synchronize()
    G.kernel_matmul(PR.cov_of(desc), hp, x, dV, None if same == SELF else x, out=out,
                    symmetric=symmetric)
    ctx.sync()
    o = out.cpu().numpy()
    assert np.all(o[:, n:] == -7.5), "Out's padding was written"
    assert ctx.get_knob("GPR_KMM_SYM") == 0
    return o[:, :n].T.copy()


@pytest.mark.parametrize("name,d,n,nv,same,slabs,pad", CASES)
def test_product_against_long_double(knobs, name, d, n, nv, same, slabs, pad):
    knobs("GPR_KMM_SLABS", slabs)
    desc, hp, x, V = _inputs(name, d, n, nv, 1000 * n + nv + d)
    out = _run(desc, hp, x, V, same, pad)
    K = R.kernel_ld(desc, hp, x, None, same=same)
    ref = K @ V.astype(LD)
    bound = (1e-13 + (n + 8) * R.U) * (np.abs(K) @ np.abs(V).astype(LD))
    err = np.abs(out.astype(LD) - ref)
    print(f"max |err| / bound = {float(np.max(err / bound)):.3g}")
    assert np.all(np.isfinite(out))
    assert np.all(err <= bound)


def test_band_chunks_reuse_the_workspace():
    """n = 16449: 258 blocks are 65 bands of 4, one more than a launch takes, so the second launch
    writes its partials over the first's.  Too large for the long-double kernel: with V >= 0 and the
    SE kernel's K > 0, sum_j |K_ij| |V_j| is the product itself, and the two routes, each inside the
    bound above, differ by at most twice it."""
    n, nv = 16449, 2
    desc, hp, x, V = _inputs("SE", 1, n, nv, 9)
    V = np.abs(V)
    sym, par = _run(desc, hp, x, V, SELF), _run(desc, hp, x, V, SELF, symmetric=False)
    bound = 2 * (1e-13 + (n + 8) * R.U) * par * (1 + 1e-12)
    print(f"max |sym - par| / bound = {float(np.max(np.abs(sym - par) / bound)):.3g}")
    assert np.all(par > 0) and np.all(np.abs(sym - par) <= bound)


@pytest.mark.parametrize("name", ["SE+M52+WN", "SE*PER+WN"])
def test_identity_columns_return_the_gram_route_s_elements(name):
    n = 200
    desc, hp, x, _ = _inputs(name, 8, n, 1, 77)
    K = G.kernel(PR.cov_of(desc), hp, x)
    eye = np.eye(n)
    out = np.hstack([_run(desc, hp, x, eye[:, c:c + 16], SELF) for c in range(0, n, 16)])
    assert np.array_equal(out, K)


def test_two_calls_agree_bit_for_bit():
    desc, hp, x, V = _inputs("SE*PER+WN", 8, 300, 16, 5)
    assert np.array_equal(_run(desc, hp, x, V, SELF), _run(desc, hp, x, V, SELF))


def test_17_columns_keep_the_full_evaluation():
    desc, hp, x, V = _inputs("SE+M52+WN", 8, 300, 17, 6)
    assert np.array_equal(_run(desc, hp, x, V, SELF), _run(desc, hp, x, V, SELF, symmetric=False))


def test_cross_kernel_is_refused():
    desc, hp, x, V = _inputs("SE", 8, 65, 1, 7)
    with pytest.raises(ValueError, match="symmetric"):
        G.kernel_matmul(PR.cov_of(desc), hp, x, V, x.copy(), symmetric=True)


@pytest.mark.parametrize("nrhs", [1, 16])
@pytest.mark.parametrize("n", [130, 300])
def test_cg_by_the_symmetric_product(n, nrhs):
    """test_gpu_solve_cg.py's problem (sigma = sigma_n = 1, d = 3, tol 1e-10) and acceptance"""
    tol, maxit = 1e-10, 400
    rng = np.random.default_rng(n + nrhs)
    x, B = rng.random((3, n)), rng.standard_normal((n, nrhs))
    hp = O.default_hp([O.SE, O.WN], 3, sigma=1.0, noise=1.0)
    md = G.GPRModel(G.SquaredExp() + G.WhiteNoise(), hp, x, B[:, 0] if nrhs == 1 else B)
    K = R.kernel_ld([SE, WN], hp, x).astype(np.float64)
    X, iters, relres = G.solve_cg(md, tol=tol, maxit=maxit, symmetric=True)
    iters0 = G.solve_cg(md, tol=tol, maxit=maxit)[1]
    X = X.reshape(n, -1)
    Xs = np.linalg.solve(K, B)
    cond = np.linalg.cond(K, 2)
    err = np.linalg.norm(X - Xs, axis=0) / np.linalg.norm(Xs, axis=0)
    true = np.linalg.norm(B - K @ X, axis=0) / np.linalg.norm(B, axis=0)
    print(f"iters {iters} (full evaluation: {iters0}), relres {relres.max():.3g}, "
          f"true {true.max():.3g}, err {err.max():.3g}, cond {cond:.1f}")
    assert iters < maxit and abs(iters - iters0) <= 1
    assert relres.shape == (nrhs,) and np.all(relres <= 10 * tol) and np.all(true <= 10 * tol)
    assert np.all(err <= cond * relres)


def test_free_gradient_by_the_symmetric_product():
    """test_gpu_mll_grad_free.py's random-probe case: both routes within its bound of the same-Z
    estimate in long double (each with its own residuals), hence within the two bounds' sum of
    each other"""
    import test_gpu_mll_grad_free as MG
    n, m, seed, desc = 130, 15, 0, [SE, M52, WN]
    hp, x, y, md = MG._model(desc, n, n + len(desc) + m)
    Z = MG._device_randn(md.ctx, seed, n * m).reshape(m, n).T
    K = R.kernel_ld(desc, hp, x).astype(np.float64)
    Kinv = np.linalg.inv(K).astype(LD)
    a, U, Zl = Kinv @ y.astype(LD), Kinv @ Z.astype(LD), Z.astype(LD)
    ref, T, S = GF.form_ref(desc, hp, x, np.outer(a, a) - (U @ Zl.T) / LD(m),
                            np.outer(np.abs(a), np.abs(a)) + (np.abs(U) @ np.abs(Zl).T) / LD(m))
    kappa = np.linalg.cond(K, 2)
    res = {}
    for sym in (True, False):
        g, iters, relres = G.mll_grad_free(md, probes=m, seed=seed, tol=1e-12, maxit=20 * n,
                                           symmetric=sym)
        bound = 4 * kappa * relres.max() * S + (1e-13 + (n + (m + 1) + 2 * MG.D + 16) * R.U) * T
        err = np.abs(g.astype(LD) - LD(-0.5) * ref)
        print(f"symmetric={sym}: iters {iters}, max relres {relres.max():.3g}, "
              f"max |err| / bound = {float(np.max(err / bound)):.3g}")
        assert np.all(err <= bound)
        res[sym] = (g, bound)
    assert np.all(np.abs(res[True][0] - res[False][0]) <= res[True][1] + res[False][1])
