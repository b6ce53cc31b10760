"""GPU: the matrix-free product (gpr_kernel_matmul) evaluates the element gpr_kernel's Gram route
writes, bit for bit -- the claim of include/gpr_hip.h and of kmatmul.hip's header -- and argument
errors.

With V a selection of unit vectors, V = I[:, cols], column c of the product is column cols[c] of K
plus exact zeros, so the product must return gpr_kernel's columns under numpy.array_equal:
  * the second MFMA multiplies a tile element by V's 0.0 or 1.0: both products are exact, and K
    is finite, so 0.0 K is 0.0 and not NaN (the tile's rows past nb are points of zero operands:
    finite values times exact zeros);
  * a column of V has a single 1.0, so every sum the product forms for an output element -- the
    four k-steps of an MFMA, the accumulation over a slab's blocks, wave 0's plus wave 1's half,
    the slabs' partials in kmm_reduce_kernel -- adds the one value and zeros: no rounding;
  * the element itself comes from gram_tile on the operands of the same gram_prepare call (the
    centre is the row points', also for the columns of a cross matrix), -D from the same products
    (2 y_a,k) y_b,k in the same k order whichever operand sits on the tile's rows.
The comparison therefore carries everything tests/test_gpu_kernel_domain.py holds gpr_kernel to
(the element bound far from the unit cube, exact zeros past the underflow, the clamp) over to the
product without a new tolerance.  The route: gpr_kernel takes the Gram form for a 16-byte aligned
K with an even leading dimension, so every n here is even.

gpr_kernel's own kernels differ from the product's: one SquaredExp part in the symmetric forms is
built by kmat_symu_kernel (other operand orientation, unclamped exponential in its interior
units), 8 < d <= 20 by tiles with the k-steps compiled in where the product walks them at run
time, and more than four parts by one accumulating launch per group.
"""
import numpy as np
import pytest
import torch

import kernel_ref_ld as R
import test_gpu_kernel_domain as KD
import test_product_cpu as PR
from kernel_ref_ld import LD, SE, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

GPR_E_ARG = -1
SENT = -7.5
CROSS_NAMES = ("SE", "SE+SE+WN", "M52+WN", "SE*SE+WN")
CROSS_CASES = [(f, name) for f in ("F1", "F1s5", "F2-1e6-d8", "F2-1e6-d21", "F3a", "F3b")
               for name in CROSS_NAMES] + [("F5", name) for name in KD.PLISTS]
SLABS = (0, 3, 1)  # the default count, three slabs, and no partials at all


def _unit(nb, cols):
    V = np.zeros((nb, len(cols)))
    V[list(cols), np.arange(len(cols))] = 1.0
    return V


@pytest.mark.parametrize("fam,name", CROSS_CASES)
def test_cross_columns_are_gpr_kernels(fam, name, knobs):
    """K(x, xp) I against gpr_kernel's K(x, xp), every column (m <= 130: up to three passes of 64
    columns of V)"""
    desc = KD.lists_of(fam)[name]
    x, xp, hp = KD._inputs(fam, name)
    cov = PR.cov_of(desc)
    assert x.shape[1] % 2 == 0 and xp.shape[1] <= 130
    K = G.kernel(cov, hp, x, xp)
    assert np.all(np.isfinite(K))
    for slabs in SLABS:
        knobs("GPR_KMM_SLABS", slabs)
        out = G.kernel_matmul(cov, hp, x, np.eye(xp.shape[1]), xp)
        assert np.array_equal(out, K), f"{fam} {name}, GPR_KMM_SLABS={slabs}: " \
            f"{np.count_nonzero(out != K)} of {K.size} elements differ"


def _cols64(n):
    """64 columns: 0..53 (the ladder's base, its copy and every rung; positions 0..31 and 32..53
    of the first diagonal tile, i.e. both quadrants that hold a diagonal) and ten more spread to
    n - 1"""
    cols = sorted(set(range(54)) | set(np.linspace(54, n - 1, 10).astype(int).tolist()))
    assert len(cols) == 64 and cols[-1] == n - 1
    return cols


@pytest.mark.parametrize("name", CROSS_NAMES)
@pytest.mark.parametrize("fam", ["F1", "F2-1e4-d3"])
def test_same_object_forms(fam, name, knobs):
    """GPR_SELF (eps per term and the noise on the diagonal) and GPR_SAME_OBJECT (eps, no noise)
    against the two symmetric forms of gpr_kernel"""
    desc = KD.KLISTS[name]
    x, _, hp = KD._inputs(fam, name)
    cov = PR.cov_of(desc)
    n = x.shape[1]
    assert n % 2 == 0 and 54 >= 2 + len(R.f1_targets())
    cols = _cols64(n)
    V = _unit(n, cols)
    Kself, Ksame = G.kernel(cov, hp, x), G.kernel(cov, hp, x, x)
    if WN in desc:
        assert not np.array_equal(np.diag(Kself), np.diag(Ksame))
    for slabs in SLABS:
        knobs("GPR_KMM_SLABS", slabs)
        assert np.array_equal(G.kernel_matmul(cov, hp, x, V), Kself[:, cols]), (slabs, "SELF")
        assert np.array_equal(G.kernel_matmul(cov, hp, x, V, x), Ksame[:, cols]), (slabs, "SAME_OBJECT")


@pytest.mark.parametrize("variant", ["i", "ii"])
def test_around_the_clamp_limit(variant, knobs):
    """kernel_ref_ld.f4_planted: distances up to 5.4e6 between points just below KU_NC_LIM, which
    gpr_kernel's one-part build takes through the unclamped exponential in its interior units and
    the product through the clamped one, and (ii) a point both must clamp for"""
    desc = [SE, WN]
    x, _, hp = R.f4_planted(desc, 3, variant)
    n = x.shape[1]
    cov = PR.cov_of(desc)
    cols = sorted(set(R.F4_IDX) | set(np.linspace(0, n - 2, 27).astype(int).tolist()))
    assert len(cols) == 32 and n == 1040
    K = G.kernel(cov, hp, x)
    for slabs in SLABS:
        knobs("GPR_KMM_SLABS", slabs)
        assert np.array_equal(G.kernel_matmul(cov, hp, x, _unit(n, cols)), K[:, cols]), slabs


def test_grouped_parts(knobs):
    """5SE+WN, cross: two groups (KMAXP = 4 parts, then one).  gpr_kernel's accumulating launch
    starts its tile from the stored sum of the first group and adds the fifth part,
    ((p1 + p2) + p3) + p4) + p5; the product adds the second group's result, 0 + p5 = p5 exactly,
    to the first group's in Out: the same sum in the same order (launch_gram_groups in assembly.hip,
    kmm_apply in kmatmul.hip), hence the same bits."""
    desc = [SE, SE, SE, SE, SE, WN]
    x, xp, hp = R.f2_far(desc, 1e4, 8)
    cov = PR.cov_of(desc)
    K = G.kernel(cov, hp, x, xp)
    for slabs in SLABS:
        knobs("GPR_KMM_SLABS", slabs)
        assert np.array_equal(G.kernel_matmul(cov, hp, x, np.eye(xp.shape[1]), xp), K), slabs


@pytest.mark.parametrize("fam", ["F2-1e6-d8", "F3b"])
def test_dense_v_off_the_unit_cube(fam):
    """A standard-normal V, nv = 17 (64 staged columns):
    |out - K_ref V| <= B @ |V| + (nb + 8) u |K_ref| @ |V|, B the Gram form's element bound of
    kernel_ref_ld and (nb + 8) u the summation term of tests/test_gpu_kernel_matmul.py."""
    name = "SE+SE+WN"
    x, xp, hp = KD._inputs(fam, name)
    Kr, bound, _ = KD._reference(fam, name, "gram", True)
    nb = xp.shape[1]
    V = np.random.default_rng(nb + 17).standard_normal((nb, 17))
    out = G.kernel_matmul(PR.cov_of(KD.KLISTS[name]), hp, x, V, xp)
    Va = np.abs(V).astype(LD)
    tol = bound @ Va + LD((nb + 8) * R.U) * (np.abs(Kr) @ Va)
    err = np.abs(out.astype(LD) - Kr @ V.astype(LD))
    print(f"{fam}: max |err| / bound = {float(np.max(err / tol)):.3g}")
    assert np.all(np.isfinite(out)) and np.all(err <= tol)


# ---------------------------------------------------------------------------------------
# argument errors: GPR_E_ARG naming the argument, before anything is written
# ---------------------------------------------------------------------------------------
BAD_ARGS = [
    (dict(same=3), "same"), (dict(dXa=None), "dXa"), (dict(dXb=None), "dXb"),
    (dict(dV=None), "dV"), (dict(dOut=None), "dOut"),
    (dict(na=0), "na="), (dict(nb=0), "nb="), (dict(nv=0), "nv="),
    (dict(same=1), "same-object"), (dict(same=2), "same-object"),   # na != nb
    (dict(ldv=-1), "ldv"), (dict(ldo=-1), "ldo"),
]


@pytest.mark.parametrize("change,word", BAD_ARGS, ids=[f"{list(c)[0]}={list(c.values())[0]}" for c, _ in BAD_ARGS])
def test_argument_errors(change, word):
    ctx = G.default_context()
    d, na, nb, nv = 3, 70, 66, 2
    rng = np.random.default_rng(3)
    desc = [SE, WN]
    hp = rng.uniform(0.3, 2.0, d + 2)
    dxa, dxb = ctx.colmajor(rng.random((d, na))), ctx.colmajor(rng.random((d, nb)))
    dV = ctx.colmajor(rng.standard_normal((nb, nv)))
    out = torch.full((nv, na), SENT, dtype=torch.float64, device=ctx.device)
    torch.cuda.synchronize()
    a = dict(dXa=dxa, na=na, dXb=dxb, nb=nb, same=0, dV=dV, nv=nv, ldv=nb, dOut=out, ldo=na)
    a.update(change)
    if a["ldv"] == -1:
        a["ldv"] = nb - 1
    if a["ldo"] == -1:
        a["ldo"] = na - 1
    ka, nk = KD.karr(desc)
    rc = G._lib.lib.gpr_kernel_matmul(ctx.h, ka, nk, KD._dp(hp), d, KD._P(a["dXa"]), a["na"],
                                      KD._P(a["dXb"]), a["nb"], a["same"], R.EPS, KD._P(a["dV"]),
                                      a["nv"], a["ldv"], KD._P(a["dOut"]), a["ldo"])
    msg = G._lib.lib.gpr_last_error(ctx.h).decode()
    assert rc == GPR_E_ARG, (rc, msg)
    assert word in msg, msg
    ctx.sync()
    assert torch.all(out == SENT).item()
