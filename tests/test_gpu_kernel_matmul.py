"""GPU: the matrix-free product Out = K(xa, xb) V (gpr_kernel_matmul) against the long-double
kernel of kernel_ref_ld.py multiplied by V in long double.

Inputs in the unit cube, hyper-parameters in [0.3, 2] (the range of the project's 1e-13 bar for
kernel entries).  Componentwise bound: |out - ref|_i <= (1e-13 + (nb + 8) u) sum_j |K_ij| |V_j|
-- 1e-13 for the entries, (nb + 8) u for any summation order plus the MFMA accumulations.
"""
import numpy as np
import pytest
import torch

import kernel_ref_ld as R
import test_product_cpu as PR
from kernel_ref_ld import CROSS, LD, M52, PER, SAME_OBJECT, SE, SELF, WN

pytestmark = pytest.mark.gpu

G = pytest.importorskip("gpr_amd")

DESCS = {"SE": [SE], "SE+M52+WN": [SE, M52, WN], "PER": [PER], "SE*PER+WN": [[SE, PER], WN],
         "5SE+WN": [SE, SE, SE, SE, SE, WN]}

# (description, d, na, nb, nv, same, GPR_KMM_SLABS, (ldv - nb, ldo - na))
CASES = [
    ("SE", 1, 1, 1, 1, CROSS, 0, (0, 0)),
    ("SE", 8, 64, 64, 17, CROSS, 0, (0, 0)),          # one full tile: the operand layout
    ("SE", 8, 63, 65, 15, CROSS, 0, (0, 0)),
    ("SE", 21, 129, 200, 64, CROSS, 0, (0, 0)),
    ("SE", 8, 300, 130, 65, CROSS, 0, (0, 0)),
    ("SE+M52+WN", 8, 129, 200, 17, CROSS, 1, (0, 0)),
    ("SE+M52+WN", 1, 300, 130, 1, CROSS, 3, (0, 0)),
    ("SE+M52+WN", 21, 63, 65, 64, CROSS, 0, (0, 0)),
    ("PER", 1, 64, 64, 15, CROSS, 0, (0, 0)),
    ("PER", 8, 129, 200, 1, CROSS, 3, (0, 0)),         # two slabs, the second ends ragged
    ("PER", 21, 63, 65, 17, CROSS, 0, (0, 0)),
    ("SE*PER+WN", 8, 300, 130, 17, CROSS, 3, (0, 0)),
    ("SE*PER+WN", 1, 129, 200, 65, CROSS, 1, (0, 0)),
    ("SE*PER+WN", 21, 64, 64, 1, CROSS, 0, (0, 0)),
    ("5SE+WN", 8, 129, 200, 15, CROSS, 3, (0, 0)),     # two part groups, each in slabs
    ("5SE+WN", 21, 63, 65, 1, CROSS, 0, (0, 0)),
    ("5SE+WN", 1, 300, 130, 64, CROSS, 0, (0, 0)),
    ("SE+M52+WN", 8, 64, 64, 17, SELF, 0, (0, 0)),
    ("SE+M52+WN", 8, 64, 64, 17, SAME_OBJECT, 0, (0, 0)),
    ("SE+M52+WN", 1, 1, 1, 1, SELF, 0, (0, 0)),
    ("PER", 1, 1, 1, 1, SAME_OBJECT, 0, (0, 0)),
    ("SE*PER+WN", 8, 200, 200, 15, SELF, 3, (0, 0)),   # diagonal tiles in different slabs
    ("5SE+WN", 8, 200, 200, 1, SELF, 0, (0, 0)),       # the noise rides on the last group
    ("SE", 8, 63, 65, 17, CROSS, 0, (7, 5)),
    ("SE+M52+WN", 8, 200, 200, 65, SELF, 3, (6, 3)),
]


def _inputs(name, d, na, nb, nv, same, seed):
    rng = np.random.default_rng(seed)
    desc = DESCS[name]
    hp = rng.uniform(0.3, 2.0, sum(R.width(k, d) for k in R.flat(desc)))
    xa = rng.random((d, na))
    xb = rng.random((d, nb)) if same == CROSS else None
    V = rng.standard_normal((nb, nv))
    return desc, hp, xa, xb, V


def _run(desc, hp, xa, xb, V, same, pad=(0, 0)):
    """the product through gpr_amd.kernel_matmul, V and Out as device buffers with padded leading
    dimensions: V's padding rows are NaN, Out is pre-filled with a sentinel"""
    ctx = G.default_context()
    na, (nb, nv) = xa.shape[1], V.shape
    dV = torch.full((nv, nb + pad[0]), float("nan"), dtype=torch.float64, device=ctx.device)
    dV[:, :nb] = torch.from_numpy(np.ascontiguousarray(V.T)).to(ctx.device)
    out = torch.full((nv, na + pad[1]), -7.5, dtype=torch.float64, device=ctx.device)
    torch.cuda.synchronize()
    xp = None if same == SELF else xa if same == SAME_OBJECT else xb
    G.kernel_matmul(PR.cov_of(desc), hp, xa, dV, xp, out=out)
    ctx.sync()
    o = out.cpu().numpy()
    assert np.all(o[:, na:] == -7.5), "Out's padding was written"
    return o[:, :na].T.copy()


@pytest.mark.parametrize("name,d,na,nb,nv,same,slabs,pad", CASES)
def test_product_against_long_double(knobs, name, d, na, nb, nv, same, slabs, pad):
    knobs("GPR_KMM_SLABS", slabs)
    desc, hp, xa, xb, V = _inputs(name, d, na, nb, nv, same, 1000 * na + nb + nv)
    out = _run(desc, hp, xa, xb, V, same, pad)
    K = R.kernel_ld(desc, hp, xa, xb, same=same)
    ref = K @ V.astype(LD)
    bound = (1e-13 + (nb + 8) * R.U) * (np.abs(K) @ np.abs(V).astype(LD))
    err = np.abs(out.astype(LD) - ref)
    print(f"max |err| / bound = {float(np.max(err / bound)):.3g}")
    assert np.all(np.isfinite(out))
    assert np.all(err <= bound)


def test_two_calls_agree_bit_for_bit(knobs):
    knobs("GPR_KMM_SLABS", 3)
    desc, hp, xa, xb, V = _inputs("SE*PER+WN", 8, 300, 130, 17, CROSS, 5)
    a = _run(desc, hp, xa, xb, V, CROSS)
    b = _run(desc, hp, xa, xb, V, CROSS)
    assert np.array_equal(a, b)
