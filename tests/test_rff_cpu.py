"""CPU: the random-feature calls are exported and bound, and the sincos of rff_sincos.hpp, restated
here in NumPy FP64 operation by operation, stays within C_POLY = 1.41 u (u = 2^-53) of long-double
sin(2 pi r) / cos(2 pi r) on r in [-1/2, 1/2] (measured: 1.4023 u sine, 1.3979 u cosine).  The
restatement rounds every multiply-add twice, the device fuses them, so the GPU tests allow
2 C_POLY (tests/test_gpu_rff.py)."""
import numpy as np

import kernel_ref_ld as R

C_POLY = 1.41
_S = [float.fromhex(h) for h in (
    "0x1.921fb54442d18p+2", "-0x1.4abbce625be53p+5", "0x1.466bc6775aae2p+6", "-0x1.32d2cce62bd86p+6",
    "0x1.50783487ee782p+5", "-0x1.e3074fde8871fp+3", "0x1.e8f434d018d63p+1", "-0x1.6fadb9f155744p-1",
    "0x1.aaec32af93359p-4")]
_C = [float.fromhex(h) for h in (
    "0x1p+0", "-0x1.3bd3cc9be45dep+4", "0x1.03c1f081b5ac4p+6", "-0x1.55d3c7e3cbffap+6",
    "0x1.e1f506891babbp+5", "-0x1.a6d1f2a204a8cp+4", "0x1.f9d38a3763cc3p+2", "-0x1.b6e24f44b128fp+0",
    "0x1.20c62c2f2d7f5p-2")]


def sincos2pi(r):
    """rff_sincos2pi: (sin(2 pi r), cos(2 pi r)) for |r| <= 1/2"""
    k = np.rint(4.0 * r)
    s = r - 0.25 * k
    z = s * s
    ps, pc = np.full_like(r, _S[8]), np.full_like(r, _C[8])
    for i in range(7, 0, -1):
        ps, pc = ps * z + _S[i], pc * z + _C[i]
    ss, cc = s * (ps * z + _S[0]), pc * z + 1.0
    n = k.astype(np.int64) & 3
    sn, cs = np.where(n & 1, cc, ss), np.where(n & 1, ss, cc)
    return np.where(n & 2, -sn, sn), np.where((n + 1) & 2, -cs, cs)


def test_symbols_and_names():
    import gpr_amd as G
    from gpr_amd import _lib
    for name in ("gpr_rff_draw", "gpr_rff_matmul"):
        assert name in _lib.header_exports() and hasattr(_lib.lib, name)
    assert {"sample_paths", "PosteriorPaths"} <= set(G.__all__)


def test_sincos_restatement_error():
    r = np.concatenate([np.linspace(-0.5, 0.5, 2000001),
                        np.random.default_rng(0).uniform(-0.5, 0.5, 2000000),
                        [0.125, -0.125, 0.375, -0.375, 0.25, -0.25, 0.5, -0.5, 0.0]])
    sn, cs = sincos2pi(r)
    a = 2 * R.PI_LD * r.astype(R.LD)
    es = float(np.abs(sn.astype(R.LD) - np.sin(a)).max() / R.U)
    ec = float(np.abs(cs.astype(R.LD) - np.cos(a)).max() / R.U)
    print(f"sin {es:.4f} u, cos {ec:.4f} u")
    assert es <= C_POLY and ec <= C_POLY
