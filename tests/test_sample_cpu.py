"""CPU: the normal generator behind gpr_randn, restated in NumPy, and the sampling exports.

The restatement is the reference of tests/test_gpu_sample.py: Philox4x32-10 (multipliers
0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85) and the Box-Muller mapping of
include/gpr_hip.h.  It is pinned here by three known answers of the generator (the first two
are Random123's published vectors, the third its pi-digits vector), and its own moments at
N = 2^22 are shown to lie inside the bounds the GPU test applies to the device stream.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
SH32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars), key: two uint32 scalars -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in ctr)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2           # 32 x 32 -> 64 bit products: no wrap in uint64
        n0 = (p1 >> SH32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> SH32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & MASK32, n2, p0 & MASK32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def randn_ref(seed, offset, count, with_r=False):
    """Elements offset .. offset + count of the standard-normal stream of `seed`."""
    seed, offset, count = int(seed), int(offset), int(count)
    g = np.arange(count, dtype=np.uint64) + np.uint64(offset)
    p = g >> np.uint64(1)
    w0, w1, w2, w3 = philox4x32_10((p & MASK32, p >> SH32, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    a = ((w1 << SH32) | w0) >> np.uint64(11)
    b = ((w3 << SH32) | w2) >> np.uint64(11)
    u1 = (a.astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = (b.astype(np.float64) + 0.5) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    t = 2.0 * np.pi * u2
    z = np.where((g & np.uint64(1)) == 0, r * np.cos(t), r * np.sin(t))
    return (z, r) if with_r else z


def moment_bounds_hold(z):
    """The three 5-sigma moment checks of the issue; returns the figures for the report."""
    N = z.size
    p = 0.0026998  # P(|z| > 3)
    mean, var, tail = z.mean(), z.var(), np.count_nonzero(np.abs(z) > 3.0) / N
    ok = (abs(mean) <= 5.0 / np.sqrt(N) and abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / N)
          and abs(tail - p) <= 5.0 * np.sqrt(p * (1.0 - p) / N))
    return ok, (mean, var, tail)


def _words(*w):
    return tuple(int(x, 16) for x in w)


def test_philox_known_answers():
    kat = [
        ((0, 0, 0, 0), (0, 0), _words("6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8")),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, _words("408f276d", "41c83b0e", "a20bc7c6", "6d5451fd")),
        (_words("243f6a88", "85a308d3", "13198a2e", "03707344"), _words("a4093822", "299f31d0"),
         _words("d16cfe09", "94fdcceb", "5001e420", "24126ea1")),
    ]
    for ctr, key, want in kat:
        got = tuple(int(x) for x in philox4x32_10(ctr, key))
        assert got == want, (ctr, key, [hex(x) for x in got])


def test_stream_is_a_function_of_the_global_index():
    z = randn_ref(7, 0, 4099)
    assert np.array_equal(z[1001:], randn_ref(7, 1001, 3098))
    assert np.array_equal(z[3:4], randn_ref(7, 3, 1))
    assert not np.array_equal(z, randn_ref(8, 0, 4099))
    big = randn_ref(2 ** 63 + 5, 2 ** 33 + 1, 9)      # counter and key words above 2^32
    assert np.all(np.isfinite(big)) and np.unique(big).size == 9


def test_restatement_moments_inside_the_gpu_bounds():
    ok, (mean, var, tail) = moment_bounds_hold(randn_ref(1, 0, 1 << 22))
    print(f"restatement, seed 1, N = 2^22: mean {mean:.3e} var-1 {var - 1:.3e} tail {tail:.6f}")
    assert ok, (mean, var, tail)


def test_package_exports_the_sampling_names():
    import gpr_amd as G
    for name in ("NormalDistribution", "GaussianProcess", "sample", "sample_posterior"):
        assert hasattr(G, name) and name in G.__all__, name


def test_lib_binds_the_sampling_symbols():
    import gpr_amd._lib as L
    for name in ("gpr_randn", "gpr_mvn_sample", "gpr_mvn_factor", "gpr_sample_prior"):
        assert name in L._SIGS and hasattr(L.lib, name), name
        assert name in L.header_exports(), name
