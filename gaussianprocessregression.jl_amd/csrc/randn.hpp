// Counter-based standard normals: Philox4x32-10 (Salmon et al., SC'11) + Box-Muller.
// Element g of the stream of `seed` is a pure function of (seed, g):
//   counter = (lo32(g >> 1), hi32(g >> 1), 0, 0), key = (lo32(seed), hi32(seed));
//   the four output words w0..w3 give u1 = (((w1 << 32 | w0) >> 11) + 0.5) 2^-53 and u2 likewise
//   from (w3, w2); r = sqrt(-2 ln u1); element g = r cos(2 pi u2) for even g, r sin(2 pi u2)
//   for odd g.  One Philox block therefore serves the pair (2p, 2p + 1).
// Host and device compile the same integer code; tests/test_sample_cpu.py restates it in NumPy.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GPR_HD __host__ __device__
#else
#define GPR_HD
#endif

GPR_HD inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                 uint32_t k1, uint32_t (&out)[4]) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += W0;
    k1 += W1;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// the pair (elements 2p and 2p + 1) of the stream of `seed`
GPR_HD inline void randn_pair(uint64_t seed, uint64_t p, double& even, double& odd) {
  uint32_t w[4];
  philox4x32_10((uint32_t)p, (uint32_t)(p >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
  const uint64_t a = ((uint64_t)w[1] << 32) | w[0], b = ((uint64_t)w[3] << 32) | w[2];
  const double u1 = ((double)(a >> 11) + 0.5) * 0x1p-53;
  const double u2 = ((double)(b >> 11) + 0.5) * 0x1p-53;
  const double r = sqrt(-2.0 * log(u1));
  double s, c;
#if defined(__HIP_DEVICE_COMPILE__)
  sincospi(2.0 * u2, &s, &c);  // 2 u2 is exact: no rounding of the argument by pi
#else
  s = std::sin(6.283185307179586476925 * u2);
  c = std::cos(6.283185307179586476925 * u2);
#endif
  even = r * c;
  odd = r * s;
}
