// sin(2 pi r) and cos(2 pi r) for |r| <= 1/2 from one shared reduction, in plain FP64: no call
// into the math library, no branch, no table (rff.hip's random features).
//
//   k = rint(4 r) in {-2..2}, s = r - k / 4: exact, |s| <= 1/8 -- the angle 2 pi s lies in the
//   octant [-pi/4, pi/4];
//   z = s^2;  sin(2 pi s) = s (S0 + z (S1 + .. + z S8)),  cos(2 pi s) = 1 + z (C1 + .. + z C8)
//   with Sk = (-1)^k (2 pi)^(2k+1) / (2k+1)!, Ck = (-1)^k (2 pi)^(2k) / (2k)!, each rounded once
//   from 80 digits: the Taylor polynomials in s, so that 2 pi never multiplies the argument.  The
//   first dropped terms are (pi/4)^19 / 19! = 8.3e-20 and (pi/4)^18 / 18! = 2.0e-18, below 0.02 u;
//   quarter turns: k & 3 = 1, 3 swap the two, k & 2 negates the sine, (k + 1) & 2 the cosine.
// tests/test_rff_cpu.py restates this operation by operation in NumPy (multiply-adds rounded
// twice there, once here) and measures 1.41 u against long-double sin / cos.
#pragma once

#if defined(__HIPCC__)
#define RFF_HD __host__ __device__
#else
#define RFF_HD
#endif

RFF_HD inline void rff_sincos2pi(double r, double& sn, double& cs) {
  const double k = __builtin_rint(4.0 * r);
  const double s = __builtin_fma(k, -0.25, r);
  const double z = s * s;
  double ps = 0x1.aaec32af93359p-4, pc = 0x1.20c62c2f2d7f5p-2;
  ps = __builtin_fma(ps, z, -0x1.6fadb9f155744p-1);
  pc = __builtin_fma(pc, z, -0x1.b6e24f44b128fp+0);
  ps = __builtin_fma(ps, z, 0x1.e8f434d018d63p+1);
  pc = __builtin_fma(pc, z, 0x1.f9d38a3763cc3p+2);
  ps = __builtin_fma(ps, z, -0x1.e3074fde8871fp+3);
  pc = __builtin_fma(pc, z, -0x1.a6d1f2a204a8cp+4);
  ps = __builtin_fma(ps, z, 0x1.50783487ee782p+5);
  pc = __builtin_fma(pc, z, 0x1.e1f506891babbp+5);
  ps = __builtin_fma(ps, z, -0x1.32d2cce62bd86p+6);
  pc = __builtin_fma(pc, z, -0x1.55d3c7e3cbffap+6);
  ps = __builtin_fma(ps, z, 0x1.466bc6775aae2p+6);
  pc = __builtin_fma(pc, z, 0x1.03c1f081b5ac4p+6);
  ps = __builtin_fma(ps, z, -0x1.4abbce625be53p+5);
  pc = __builtin_fma(pc, z, -0x1.3bd3cc9be45dep+4);
  const double ss = s * __builtin_fma(ps, z, 0x1.921fb54442d18p+2);
  const double cc = __builtin_fma(pc, z, 1.0);
  const int n = (int)k;
  const double a = (n & 1) ? cc : ss, b = (n & 1) ? ss : cc;
  sn = (n & 2) ? -a : a;
  cs = ((n + 1) & 2) ? -b : b;
}
