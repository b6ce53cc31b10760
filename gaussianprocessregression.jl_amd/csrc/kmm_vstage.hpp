// The staged V block of the matrix-free products (kmatmul.hip, kmatmul_f32.hip): 64 rows x 16 NVB
// columns of V in LDS, column by column, and the register prefetch of the next block.
#pragma once
#include "gram_tile.hpp"

namespace {

constexpr int KMM_VS = KT + 2;   // LDS stride (doubles) between the staged V block's columns
constexpr int KMM_MAXS = 64;     // most slabs of one launch
typedef double kv2 __attribute__((ext_vector_type(2)));

// this thread's share of rows [j0, j0 + 64) x columns [0, 16 NVB) of V: row pair 2 (t & 31) of
// columns (t >> 5) + 8 k.  Zero past nb or nvc, and nothing past them is read.
template <int NVB>
__device__ __forceinline__ void kmm_fetch_v(const double* __restrict__ V, size_t ldv, int nb,
                                            int nvc, int j0, bool vec, kv2 (&r)[2 * NVB]) {
  const int j = j0 + 2 * (int)(threadIdx.x & 31), cg = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 2 * NVB; ++k) {
    const int c = cg + 8 * k;
    kv2 e = {0.0, 0.0};
    if (c < nvc && j < nb) {
      const double* src = V + (size_t)c * ldv + j;
      if (j + 1 < nb) {
        if (vec) {
          e = *reinterpret_cast<const kv2*>(src);
        } else {
          e[0] = src[0];
          e[1] = src[1];
        }
      } else {
        e[0] = src[0];
      }
    }
    r[k] = e;
  }
}

template <int NVB>
__device__ __forceinline__ void kmm_stage_v(const kv2 (&r)[2 * NVB], double* Vs) {
  const int pr = threadIdx.x & 31, cg = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 2 * NVB; ++k)
    *reinterpret_cast<kv2*>(Vs + (cg + 8 * k) * KMM_VS + 2 * pr) = r[k];
}

}  // namespace
