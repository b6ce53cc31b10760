// Inter-workgroup hand-off of the single-launch triangular sweeps (potrf.hip's dpotrs sweeps,
// append.hip's skinny forward solve): one monotonic "blocks done" counter, the payload in a
// buffer of its own that is never read before it is written inside the launch.
#pragma once
#include <hip/hip_runtime.h>

// SWEEP_SC1 (default): the hand-off vector is written and read ONLY with sc1 (L2-coherent,
// write-through) accesses and the counter is an sc1 store polled by sc1 loads, each polling
// wave loading only after its own poll matched -- MI355X_MICROARCH.md's first sc1 hand-off
// row (hipMalloc memory, one workgroup per CU), which needs neither the producer's L2
// write-back (release, 1.7-6.5 us) nor the consumer's L1 invalidate (acquire, 1.7-7 us) on
// each of the 256 hops of a sweep.  SWEEP_SC1=0: plain accesses behind agent fences.
#ifndef SWEEP_SC1
#define SWEEP_SC1 1
#endif
__device__ __forceinline__ double hand_ld(const double* p) {
#if SWEEP_SC1
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}
__device__ __forceinline__ void hand_st(double* p, double v) {
#if SWEEP_SC1
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *p = v;
#endif
}

// Block until at least `need` blocks are published; `known` caches the last observed count.
__device__ __forceinline__ void sweep_wait(int* sync, int need, int& known, int lane) {
  if (known >= need) return;
  int v = 0;
  if (lane == 0) {
    while ((v = __hip_atomic_load(&sync[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < need)
      __builtin_amdgcn_s_sleep(1);
  }
  known = __shfl(v, 0);
#if SWEEP_SC1
  // no instruction: keeps the compiler from hoisting the sc1 hand-off loads above the poll
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#else
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
}

__device__ __forceinline__ void sweep_publish(int* sync, int value) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave, before the barrier
  __syncthreads();
  if (threadIdx.x == 0) {
#if !SWEEP_SC1
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    __hip_atomic_store(&sync[1], value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
