// Accumulation-pipeline probe for the tile-DAG (dag.hip dag_accum): one persistent workgroup
// per CU computes acc += P^T Q over a long K, P = 128 TMR columns, Q = 128 columns of a
// K-contiguous (column-major, ld = K) matrix, TMR = 1: 4 waves (each 64 x 64, today's kernel),
// TMR = 2: 8 waves over a 256 x 128 tile (2 waves per SIMD; Q shared by both row halves: 48 KB
// of operands per 16-deep stage for twice the flops of a 32-KB 128 x 128 stage).
// Answers: per-CU FP64 MFMA rate and HBM traffic per flop of the two shapes before the DAG
// is restructured around either.   Usage: accum_probe [K] [reps] [config] [mode] [warm seconds]
// (warm seconds: back-to-back launches of the same kernel before the timed ones, so the rate and
// the in-kernel clock -- s_memtime / s_memrealtime around the loop, median over the workgroups
// of the last launch -- are those of a chip that has settled under the load)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

typedef double d4v __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int DT = 128, DTK = 16, DNCH = DTK / 2, DRPD = 64 / DNCH;

__device__ __forceinline__ int swz(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int lidx(int row, int chunk) { return row * DTK + ((chunk ^ swz(row)) << 1); }

template <int VM>
__device__ __forceinline__ void vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM) : "memory");
}

typedef __attribute__((address_space(3))) const char* ldsp;

// One 1-KB LDS-DMA piece in the scalar-base form: lane source = sbase (SGPR pair) + voff (32-bit
// VGPR byte offset), LDS destination = lds_dst (wave-uniform byte address, through M0) + 16 lane.
// M0 is written in the statement that reads it and handed back as found.  Not counted by the
// compiler: the caller keeps vmcnt.
__device__ __forceinline__ void dma16_sbase(unsigned voff, const char* sbase, unsigned lds_dst) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}

// TMR: 128-row tiles of P (1 or 2); NW: waves (4 = one per SIMD, 8 = two); each wave owns
// (128 TMR / (NW / 2)) rows x 64 columns; NSTG: LDS stages; DBUF: next stage's fragments read
// into a second register set during the current stage's MFMAs.  RING (NSTG = 5, DBUF): ONE
// barrier per two stages -- period p computes stages 2 p and 2 p + 1, DMA of stages 2 p + 4 and
// 2 p + 5 issued behind its barrier (dag.hip's dag_accum before round 8).  SBASE (RING): the same
// schedule with no vector-ALU address arithmetic in the loop -- DMA sources are a scalar base per
// 8-row piece plus a loop-invariant 32-bit lane offset, and five periods are unrolled so that the
// ring position is a compile-time value and every fragment read is a loop-invariant lane base plus
// an immediate.
template <int TMR, int NW, int NSTG, bool DBUF, bool RING = false, bool SBASE = false>
__global__ __launch_bounds__(NW * 64, 1) void accum_kernel(const double* __restrict__ M, size_t ld,
                                                          int ncolblk, int nst, int mode,
                                                          double* out, unsigned long long* clk) {
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass cannot instantiate the amdgcn builtins)
  constexpr int PR = DT * TMR;             // P rows (tile rows)
  constexpr int WR = NW / 2;               // wave row groups
  constexpr int RB = PR / WR / 16;         // 16-row blocks per wave
  constexpr int DSTAGE = (PR + DT) * DTK;  // doubles per stage
  constexpr int NDP = PR / (NW * DRPD);    // DMA per wave for P
  constexpr int NDQ = DT / (NW * DRPD);    // DMA per wave for Q
  constexpr int DVM = NDP + NDQ;
  constexpr int DNP = DTK / 8;
  constexpr int NF = 4 + RB;
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w % WR, wn = w / WR;
  const int b = blockIdx.x;
  // mode 0 (hot): every workgroup reads the same P (panels 0..TMR-1) and Q (panel TMR):
  // the pipeline's own rate.  mode 1 (DAG-like): P shared by groups of 32 workgroups (a row
  // of tasks), Q distinct per workgroup (every task its own column panel).  P spans TMR
  // consecutive panels, so it starts at most at panel ncolblk - TMR - 1.
  const int np_ = ncolblk - TMR - 1;
  // mode 2 (L2-resident): mode 0's operands, K wrapped at 1024 rows (64 stages): 2 MB of
  // operands per launch, held in every XCD's 4-MB L2 -- the same MFMA work with no HBM stream
  // mode 3 (own panel): mode 1 with a Q panel of its own for EVERY workgroup (needs ncolblk >=
  // workgroups + TMR; mode 1 at ncolblk = 64 wraps: four workgroups share each Q panel)
  const int pp = mode == 1 || mode == 3 ? (b / 32) % np_ : 0;
  const int qp = mode == 1 ? TMR + (b % np_) : mode == 3 ? TMR + b : TMR;
  const double* P = M + (size_t)pp * DT * ld;
  const double* Q = M + (size_t)qp * DT * ld;
  d4v acc[4][RB];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      if (NW == 4)  // one wave per SIMD: accumulators defined in AGPRs (gemm.hip's idiom), so
                    // the loop never copies them between register files
        asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %1, 0" : "=a"(acc[i][j]) : "v"(0.0));
      else
        acc[i][j] = d4v{0, 0, 0, 0};
    }
  const double* srcP[NDP];
  const double* srcQ[NDQ];
#pragma unroll
  for (int r = 0; r < NDP; ++r) {
    const int row = DRPD * (NW * r + w) + lane / DNCH;
    srcP[r] = P + 2 * ((lane % DNCH) ^ swz(row)) + (size_t)row * ld;
  }
#pragma unroll
  for (int r = 0; r < NDQ; ++r) {
    const int row = DRPD * (NW * r + w) + lane / DNCH;
    srcQ[r] = Q + 2 * ((lane % DNCH) ^ swz(row)) + (size_t)row * ld;
  }
  // (stage s into / out of LDS buffer b)
  auto issue_b = [&](int s, int b) {
    double* base = lds + b * DSTAGE;
    const size_t ko = (size_t)(mode == 2 ? min(s, nst - 1) & 63 : min(s, nst - 1)) * DTK;
#pragma unroll
    for (int r = 0; r < NDP; ++r)
      __builtin_amdgcn_global_load_lds(srcP[r] + ko, base + (NW * r + w) * 128, 16, 0, 0);
#pragma unroll
    for (int r = 0; r < NDQ; ++r)
      __builtin_amdgcn_global_load_lds(srcQ[r] + ko, base + PR * DTK + (NW * r + w) * 128, 16, 0, 0);
  };
  auto issue = [&](int s) { issue_b(s, s % NSTG); };
  auto read_frags_b = [&](d2 (&F)[DNP][NF], int b) {
    const double* ps = lds + b * DSTAGE;
    const double* qs = ps + PR * DTK;
#pragma unroll
    for (int p = 0; p < DNP; ++p) {
      const int ch = (lane >> 4) + 4 * p;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        F[p][i] = *reinterpret_cast<const d2*>(&qs[lidx(wn * 64 + i * 16 + (lane & 15), ch)]);
#pragma unroll
      for (int j = 0; j < RB; ++j)
        F[p][4 + j] = *reinterpret_cast<const d2*>(&ps[lidx(wm * 16 * RB + j * 16 + (lane & 15), ch)]);
    }
  };
  auto read_frags = [&](d2 (&F)[DNP][NF], int s) { read_frags_b(F, s % NSTG); };
  auto mfma_stage = [&](const d2 (&F)[DNP][NF]) {
#pragma unroll
    for (int p = 0; p < DNP; ++p)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < RB; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(F[p][i][h], F[p][4 + j][h], acc[i][j], 0, 0, 0);
  };
  constexpr int NMF = DNP * 2 * 4 * RB, NDS = DNP * NF;
  auto sched = [&]() {
#pragma unroll
    for (int t = 0; t < DVM; ++t) {
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // VMEM read (LDS-DMA)
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
    }
    if (DBUF) {
#pragma unroll
      for (int t = 0; t < NDS; ++t) {
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, NMF - DVM - 2 * NDS, 0);
    } else {
      __builtin_amdgcn_sched_group_barrier(0x008, NMF - DVM, 0);
    }
  };
  d2 F0[DNP][NF], F1[DNP][NF];
  const unsigned long long ck0 = __builtin_amdgcn_s_memtime(), rt0 = __builtin_amdgcn_s_memrealtime();
  if constexpr (RING && SBASE) {
    static_assert(NSTG == 5 && DBUF && TMR == 1 && NW == 4, "written for dag_accum's shape");
    // DMA piece r of an operand: rows 8 (4 r + w) .. + 7.  Scalar base: the piece's first row;
    // lane offset: chunk (swizzled) + row within the piece -- < 7 * 8 ld + 128 bytes
    const char* gP[NDP];
    const char* gQ[NDQ];
    unsigned oP[NDP], oQ[NDQ];
#pragma unroll
    for (int r = 0; r < NDP; ++r) {
      const int row0 = DRPD * (NW * r + w), rl = lane / DNCH;
      const unsigned off = 16u * ((lane % DNCH) ^ swz(row0 + rl)) + (unsigned)rl * (unsigned)(8 * ld);
      gP[r] = reinterpret_cast<const char*>(P + (size_t)row0 * ld);
      gQ[r] = reinterpret_cast<const char*>(Q + (size_t)row0 * ld);
      oP[r] = oQ[r] = off;
      asm volatile("" : "+v"(oP[r]), "+v"(oQ[r]));
    }
    const unsigned lds0 = (unsigned)(uintptr_t)(ldsp)lds;
    // piece t (0..7: P 0..3, then Q 0..3) of stage s into buffer bb
    auto piece = [&](int t, int s, int bb) __attribute__((always_inline)) {
      const size_t ko = (size_t)(mode == 2 ? min(s, nst - 1) & 63 : min(s, nst - 1)) * (DTK * 8);
      const unsigned dst = lds0 + bb * (DSTAGE * 8) + (t >= NDP ? PR * DTK * 8 : 0) + (NW * (t % NDP) + w) * 1024;
      if (t < NDP) dma16_sbase(oP[t], gP[t] + ko, dst);
      else dma16_sbase(oQ[t - NDP], gQ[t - NDP] + ko, dst);
    };
    // fragment reads: lane bases (block p, 64-KB window k), then immediates only
    ldsp qb[DNP][3], pb[DNP][3];
    {
      const int l15 = lane & 15;
      const unsigned a0 = 8u * (l15 * DTK + ((((lane >> 4) ^ swz(l15))) << 1));
#pragma unroll
      for (int p = 0; p < DNP; ++p)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const unsigned ap = a0 ^ (64u * p);
          qb[p][k] = (ldsp)lds + PR * DTK * 8 + wn * (64 * DTK * 8) + ap + k * 65536;
          pb[p][k] = (ldsp)lds + wm * (64 * DTK * 8) + ap + k * 65536;
          asm volatile("" : "+v"(qb[p][k]), "+v"(pb[p][k]));
        }
    }
    typedef __attribute__((address_space(3))) const d2* ldsd2;
    // read t (0..15) of a stage's fragments out of buffer bb (compile-time)
    auto rd = [&](d2 (&F)[DNP][NF], int t, int bb) __attribute__((always_inline)) {
      const int p = t / NF, f = t % NF;
      const int imm = (bb & 1) * (DSTAGE * 8) + (f & 3) * (16 * DTK * 8);
      F[p][f] = *reinterpret_cast<ldsd2>((f < 4 ? qb[p][bb >> 1] : pb[p][bb >> 1]) + imm);
    };
    auto mf = [&](const d2 (&F)[DNP][NF], int t) __attribute__((always_inline)) {  // MFMA t of a stage, mfma_stage's order
      const int j = t % RB, i = (t / RB) % 4, h = (t / (4 * RB)) % 2, p = t / (8 * RB);
      acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(F[p][i][h], F[p][4 + j][h], acc[i][j], 0, 0, 0);
    };
    // half a period: stage s's MFMAs (fragments Fc) with the DMA of stage sd into buffer bd two
    // MFMAs apart behind LEAD MFMAs, then the reads of buffer br into Fn two MFMAs apart
    auto half = [&](const d2 (&Fc)[DNP][NF], d2 (&Fn)[DNP][NF], int sd, int bd, int br, auto leadc) __attribute__((always_inline)) {
      constexpr int lead = decltype(leadc)::value;
      int m = 0;
#pragma unroll
      for (; m < lead; ++m) mf(Fc, m);
#pragma unroll
      for (int t = 0; t < DVM; ++t) {
        __builtin_amdgcn_sched_barrier(0);
        piece(t, sd, bd);
        mf(Fc, m++);
        mf(Fc, m++);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < NDS; ++t) rd(Fn, t, br);
#pragma unroll
      for (; m < NMF; ++m) mf(Fc, m);
#pragma unroll
      for (int t = 0; t < NDS; ++t) {
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, NMF - lead - 2 * DVM - 2 * NDS, 0);
    };
    auto period = [&](int s, auto bc) __attribute__((always_inline)) {  // stages s (in F0) and s + 1; bc: s % 5
      constexpr int B = decltype(bc)::value;
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(0xC07F);
      vmcnt<DVM>();
      __builtin_amdgcn_s_barrier();
      half(F0, F1, s + 4, (B + 4) % NSTG, (B + 1) % NSTG, std::integral_constant<int, 1>{});
      half(F1, F0, s + 5, B, (B + 2) % NSTG, std::integral_constant<int, 0>{});
    };
#pragma unroll
    for (int t = 0; t < NSTG - 1; ++t)
#pragma unroll
      for (int u = 0; u < DVM; ++u) piece(u, t, t);
    vmcnt<DVM * 3>();
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int t = 0; t < NDS; ++t) rd(F0, t, 0);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    int s = 0;
    auto per = [&](auto bc) __attribute__((always_inline)) {
      period(s, bc);
      s += 2;
    };
    using std::integral_constant;
    // five periods are two laps of the ring: whole groups of five in the loop, then the 0..4
    // periods that are left, each behind a check of its own (one loop exit and plain if-thens:
    // with an exit between the unrolled periods the compiler copies all 128 accumulator
    // registers at every exit edge)
    int np = nst >> 1;
    for (; np >= 5; np -= 5) {
      per(integral_constant<int, 0>{});
      per(integral_constant<int, 2>{});
      per(integral_constant<int, 4>{});
      per(integral_constant<int, 1>{});
      per(integral_constant<int, 3>{});
    }
    if (np > 0) per(integral_constant<int, 0>{});
    if (np > 1) per(integral_constant<int, 2>{});
    if (np > 2) per(integral_constant<int, 4>{});
    if (np > 3) per(integral_constant<int, 1>{});
    if (s < nst) mfma_stage(F0);
  } else if constexpr (RING) {
#pragma unroll
    for (int t = 0; t < NSTG - 1; ++t) issue(t);
    static_assert(NSTG == 5 && DBUF, "the ring schedule is written for five buffers");
    vmcnt<DVM * 3>();  // stage 0 landed (1, 2, 3 in flight)
    __builtin_amdgcn_s_barrier();
    read_frags_b(F0, 0);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    // b: buffer of stage s (= s % 5, kept incrementally); F0 holds stage s's fragments
    auto ring = [](int b, int k) { return b + k >= NSTG ? b + k - NSTG : b + k; };
    auto period = [&](int s, int b) {
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(0xC07F);  // own reads of stages s - 1, s retired
      vmcnt<DVM>();                         // own DMA of stages <= s + 2 landed, s + 3 in flight
      __builtin_amdgcn_s_barrier();
      issue_b(s + 4, ring(b, 4));  // stage s - 1's buffer
      read_frags_b(F1, ring(b, 1));
      mfma_stage(F0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // an MFMA first: F0 is in registers
#pragma unroll
      for (int t = 0; t < DVM; ++t) {  // (DMA pieces two MFMAs apart, as dag.hip)
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      }
#pragma unroll
      for (int t = 0; t < NDS; ++t) {
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, NMF - 1 - 2 * DVM - 2 * NDS, 0);
      // second half, no barrier (stage s + 2 landed above) and one scheduling region with the first
      issue_b(s + 5, b);            // stage s's buffer
      read_frags_b(F0, ring(b, 2));
      mfma_stage(F1);
#pragma unroll
      for (int t = 0; t < DVM; ++t) {
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      }
#pragma unroll
      for (int t = 0; t < NDS; ++t) {
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, NMF - 2 * DVM - 2 * NDS, 0);
    };
    int s = 0, b = 0;
    for (; s + 1 < nst; s += 2, b = ring(b, 2)) period(s, b);
    if (s < nst) mfma_stage(F0);
  } else if (DBUF) {
#pragma unroll
    for (int t = 0; t < NSTG - 1; ++t) issue(t);
    vmcnt<DVM * (NSTG - 2)>();
    __builtin_amdgcn_s_barrier();
    read_frags(F0, 0);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    auto step = [&](int s, d2 (&Fc)[DNP][NF], d2 (&Fn)[DNP][NF]) {
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(0xC07F);
      vmcnt<DVM * (NSTG - 3)>();
      __builtin_amdgcn_s_barrier();
      issue(s + NSTG - 1);
      read_frags(Fn, s + 1);
      mfma_stage(Fc);
      sched();
    };
    int s = 0;
    for (; s + 1 < nst; s += 2) {
      step(s, F0, F1);
      step(s + 1, F1, F0);
    }
    if (s < nst) mfma_stage(F0);
  } else {
    // one fragment set: stage s's fragments read right after the barrier that makes it
    // complete (the other wave on the SIMD covers the LDS latency)
#pragma unroll
    for (int t = 0; t < NSTG - 1; ++t) issue(t);
    for (int s = 0; s < nst; ++s) {
      __builtin_amdgcn_sched_barrier(0);
      vmcnt<DVM * (NSTG - 2)>();
      __builtin_amdgcn_s_barrier();
      issue(s + NSTG - 1);
      read_frags(F0, s);
      mfma_stage(F0);
      sched();
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(0xC07F);  // own fragment reads of stage s done before the
    }                                       // next barrier frees the stage for re-fill
  }
  vmcnt<0>();
  __syncthreads();
  // the loop's clock: core-clock ticks per 100-MHz realtime tick, into a buffer of its own
  const unsigned long long ck1 = __builtin_amdgcn_s_memtime(), rt1 = __builtin_amdgcn_s_memrealtime();
  if (tid == 0) {
    clk[blockIdx.x * 2] = ck1 - ck0;
    clk[blockIdx.x * 2 + 1] = rt1 - rt0;
  }
  double t = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < RB; ++j) t += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
  out[blockIdx.x * 512 + tid] = t;
#endif
}

// Barrier-free variant: every wave DMAs its OWN operand rows (its 64 P rows and 64 Q rows)
// into a private LDS region, so a wave waits only for its own DMA (vmcnt) and never for the
// other waves (no s_barrier in the loop); each P / Q row is fetched by two waves (L2 hits).
// PK-deep stages (8: 4 chunks per row, swizzle (row >> 2) & 3; 16: 8 chunks, (row >> 1) & 7),
// NSTG stages, next stage's fragments prefetched into a second register set.
template <int PK, int NSTG>
__global__ __launch_bounds__(256, 1) void accum_priv_kernel(const double* __restrict__ M, size_t ld,
                                                           int ncolblk, int nst, int mode,
                                                           double* out) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NCH = PK / 2;              // 16-B chunks per LDS row
  constexpr int RPD = 64 / NCH;            // rows per wave-wide 1-KB DMA
  constexpr int ND = 64 / RPD;             // DMA per operand per wave per stage
  constexpr int WSTAGE = 2 * 64 * PK;      // doubles per wave per stage (P rows, then Q rows)
  constexpr int DNP = PK / 8;              // fragment blocks (2 k-steps each) per stage
  constexpr int DVM = 2 * ND;
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w & 1, wn = w >> 1;
  const int b = blockIdx.x;
  const int np_ = ncolblk - 2;
  const int pp = mode ? (b / 32) % np_ : 0, qp = mode ? 1 + (b % np_) : 1;
  const double* P = M + (size_t)pp * DT * ld + (size_t)wm * 64 * ld;
  const double* Q = M + (size_t)qp * DT * ld + (size_t)wn * 64 * ld;
  auto sw = [](int row) { return PK == 8 ? ((row >> 2) & 3) : ((row >> 1) & 7); };
  d4v acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %1, 0" : "=a"(acc[i][j]) : "v"(0.0));
  const double* srcP[ND];
  const double* srcQ[ND];
#pragma unroll
  for (int r = 0; r < ND; ++r) {
    const int row = RPD * r + lane / NCH;
    const int c = (lane % NCH) ^ sw(row);
    srcP[r] = P + 2 * c + (size_t)row * ld;
    srcQ[r] = Q + 2 * c + (size_t)row * ld;
  }
  double* mine = lds + w * WSTAGE;
  auto issue = [&](int s) {
    double* base = mine + (s % NSTG) * 4 * WSTAGE;
    const size_t ko = (size_t)min(s, nst - 1) * PK;
#pragma unroll
    for (int r = 0; r < ND; ++r) {
      __builtin_amdgcn_global_load_lds(srcP[r] + ko, base + r * 128, 16, 0, 0);
      __builtin_amdgcn_global_load_lds(srcQ[r] + ko, base + 64 * PK + r * 128, 16, 0, 0);
    }
  };
  auto read_frags = [&](d2 (&F)[DNP][8], int s) {
    const double* ps = mine + (s % NSTG) * 4 * WSTAGE;
    const double* qs = ps + 64 * PK;
#pragma unroll
    for (int p = 0; p < DNP; ++p) {
      const int ch = (lane >> 4) + 4 * p;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = i * 16 + (lane & 15);
        F[p][i] = *reinterpret_cast<const d2*>(&qs[row * PK + 2 * (ch ^ sw(row))]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = j * 16 + (lane & 15);
        F[p][4 + j] = *reinterpret_cast<const d2*>(&ps[row * PK + 2 * (ch ^ sw(row))]);
      }
    }
  };
  auto mfma_stage = [&](const d2 (&F)[DNP][8]) {
#pragma unroll
    for (int p = 0; p < DNP; ++p)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(F[p][i][h], F[p][4 + j][h], acc[i][j], 0, 0, 0);
  };
  auto step = [&](int s, d2 (&Fc)[DNP][8], d2 (&Fn)[DNP][8]) {
    __builtin_amdgcn_sched_barrier(0);
    // stage s - 1's buffer: its fragments were read (and waited for) a step ago
    issue(s + NSTG - 1);
    vmcnt<DVM * (NSTG - 2)>();  // own DMA of stage s + 1 landed (s + 2 .. s + NSTG - 1 in flight)
    read_frags(Fn, s + 1);
    mfma_stage(Fc);
#pragma unroll
    for (int t = 0; t < 8 * DNP; ++t) {
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // MFMA
    }
    __builtin_amdgcn_sched_group_barrier(0x008, 32 * DNP - 16 * DNP, 0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): Fn in registers before the next issue
  };
  d2 F0[DNP][8], F1[DNP][8];
#pragma unroll
  for (int t = 0; t < NSTG - 1; ++t) issue(t);
  vmcnt<DVM * (NSTG - 2)>();
  read_frags(F0, 0);
  __builtin_amdgcn_s_waitcnt(0xC07F);
  int s = 0;
  for (; s + 1 < nst; s += 2) {
    step(s, F0, F1);
    step(s + 1, F1, F0);
  }
  if (s < nst) mfma_stage(F0);
  vmcnt<0>();
  double t = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) t += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
  out[blockIdx.x * 512 + tid] = t;
#endif
}

template <int PK, int NSTG>
void run_priv(const double* M, size_t ld, int ncolblk, int K, int reps, int mode, double* out, int cus) {
  constexpr size_t lds = sizeof(double) * NSTG * 4 * 2 * 64 * PK;
  if (hipFuncSetAttribute((const void*)accum_priv_kernel<PK, NSTG>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    printf("priv PK=%d NSTG=%d: cannot set %zu B of LDS\n", PK, NSTG, lds);
    return;
  }
  const int nst = K / PK;
  hipLaunchKernelGGL((accum_priv_kernel<PK, NSTG>), dim3(cus), dim3(256), lds, 0, M, ld, ncolblk, 8, mode, out);
  hipError_t le = hipGetLastError();
  if (le == hipSuccess) le = hipDeviceSynchronize();
  if (le != hipSuccess) {
    printf("priv PK=%d NSTG=%d: launch failed: %s\n", PK, NSTG, hipGetErrorString(le));
    return;
  }
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  (void)hipEventRecord(e0);
  for (int r = 0; r < reps; ++r)
    hipLaunchKernelGGL((accum_priv_kernel<PK, NSTG>), dim3(cus), dim3(256), lds, 0, M, ld, ncolblk, nst, mode, out);
  (void)hipEventRecord(e1);
  (void)hipEventSynchronize(e1);
  float ms;
  (void)hipEventElapsedTime(&ms, e0, e1);
  const double flops = 2.0 * DT * DT * (double)nst * PK * cus * reps;
  printf("%s private-buffer 128x128, 4 waves, %2d-deep x %d stages (%3zu KB), no barrier: "
         "%.2f TFLOP/s = %.4f per CU (%.3f ms per launch)\n", mode ? "dag-like" : "hot     ",
         PK, NSTG, lds / 1024, flops / ms / 1e9, flops / ms / 1e9 / cus, ms / reps);
}

__global__ void fill_kernel(double* M, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    M[i] = (double)((i * 2654435761u) % 1000) * 1e-3;
}

static double g_warm_s = 0.0;  // back-to-back launches before the timed ones (seconds)

template <int TMR, int NW, int NSTG, bool DBUF, bool RING = false, bool SBASE = false>
void run(const double* M, size_t ld, int ncolblk, int K, int reps, int mode, double* out, int cus) {
  constexpr size_t lds = sizeof(double) * NSTG * (DT * TMR + DT) * DTK;
  auto kern = accum_kernel<TMR, NW, NSTG, DBUF, RING, SBASE>;
  unsigned long long* clk = nullptr;
  if (hipMalloc(&clk, sizeof(unsigned long long) * 2 * cus) != hipSuccess) return;
  if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess) {
    printf("TMR=%d NW=%d NSTG=%d: cannot set %zu B of LDS\n", TMR, NW, NSTG, lds);
    return;
  }
  const int nst = K / DTK;
  hipLaunchKernelGGL(kern, dim3(cus), dim3(NW * 64), lds, 0, M, ld, ncolblk, 8, mode, out, clk);
  hipError_t le = hipGetLastError();
  if (le == hipSuccess) le = hipDeviceSynchronize();
  if (le != hipSuccess) {
    printf("TMR=%d NW=%d NSTG=%d: launch failed: %s\n", TMR, NW, NSTG, hipGetErrorString(le));
    return;
  }
  // warm-up: batches of 8 launches, at most two batches queued, until g_warm_s has passed
  if (g_warm_s > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    hipEvent_t eb[2];
    (void)hipEventCreate(&eb[0]);
    (void)hipEventCreate(&eb[1]);
    for (int it = 0; std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < g_warm_s; ++it) {
      if (it >= 2 && hipEventSynchronize(eb[it & 1]) != hipSuccess) return;
      for (int r = 0; r < 8; ++r)
        hipLaunchKernelGGL(kern, dim3(cus), dim3(NW * 64), lds, 0, M, ld, ncolblk, nst, mode, out, clk);
      (void)hipEventRecord(eb[it & 1]);
    }
  }
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  (void)hipEventRecord(e0);
  for (int r = 0; r < reps; ++r)
    hipLaunchKernelGGL(kern, dim3(cus), dim3(NW * 64), lds, 0, M, ld, ncolblk, nst, mode, out, clk);
  (void)hipEventRecord(e1);
  if (hipEventSynchronize(e1) != hipSuccess) {
    printf("TMR=%d NW=%d NSTG=%d: timed launches failed\n", TMR, NW, NSTG);
    return;
  }
  float ms;
  (void)hipEventElapsedTime(&ms, e0, e1);
  std::vector<unsigned long long> hc(2 * (size_t)cus);
  (void)hipMemcpy(hc.data(), clk, sizeof(unsigned long long) * hc.size(), hipMemcpyDeviceToHost);
  std::vector<double> ghz(cus);
  for (int c = 0; c < cus; ++c) ghz[c] = hc[2 * c + 1] ? 0.1 * (double)hc[2 * c] / (double)hc[2 * c + 1] : 0.0;
  std::sort(ghz.begin(), ghz.end());
  // (the sums of the last launch: equal, bit for bit, between configs of one MFMA order)
  std::vector<double> ho((size_t)cus * 512);
  (void)hipMemcpy(ho.data(), out, sizeof(double) * ho.size(), hipMemcpyDeviceToHost);
  double chk = 0;
  for (int c = 0; c < cus; ++c)
    for (int t = 0; t < NW * 64; ++t) chk += ho[(size_t)c * 512 + t];
  printf("checksum %.17g\n", chk);
  const double flops = 2.0 * DT * TMR * DT * (double)nst * DTK * cus * reps;
  const double bytes = 8.0 * (DT * TMR + DT) * (double)nst * DTK * cus * reps;
  printf("%s tile %3dx128, %d waves, %d stages (%3zu KB), %s fragments%s: %.2f TFLOP/s = %.4f per CU, "
         "%.1f flop/B, operand stream %.2f TB/s (%.3f ms per launch), in-kernel clock %.3f GHz "
         "(median of %d workgroups, after %.1f s of launches)\n",
         mode == 1 ? "dag-like" : mode == 2 ? "L2-held " : mode == 3 ? "own-panel" : "hot     ",
         DT * TMR, NW, NSTG, lds / 1024, DBUF ? "2-set" : "1-set",
         SBASE ? ", one barrier per two stages, scalar-addressed" : RING ? ", one barrier per two stages" : "", flops / ms / 1e9,
         flops / ms / 1e9 / cus, flops / bytes, bytes / ms / 1e9, ms / reps, ghz[cus / 2], cus, g_warm_s);
  (void)hipFree(clk);
}

int main(int argc, char** argv) {
  const int K = argc > 1 ? atoi(argv[1]) : 16384;
  const int reps = argc > 2 ? atoi(argv[2]) : 5;
  hipDeviceProp_t p;
  (void)hipGetDeviceProperties(&p, 0);
  const int cus = p.multiProcessorCount;
  const int cfg = argc > 3 ? atoi(argv[3]) : 0;
  const int mode = argc > 4 ? atoi(argv[4]) : 0;
  // 64 panels of 128 columns, K deep; mode 3: a Q panel per workgroup behind the P panels (at
  // K = 32768 about 9 GB, so that every launch streams its operands from HBM)
  const int ncolblk = mode == 3 ? cus + 9 : 64;
  const size_t ld = K, ncols = (size_t)ncolblk * DT;
  double *M, *out;
  if (hipMalloc(&M, sizeof(double) * ld * ncols) != hipSuccess ||
      hipMalloc(&out, sizeof(double) * cus * 512) != hipSuccess) {
    printf("cannot allocate %zu MB\n", sizeof(double) * ld * ncols >> 20);
    return 1;
  }
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, M, ld * ncols);
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  g_warm_s = argc > 5 ? atof(argv[5]) : 0.0;
  printf("K = %d, %d CUs, %d reps, config %d\n", K, cus, reps, cfg);
  switch (cfg) {
    case 0: run<1, 4, 4, true>(M, ld, ncolblk, K, reps, mode, out, cus); break;   // today's dag_accum
    case 1: run<2, 4, 3, false>(M, ld, ncolblk, K, reps, mode, out, cus); break;  // 256 x 128, 1 wave/SIMD
    case 2: run<2, 8, 3, false>(M, ld, ncolblk, K, reps, mode, out, cus); break;  // 256 x 128, 2 waves/SIMD
    case 3: run<1, 4, 4, false>(M, ld, ncolblk, K, reps, mode, out, cus); break;
    case 4: run_priv<8, 4>(M, ld, ncolblk, K, reps, mode, out, cus); break;   // 128 KB
    case 5: run_priv<8, 5>(M, ld, ncolblk, K, reps, mode, out, cus); break;   // 160 KB
    case 6: run_priv<16, 2>(M, ld, ncolblk, K, reps, mode, out, cus); break;  // 128 KB
    case 7: run<1, 8, 4, true>(M, ld, ncolblk, K, reps, mode, out, cus); break;   // 128 x 128, 2 waves/SIMD (32 x 64 each)
    case 8: run<1, 8, 4, false>(M, ld, ncolblk, K, reps, mode, out, cus); break;
    case 9: run<1, 4, 5, true, true>(M, ld, ncolblk, K, reps, mode, out, cus); break;  // ring of 5, barrier per 2 stages
    case 10: run<1, 4, 5, true, true, true>(M, ld, ncolblk, K, reps, mode, out, cus); break;  // + scalar-addressed (dag_accum)
  }
  return 0;
}
