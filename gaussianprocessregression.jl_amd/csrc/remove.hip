// gpr_fit_remove: take r observations out of a fitted model without refactoring it.
//
// The fitted buffer holds U above the diagonal (K = U^T U) and K strictly below.  With D the removed
// indices, `keep` the others in ascending order, T = U[keep, keep] (upper triangular) and
// W = U[D, keep] (W[s, j'] = 0 wherever keep[j'] < p_s: the buffer holds K there, so those entries
// are masked, never used), K[keep, keep] = T^T T + W^T W: the new factor is T after a rank-r
// positive update, done with Givens rotations.  For each row i' of T in ascending order and each s
// in ascending order: rho = hypot(T[i',i'], W[s,i']), c = T[i',i'] / rho, sg = W[s,i'] / rho, and for
// every j' >= i' the pair (t, w) = (T[i',j'], W[s,j']) becomes (c t + sg w, -sg t + c w).  No pivot
// can fail and no kernel function is evaluated.
//
// Out of place: the compacted strict lower triangle and the upper rows above the first touched
// 128-row block are a streaming gather (remove_gather_kernel); the update works in blocks of 128
// columns in NEW coordinates, RM_R removed points (a group) at a time: the first group reads
// dK through `keep` and writes dKout, further groups update dKout in place (a block column is read
// and written by its owner only) with their W rows from the untouched dK.  Order: groups ascending,
// s ascending within a row -- any grouping gives a valid factor, this one is fixed.
//
// Two routes, the same device functions on every element, so they agree bit for bit:
//   route 0  per 128-row block a one diagonal launch (generates block a's rotations) and one panel
//            launch (applies them to the tiles (a, b > a)), ordered by the stream; W between
//            launches lives in a workspace.
//   route 1  one persistent launch per group: one workgroup per column block b, handed out by an
//            atomic ticket, keeps W_b in registers and walks the tiles a = a0 .. b of its column;
//            block a's rotations come through sweep_handoff.hpp (sc1 stores -> vmcnt(0) drain ->
//            barrier -> sc1 counter store; every wave polls for itself, then loads with sc1 loads),
//            tile a + 1 is requested before the wait on block a.  145 KB of LDS per workgroup keep
//            a second workgroup off the CU (the hand-off table's one-workgroup-per-CU cell).
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "sweep_handoff.hpp"

namespace {

// RM_R: removed points per pass.  A thread owns one column: RM_R doubles of W, the 128 doubles of the
// prefetched tile column and a row's running value -- about 300 VGPRs of the 512 a wave has at
// 128 threads per CU; the rotations of a block are RM_R x 128 (c, sg) pairs = 16 KB beside the
// 129-KB tile in LDS.  16 would need 32 KB of rotations: past the 160 KB of LDS.
constexpr int RM_NB = 128, RM_R = 8, RM_THREADS = 128, RM_P = 129;
constexpr int RM_ROT = RM_NB * RM_R * 2;                      // doubles per block of rotations
constexpr size_t RM_LDS = (size_t)(RM_NB * RM_P + RM_ROT) * sizeof(double);

// new index -> index in the source matrix (keep == nullptr: the matrix is already compacted)
__device__ __forceinline__ int rm_src(const int* keep, int i) { return keep ? keep[i] : i; }

// tile (a, b) of the source in NEW coordinates: thread tid takes row a 128 + tid (coalesced along
// the column-major contiguous direction) of each of the 128 columns; rows and columns beyond np
// are clamped to np - 1 (valid addresses, values never stored)
__device__ __forceinline__ void rm_load_tile(double (&v)[RM_NB], const double* A, size_t ld,
                                             const int* keep, int np, int a, int b, int tid) {
  const size_t row = (size_t)rm_src(keep, min(a * RM_NB + tid, np - 1));
#pragma unroll
  for (int k = 0; k < RM_NB; ++k) {
    const size_t col = (size_t)rm_src(keep, min(b * RM_NB + k, np - 1));
    v[k] = A[row + col * ld];
  }
}

__device__ __forceinline__ void rm_stage_tile(double* tile, const double (&v)[RM_NB], int tid) {
#pragma unroll
  for (int k = 0; k < RM_NB; ++k) tile[tid + k * RM_P] = v[k];
}

// rows <= np of tile (a, b), on and above the diagonal, columns < kb, from LDS to Out
__device__ __forceinline__ void rm_store_tile(const double* tile, double* Out, size_t ldo, int np,
                                              int a, int b, int kb, int tid) {
  const int i = a * RM_NB + tid;
  if (i >= np) return;
  double* o = Out + (size_t)i + (size_t)b * RM_NB * ldo;
  for (int k = (a == b ? tid : 0); k < kb; ++k) o[(size_t)k * ldo] = tile[tid + k * RM_P];
}

typedef double r2v __attribute__((ext_vector_type(2)));

// A group of removed points: rs of them, q[s] the NEW position of the first kept point behind point s
// (ascending).  Row i' meets point s only from i' = q[s] on (W[s, i'] = 0 before: c = 1, sg = 0), so row
// block a needs the first ns(a) = #{s : q[s] < 128 (a + 1)} rotations per row only.  The kernels run
// NS(a) = ns(a) rounded up to 1, 2, 4 or 8 of them without a branch -- the slots beyond are exact
// identities (w = 0 selects c = 1, sg = 0; c t + 0 w = t and c w - 0 t = w bit for bit) -- and the
// producer and the consumers of block a's rotations use the same NS(a).
struct RmGroup {
  int rs;
  int q[RM_R];
};
__device__ __forceinline__ int rm_ns(const RmGroup& g, int a) {
  int ns = 0;
#pragma unroll
  for (int s = 0; s < RM_R; ++s) ns += (s < g.rs && g.q[s] < (a + 1) * RM_NB) ? 1 : 0;
  return ns <= 1 ? 1 : ns <= 2 ? 2 : ns <= 4 ? 4 : 8;
}

// one row's NS rotations, in order, on one column's pair (t, w); rr: that row's (c, sg) pairs in LDS
template <int NS>
__device__ __forceinline__ void rm_rotate(double& t, double (&w)[RM_R], const double* __restrict__ rr) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const r2v cs = *reinterpret_cast<const r2v*>(rr + 2 * s);
    const double tn = fma(cs.x, t, cs.y * w[s]);
    w[s] = fma(cs.x, w[s], -(cs.y * t));
    t = tn;
  }
}

// an off-diagonal tile: block a's 128 x NS rotations on column j of the tile and of W, four rows at
// a time (the rows chain through w[s], a row's rotations through t: the four rows' steps overlap)
template <int NS>
__device__ __forceinline__ void rm_apply_tile(double* __restrict__ tile, const double* __restrict__ rot,
                                              double (&w)[RM_R], int j) {
  double* col = tile + j * RM_P;
  for (int i0 = 0; i0 < RM_NB; i0 += 4) {
    double t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = col[i0 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) rm_rotate<NS>(t[k], w, rot + (i0 + k) * RM_R * 2);
#pragma unroll
    for (int k = 0; k < 4; ++k) col[i0 + k] = t[k];
  }
}

// the diagonal tile: row by row the owner of column i generates that row's rotations from its
// (t, w) -- rho_s^2 = t^2 + sum_{k <= s} w_k^2, c_s = rho_{s-1} / rho_s, sg_s = w_s / rho_s with
// 1 / rho_s one reciprocal square root, so the NS of them do not wait for one another -- and columns
// j >= i apply them.  The next row's entry is read before the barrier: row i does not change it.
template <int NS>
__device__ __forceinline__ void rm_diag_tile(double* __restrict__ tile, double* __restrict__ rot,
                                             double (&w)[RM_R], int j, int kb) {
  double* col = tile + j * RM_P;
  double tn = col[0];
  for (int i = 0; i < kb; ++i) {
    double t = tn;
    tn = col[min(i + 1, RM_NB - 1)];
    double* rr = rot + i * RM_R * 2;
    if (j == i) {
      double prev = t, q = t * t;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const double wv = w[s];
        q = fma(wv, wv, q);
        const double inv = rsqrt(q);
        const bool on = wv != 0.0;
        r2v cs;
        cs.x = on ? prev * inv : 1.0;
        cs.y = on ? wv * inv : 0.0;
        prev = on ? q * inv : prev;
        *reinterpret_cast<r2v*>(rr + 2 * s) = cs;
      }
    }
    __syncthreads();
    if (j >= i) {
      rm_rotate<NS>(t, w, rr);
      col[i] = t;
    }
  }
}

// the two, on the NS of row block a
__device__ __forceinline__ void rm_tile(bool diag, int ns, double* tile, double* rot,
                                        double (&w)[RM_R], int j, int kb) {
  if (diag) {
    if (ns == 1) rm_diag_tile<1>(tile, rot, w, j, kb);
    else if (ns == 2) rm_diag_tile<2>(tile, rot, w, j, kb);
    else if (ns == 4) rm_diag_tile<4>(tile, rot, w, j, kb);
    else rm_diag_tile<8>(tile, rot, w, j, kb);
  } else {
    if (ns == 1) rm_apply_tile<1>(tile, rot, w, j);
    else if (ns == 2) rm_apply_tile<2>(tile, rot, w, j);
    else if (ns == 4) rm_apply_tile<4>(tile, rot, w, j);
    else rm_apply_tile<8>(tile, rot, w, j);
  }
}

// column c0 + j of the group's W (RM_R rows of np doubles, masked when it was filled)
__device__ __forceinline__ void rm_load_w(double (&w)[RM_R], const double* wbuf, int np, int col,
                                          int rs) {
#pragma unroll
  for (int s = 0; s < RM_R; ++s) w[s] = s < rs ? wbuf[(size_t)s * np + col] : 0.0;
}

// ---- route 1: the sweep ---------------------------------------------------------------------------
// sync[0] = ticket, sync[1] = blocks done (block a0 + k is published once sync[1] > k); both zeroed
// before the launch.  hand: RM_ROT doubles per block, indexed by the block.
__global__ __launch_bounds__(RM_THREADS) void remove_sweep_kernel(
    const double* A, size_t ld, const int* keep, double* Out, size_t ldo, int np, int a0, RmGroup g,
    const double* __restrict__ wbuf, double* hand, int* sync) {
  extern __shared__ double rm_lds[];
  __shared__ int sblk;
  double* tile = rm_lds;
  double* rot = rm_lds + RM_NB * RM_P;
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid == 0) sblk = atomicAdd(&sync[0], 1);
  __syncthreads();
  const int b = a0 + sblk, nblk = (np + RM_NB - 1) / RM_NB;
  const int c0 = b * RM_NB, kb = min(RM_NB, np - c0);
  double w[RM_R], v[RM_NB];
  rm_load_w(w, wbuf, np, min(c0 + tid, np - 1), g.rs);
  rm_load_tile(v, A, ld, keep, np, a0, b, tid);
  int known = 0;
  for (int a = a0; a <= b; ++a) {
    rm_stage_tile(tile, v, tid);
    if (a < b) {
      rm_load_tile(v, A, ld, keep, np, a + 1, b, tid);  // requested before the wait
      sweep_wait(sync, a - a0 + 1, known, lane);
      const double* h = hand + (size_t)a * RM_ROT;
#pragma unroll
      for (int t = 0; t < RM_ROT / RM_THREADS; ++t)
        rot[tid + t * RM_THREADS] = hand_ld(h + tid + t * RM_THREADS);
      __syncthreads();
      rm_tile(false, rm_ns(g, a), tile, rot, w, tid, kb);
      __syncthreads();
    } else {
      __syncthreads();
      rm_tile(true, rm_ns(g, a), tile, rot, w, tid, kb);
      __syncthreads();
      if (b + 1 < nblk) {  // (a full block: every rotation slot was written)
        double* h = hand + (size_t)b * RM_ROT;
#pragma unroll
        for (int t = 0; t < RM_ROT / RM_THREADS; ++t)
          hand_st(h + tid + t * RM_THREADS, rot[tid + t * RM_THREADS]);
        sweep_publish(sync, b - a0 + 1);
      }
    }
    rm_store_tile(tile, Out, ldo, np, a, b, kb, tid);
    __syncthreads();
  }
}

// ---- route 0: one launch per step -------------------------------------------------------------------
// DIAG: tile (a, a), generates rotbuf[a].  Otherwise tile (a, a + 1 + blockIdx.x), applies
// rotbuf[a]; W goes back to the workspace for the next row block's launch.
template <bool DIAG>
__global__ __launch_bounds__(RM_THREADS) void remove_step_kernel(
    const double* A, size_t ld, const int* keep, double* Out, size_t ldo, int np, int a, RmGroup g,
    double* wbuf, double* rotbuf) {
  extern __shared__ double rm_lds[];
  double* tile = rm_lds;
  double* rot = rm_lds + RM_NB * RM_P;
  const int tid = threadIdx.x;
  const int b = DIAG ? a : a + 1 + (int)blockIdx.x;
  const int c0 = b * RM_NB, kb = min(RM_NB, np - c0);
  double w[RM_R], v[RM_NB];
  rm_load_w(w, wbuf, np, min(c0 + tid, np - 1), g.rs);
  rm_load_tile(v, A, ld, keep, np, a, b, tid);
  rm_stage_tile(tile, v, tid);
  double* gr = rotbuf + (size_t)a * RM_ROT;
  if (DIAG) {
    __syncthreads();
    rm_tile(true, rm_ns(g, a), tile, rot, w, tid, kb);
    __syncthreads();
    if (kb == RM_NB)
      for (int t = 0; t < RM_ROT / RM_THREADS; ++t)
        gr[tid + t * RM_THREADS] = rot[tid + t * RM_THREADS];
  } else {
    for (int t = 0; t < RM_ROT / RM_THREADS; ++t)
      rot[tid + t * RM_THREADS] = gr[tid + t * RM_THREADS];
    __syncthreads();
    rm_tile(false, rm_ns(g, a), tile, rot, w, tid, kb);
    __syncthreads();
    if (tid < kb)
      for (int s = 0; s < g.rs; ++s) wbuf[(size_t)s * np + c0 + tid] = w[s];
  }
  rm_store_tile(tile, Out, ldo, np, a, b, kb, tid);
}

// ---- the kernels around them ----------------------------------------------------------------------
// Out[i', j'] = K[keep[i'], keep[j']] for the strict lower triangle (i' > j') and for the upper
// rows i' < rowlim that no rotation touches; a thread per row, 16 columns per workgroup
constexpr int RG_ROWS = 256, RG_COLS = 16;
__global__ __launch_bounds__(RG_ROWS) void remove_gather_kernel(
    const double* __restrict__ K, size_t ldk, const int* __restrict__ keep, int np, int rowlim,
    double* __restrict__ Out, size_t ldo) {
  const int i0 = blockIdx.x * RG_ROWS, j0 = blockIdx.y * RG_COLS;
  if (i0 >= rowlim && i0 + RG_ROWS - 1 <= j0) return;  // wholly in the update's part
  const int i = i0 + threadIdx.x;
  if (i >= np) return;
  const size_t si = (size_t)keep[i];
  const int j1 = min(np, j0 + RG_COLS);
  for (int j = j0; j < j1; ++j)
    if (i > j || i < rowlim) Out[(size_t)i + (size_t)j * ldo] = K[si + (size_t)keep[j] * ldk];
}

// wbuf[s, j'] = U[p_s, keep[j']] where keep[j'] > p_s, else 0 (below the diagonal the buffer holds
// K: selected after the load, the address is valid either way).  A row of a column-major matrix:
// one 8-B word per column, 8 rs np bytes in all.
__global__ __launch_bounds__(256) void remove_w_kernel(const double* __restrict__ K, size_t ldk,
                                                       const int* __restrict__ keep, int np,
                                                       const int* __restrict__ idx, int rs,
                                                       double* __restrict__ wbuf) {
  const int j = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (j >= np || s >= rs) return;
  const int p = idx[s], col = keep[j];
  const double v = K[(size_t)p + (size_t)col * ldk];
  wbuf[(size_t)s * np + j] = col > p ? v : 0.0;
}

}  // namespace

extern "C" {

int gpr_fit_remove(gpr_ctx_t ctx, const double* dK, int n0, int ldk, const int* idx, int r,
                   const double* dy, int nrhs, int ldy, double* dKout, int ldo, double* dalpha) {
  if (r < 1) return set_err(ctx, GPR_E_ARG, "r=%d (needs r >= 1)", r);
  if (r >= n0) return set_err(ctx, GPR_E_ARG, "r=%d >= n0=%d (cannot remove every point)", r, n0);
  const int np = n0 - r;
  if (nrhs < 1) return set_err(ctx, GPR_E_ARG, "nrhs=%d (needs nrhs >= 1)", nrhs);
  if (ldk < n0) return set_err(ctx, GPR_E_ARG, "ldk=%d < n0=%d", ldk, n0);
  if (ldo < np) return set_err(ctx, GPR_E_ARG, "ldo=%d < n0 - r=%d", ldo, np);
  if (ldy < np) return set_err(ctx, GPR_E_ARG, "ldy=%d < n0 - r=%d", ldy, np);
  if (!dK || !idx || !dy || !dKout || !dalpha)
    return set_err(ctx, GPR_E_ARG, "%s is NULL",
                   !dK ? "dK" : !idx ? "idx" : !dy ? "dy" : !dKout ? "dKout" : "dalpha");
  for (int s = 0; s < r; ++s) {
    if (idx[s] < 0 || idx[s] >= n0)
      return set_err(ctx, GPR_E_ARG, "idx[%d]=%d outside [0, n0=%d)", s, idx[s], n0);
    if (s > 0 && idx[s] <= idx[s - 1])
      return set_err(ctx, GPR_E_ARG, "idx not strictly ascending at idx[%d]=%d", s, idx[s]);
  }
  {
    const double* k1 = dK + (size_t)(n0 - 1) * ldk + n0;
    const double* o1 = dKout + (size_t)(np - 1) * ldo + np;
    if (dKout < k1 && dK < o1) return set_err(ctx, GPR_E_ARG, "dKout overlaps dK");
  }
  static const hipError_t lds_ok = [] {  // 145 KB of dynamic LDS: above the default launch limit
    const auto bytes = (int)RM_LDS;
    const auto attr = hipFuncAttributeMaxDynamicSharedMemorySize;
    hipError_t e = hipFuncSetAttribute((const void*)remove_sweep_kernel, attr, bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)remove_step_kernel<true>, attr, bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)remove_step_kernel<false>, attr, bytes);
    return e;
  }();
  HIP_TRY(ctx, lds_ok);
  hipStream_t st = ctx->stream;
  ctx->ls = st;
  const int nblk = (np + RM_NB - 1) / RM_NB;

  // keep[] and idx[] on the device, behind the group's W rows
  std::vector<int> hk((size_t)np + r);
  for (int i = 0, s = 0, o = 0; i < n0; ++i) {
    if (s < r && idx[s] == i) ++s;
    else hk[o++] = i;
  }
  std::copy(idx, idx + r, hk.begin() + np);
  const size_t wdoubles = (size_t)RM_R * np;
  GPR_TRY(ensure_buf(ctx, ctx->drmw, wdoubles + (hk.size() + 1) / 2));
  GPR_TRY(ensure_buf(ctx, ctx->dahand, (size_t)nblk * RM_ROT));
  double* wbuf = ctx->drmw;
  int* dkeep = reinterpret_cast<int*>(ctx->drmw + wdoubles);
  const int* didx = dkeep + np;
  HIP_TRY(ctx, hipMemcpyAsync(dkeep, hk.data(), hk.size() * sizeof(int), hipMemcpyHostToDevice, st));

  // dKout receives a new factor: whatever the context cached for that buffer is stale
  ctx->fc.factor_forget();

  const int rowlim = std::min(nblk, idx[0] / RM_NB) * RM_NB;
  {
    TimerScope ts(ctx, TC_OTHER, 0.0);
    remove_gather_kernel<<<dim3((np + RG_ROWS - 1) / RG_ROWS, (np + RG_COLS - 1) / RG_COLS),
                           RG_ROWS, 0, st>>>(dK, (size_t)ldk, dkeep, np, rowlim, dKout,
                                             (size_t)ldo);
    LAUNCH_CHECK(ctx);
  }
  // GPR_REMOVE_SWEEP auto: the launch chain, which measured faster at every case of bench_remove.py
  // (profiles/r17_bench_remove.json; n0 = 32768, ms per update, sweep vs chain): r = 1 oldest 19.1 vs
  // 16.1, r = 1 middle 9.5 vs 7.9, r = 8 34.2 vs 27.4, r = 16 60.3 vs 47.1, r = 128 427 vs 316 -- a hop
  // of the sweep carries the store of the tile above the diagonal and the drain before the publish
  const bool sweep = ctx->remove_sweep > 0;
  int* sync = ctx->dinfo + INFO_SKINNY;
  {
    TimerScope ts(ctx, TC_REMOVE_UPDATE, 0.0);
    for (int s0 = 0; s0 < r; s0 += RM_R) {
      const int rs = std::min(RM_R, r - s0);
      const int a0 = (idx[s0] - s0) / RM_NB;  // the first row block this group's rotations touch
      if (a0 >= nblk) break;                  // only the newest points are left: copied already
      remove_w_kernel<<<dim3((np + 255) / 256, rs), 256, 0, st>>>(dK, (size_t)ldk, dkeep, np,
                                                                 didx + s0, rs, wbuf);
      LAUNCH_CHECK(ctx);
      const double* A = s0 == 0 ? dK : dKout;
      const size_t ld = s0 == 0 ? (size_t)ldk : (size_t)ldo;
      const int* keep = s0 == 0 ? dkeep : nullptr;
      RmGroup g{};
      g.rs = rs;
      for (int s = 0; s < rs; ++s) g.q[s] = idx[s0 + s] - (s0 + s);
      if (sweep) {
        HIP_TRY(ctx, hipMemsetAsync(sync, 0, INFO_SKINNY_N * sizeof(int), st));
        remove_sweep_kernel<<<nblk - a0, RM_THREADS, RM_LDS, st>>>(
            A, ld, keep, dKout, (size_t)ldo, np, a0, g, wbuf, ctx->dahand, sync);
        LAUNCH_CHECK(ctx);
      } else {
        for (int a = a0; a < nblk; ++a) {
          remove_step_kernel<true><<<1, RM_THREADS, RM_LDS, st>>>(
              A, ld, keep, dKout, (size_t)ldo, np, a, g, wbuf, ctx->dahand);
          LAUNCH_CHECK(ctx);
          if (a + 1 == nblk) break;
          remove_step_kernel<false><<<nblk - 1 - a, RM_THREADS, RM_LDS, st>>>(
              A, ld, keep, dKout, (size_t)ldo, np, a, g, wbuf, ctx->dahand);
          LAUNCH_CHECK(ctx);
        }
      }
    }
  }
  // alpha' = K'^{-1} y by the two sweeps on the new factor (which establish the factor cache)
  GPR_TRY(copy_columns(ctx, dalpha, np, dy, ldy, nrhs));
  GPR_TRY(potrs_core(ctx, dKout, np, ldo, dalpha, nrhs, np));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"
