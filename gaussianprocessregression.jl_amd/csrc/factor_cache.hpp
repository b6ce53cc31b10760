// What a context remembers about the caller's matrices, keyed on their device pointers.  Pure
// bookkeeping: no HIP call and no gpr_ctx, so the rules are checked on the CPU
// (tests/host/factor_cache_check.cpp).  Nothing outside this struct touches the fields.
#pragma once
#include <cstddef>
#include <cstdint>

struct FactorCache {
  // ---- U_bb^{-1} of the diagonal blocks of a factor, in gpr_ctx::winv (one nb x nb slot each) --
  void factor_adopt(const double* U, int n, int ld, int nb) {
    fac_ptr = U; fac_n = n; fac_ld = ld; fac_nb = nb;
  }
  bool factor_known(const double* U, int n, int ld, int nb) const {
    return fac_ptr && fac_ptr == U && fac_n == n && fac_ld == ld && fac_nb == nb;
  }
  // ---- U_sq^{-1} of its outer panel squares, in gpr_ctx::dsqinv (one nb2 x nb2 slot each) -----
  void sq_adopt(const double* U, int n, int ld, int nb2) {
    sq_ptr = U; sq_n = n; sq_ld = ld; sq_nb2_ = nb2;
  }
  bool sq_known(const double* U, int n, int ld, int nb2) const {
    return sq_ptr && sq_ptr == U && sq_n == n && sq_ld == ld && sq_nb2_ == nb2;
  }
  int sq_nb2() const { return sq_nb2_; }  // the panel width the slots were written with
  // the block cache alone dropped: winv lost its contents or its block width (gpr_set_block,
  // a regrown winv) while the factor stands -- its squares stay valid.  Not to be folded into
  // factor_forget: with the squares dropped here too, the posterior after gpr_set_block(64),
  // gpr_set_block(128) differed in its last bits from the one before (the squares are then
  // recomputed from recomputed block inverses); tests/test_gpu_ctx_state.py
  // test_block_width_there_and_back failed on that and pins the kept squares
  void factor_forget_blocks() {
    fac_ptr = nullptr;
    fac_n = fac_ld = fac_nb = 0;
  }
  // both caches dropped: a factorisation starts, a factor buffer is overwritten
  // (gpr_forget_factor for the caller's own writes)
  void factor_forget() {
    fac_ptr = sq_ptr = nullptr;
    fac_n = fac_ld = fac_nb = sq_n = sq_ld = sq_nb2_ = 0;
  }
  // the cached factor grew in place to order n (gpr_fit_append, which wrote the new blocks'
  // inverses): the block cache follows it, the squares are not extended
  void factor_extend(int n) {
    fac_n = n;
    sq_ptr = nullptr;
    sq_n = sq_ld = sq_nb2_ = 0;
  }
  // ---- the matrix the upper-only K assembly left without its strict lower off-diagonal tiles --
  void kup_claim(const double* K, int n, int ld) { kup_ptr = K; kup_n = n; kup_ld = ld; }
  bool kup_pending(const double* K) const { return kup_ptr && kup_ptr == K; }
  void kup_drop() { kup_ptr = nullptr; kup_n = kup_ld = 0; }
  // the next factorisation takes the claim, whatever it factors: true for exactly that matrix
  // (which then owes the lower tiles), and the claim is gone either way
  bool kup_take(const double* K, int n, int ld) {
    const bool mine = kup_pending(K) && kup_n == n && kup_ld == ld;
    kup_drop();
    return mine;
  }
  // a workspace [p, p + cap) was freed: no key may point into it, or the allocator handing the
  // address out again would read as a hit
  void release_range(const double* p, size_t cap) {
    auto inside = [&](const double* q) {
      return q && (uintptr_t)q - (uintptr_t)p < cap * sizeof(double);
    };
    if (inside(fac_ptr)) factor_adopt(nullptr, 0, 0, 0);
    if (inside(sq_ptr)) sq_adopt(nullptr, 0, 0, 0);
    if (inside(kup_ptr)) kup_drop();
  }

 private:
  const double* fac_ptr = nullptr;
  int fac_n = 0, fac_ld = 0, fac_nb = 0;
  const double* sq_ptr = nullptr;
  int sq_n = 0, sq_ld = 0, sq_nb2_ = 0;
  const double* kup_ptr = nullptr;
  int kup_n = 0, kup_ld = 0;
};
