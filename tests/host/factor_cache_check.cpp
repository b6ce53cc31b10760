// Stand-alone host check of the context's cache rules (csrc/factor_cache.hpp, which includes
// nothing from HIP).  Built and run by tests/test_factor_cache_host.py; exits non-zero at the
// first rule that does not hold.
#include <cstdio>

#include "factor_cache.hpp"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

int main() {
  static double buf[64], other[8];
  const double* U = buf + 8;

  {  // adopt, then known with the same key; unknown with any one of pointer / n / ld / nb changed
    FactorCache c;
    CHECK(!c.factor_known(U, 300, 384, 128));
    CHECK(!c.factor_known(nullptr, 0, 0, 0));  // (an empty cache matches nothing)
    c.factor_adopt(U, 300, 384, 128);
    CHECK(c.factor_known(U, 300, 384, 128));
    CHECK(!c.factor_known(U + 1, 300, 384, 128));
    CHECK(!c.factor_known(other, 300, 384, 128));
    CHECK(!c.factor_known(U, 299, 384, 128));
    CHECK(!c.factor_known(U, 300, 300, 128));
    CHECK(!c.factor_known(U, 300, 384, 64));
    CHECK(!c.sq_known(U, 300, 384, 1024));  // (the two caches are separate)
    c.sq_adopt(U, 300, 384, 1024);
    CHECK(c.sq_known(U, 300, 384, 1024) && c.sq_nb2() == 1024);
    CHECK(!c.sq_known(U + 1, 300, 384, 1024));
    CHECK(!c.sq_known(U, 301, 384, 1024));
    CHECK(!c.sq_known(U, 300, 385, 1024));
    CHECK(!c.sq_known(U, 300, 384, 512));
    CHECK(c.factor_known(U, 300, 384, 128));
  }
  {  // forget clears both caches
    FactorCache c;
    c.factor_adopt(U, 300, 384, 128);
    c.sq_adopt(U, 300, 384, 1024);
    c.factor_forget();
    CHECK(!c.factor_known(U, 300, 384, 128));
    CHECK(!c.sq_known(U, 300, 384, 1024));
    CHECK(c.sq_nb2() == 0);
  }
  {  // forgetting the blocks alone keeps the squares
    FactorCache c;
    c.factor_adopt(U, 300, 384, 128);
    c.sq_adopt(U, 300, 384, 1024);
    c.factor_forget_blocks();
    CHECK(!c.factor_known(U, 300, 384, 128));
    CHECK(c.sq_known(U, 300, 384, 1024) && c.sq_nb2() == 1024);
  }
  {  // extend keeps the block cache, re-keys n, and drops the squares
    FactorCache c;
    c.factor_adopt(U, 300, 384, 128);
    c.sq_adopt(U, 300, 384, 1024);
    c.factor_extend(301);
    CHECK(c.factor_known(U, 301, 384, 128));
    CHECK(!c.factor_known(U, 300, 384, 128));
    CHECK(!c.sq_known(U, 300, 384, 1024));
    CHECK(!c.sq_known(U, 301, 384, 1024));
  }
  {  // a released range [p, p + cap) drops a key at p, in the middle and at the last element;
     // it keeps a key at p + cap and one below p
    const double* p = buf + 16;
    const size_t cap = 32;
    const double* inside[] = {p, p + 7, p + cap - 1};
    for (const double* k : inside) {
      FactorCache c;
      c.factor_adopt(k, 10, 10, 128);
      c.sq_adopt(k, 10, 10, 1024);
      c.kup_claim(k, 10, 10);
      c.release_range(p, cap);
      CHECK(!c.factor_known(k, 10, 10, 128));
      CHECK(!c.sq_known(k, 10, 10, 1024));
      CHECK(!c.kup_pending(k));
    }
    const double* outside[] = {p + cap, p - 1, buf, other};
    for (const double* k : outside) {
      FactorCache c;
      c.factor_adopt(k, 10, 10, 128);
      c.sq_adopt(k, 10, 10, 1024);
      c.kup_claim(k, 10, 10);
      c.release_range(p, cap);
      CHECK(c.factor_known(k, 10, 10, 128));
      CHECK(c.sq_known(k, 10, 10, 1024));
      CHECK(c.kup_pending(k));
    }
    {  // each cache by its own key
      FactorCache c;
      c.factor_adopt(p + 3, 10, 10, 128);
      c.sq_adopt(other, 10, 10, 1024);
      c.release_range(p, cap);
      CHECK(!c.factor_known(p + 3, 10, 10, 128));
      CHECK(c.sq_known(other, 10, 10, 1024));
    }
    {  // an empty range and an empty cache
      FactorCache c;
      c.release_range(p, 0);
      c.factor_adopt(p, 10, 10, 128);
      c.release_range(p, 0);
      CHECK(c.factor_known(p, 10, 10, 128));
    }
  }
  {  // the kup claim is consumed exactly once, and only by the matching (pointer, n, ld)
    FactorCache c;
    CHECK(!c.kup_take(U, 300, 384));
    c.kup_claim(U, 300, 384);
    CHECK(c.kup_pending(U) && !c.kup_pending(other));
    CHECK(c.kup_take(U, 300, 384));
    CHECK(!c.kup_take(U, 300, 384));
    CHECK(!c.kup_pending(U));
    const struct { const double* p; int n, ld; } wrong[] = {
        {other, 300, 384}, {U, 299, 384}, {U, 300, 300}};
    for (const auto& w : wrong) {  // any other factorisation takes nothing, and the claim goes
      c.kup_claim(U, 300, 384);
      CHECK(!c.kup_take(w.p, w.n, w.ld));
      CHECK(!c.kup_take(U, 300, 384));
    }
    c.kup_claim(U, 300, 384);
    c.kup_drop();
    CHECK(!c.kup_take(U, 300, 384));
    c.kup_claim(U, 300, 384);  // the factor caches and the claim do not touch each other
    c.factor_forget();
    CHECK(c.kup_take(U, 300, 384));
  }
  if (failures) return 1;
  std::printf("factor cache rules ok\n");
  return 0;
}
