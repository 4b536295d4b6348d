// lintrans.hpp — internal interface between the host entry points of include/nttmul_lintrans.h
// (lintrans.cpp) and the launcher of lintrans.hip.  lib/libnttmul_lintrans.so only.
#pragma once
#include "ksntt.hpp"
#include "lintrans_plan.hpp"

namespace nttmul {

// Constants of one limb of Q u P beyond its BconvTo entry: R^2 mod m as the (value, companion)
// pair the word class multiplies by (bconv.hpp mul_pair), and P mod m in the form mont takes (the
// canonical word; 0 on the limbs of P, which never read it)
template <class W>
struct LtLimb {
  W r2, r2s, pq;
};

// Per-device view of a context: what the launch needs (pointers are device memory).  M = L + K.
struct LtTables {
  uint32_t logn = 0, L = 0, K = 0;
  int word_bits = 0;
  const void *to = nullptr;    // BconvTo<W>[bconv_pad(M)]: m, -m^-1, R mod m, the pair of R mod m
  const void *limb = nullptr;  // LtLimb<W>[M]
};

// The one launch of apply: a_hat [batch][terms][M][n], b_hat [rots][comps][terms][M][n],
// w_hat [rots][M][n] or NULL, c0_hat [batch][L][n] or NULL -> c_hat [batch][comps][M][n]
hipError_t launch_lintrans(const LtTables &T, void *c_hat, const void *a_hat, const void *b_hat,
                           const void *w_hat, const void *c0_hat, const HoistArgs &H, size_t batch,
                           uint32_t terms, hipStream_t s);
// "k_lintrans<Arith64,u64,2,1>": the dry run of the launching statement itself
hipError_t describe_lintrans(const LtTables &T, uint32_t comps, bool weighted, std::string *out);

// apply with b_hat and, when given, w_hat viewed (ksntt.hpp KsnttViewed's shape): `check` in
// place of their range checks, `launch` in place of launch_lintrans, b_words and w_words the whole
// viewed operands (what the host form stages)
struct LtViewed {
  const LevelAddr *addr;
  size_t b_words, w_words;
  LevelCheck check;
  hipError_t (*launch)(const LtTables &T, void *c_hat, const void *a_hat, const void *b_hat,
                       const void *w_hat, const void *c0_hat, const HoistArgs &H, size_t batch,
                       uint32_t terms, const LevelAddr &A, hipStream_t s);
};
// nttmul_lintrans_apply (host != 0; dev and stream unused) or nttmul_lintrans_apply_device with V
// for b_hat and w_hat: the same argument checks, device selection, range checks of a_hat and
// c0_hat and error text
int lintrans_apply_viewed(nttmul_lintrans *h, const LtViewed &V, void *c_hat, const void *a_hat,
                          const void *b_hat, const void *w_hat, const void *c0_hat,
                          const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                          uint32_t comps, int host, int dev, void *stream);

}  // namespace nttmul
