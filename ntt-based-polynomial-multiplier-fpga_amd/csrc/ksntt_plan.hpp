// ksntt_plan.hpp — the host-only part of include/nttmul_ksntt.h: what create and a call decide
// before any device access, the digit table and the sub-batch arithmetic of a call.  Plain C++
// with no HIP header, so that a CPU build can run it under sanitizers
// (tests/sanitize/ksntt_san.cpp, with basis.cpp, planner.cpp and ks_plan.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hoist_plan.hpp"
#include "ks_plan.hpp"
#include "subbatch.hpp"

namespace nttmul {

// nttmul_ksntt_create's status: nttmul_ks_create's, in the same order (ks_plan.cpp ks_validate)
inline int ksntt_validate(const nttmul_params *caller, size_t size, const uint64_t *q, uint32_t L,
                          const uint64_t *p, uint32_t K, uint32_t digit_limbs, KsPlan *P) {
  return ks_validate(caller, size, q, L, p, K, digit_limbs, P);
}

// Digit d of Q: limbs [first, first + len).  Every digit has alpha limbs but the last, which has
// what is left of L (1 .. alpha)
struct KsnttDigit {
  uint32_t first, len;
};
inline uint32_t ksntt_digits(uint32_t L, uint32_t alpha) { return (L + alpha - 1) / alpha; }
inline KsnttDigit ksntt_digit(uint32_t L, uint32_t alpha, uint32_t d) {
  const uint32_t first = d * alpha;
  return KsnttDigit{first, first + alpha < L ? alpha : L - first};
}
// m is one of digit d's own limbs (a limb of P never is)
inline bool ksntt_own(uint32_t L, uint32_t alpha, uint32_t d, uint32_t m) {
  const KsnttDigit D = ksntt_digit(L, alpha, d);
  return m >= D.first && m < D.first + D.len;
}

// modup's status before any device access
inline int ksntt_modup_status(bool have_ctx, const void *up_hat, const void *x_hat, size_t batch) {
  if (!have_ctx) return NTTMUL_EINVAL;
  if (batch && (!up_hat || !x_hat)) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

// mac's status before any device access: nttmul_rns_hoist_ntt_device's, in its order
// (hoist_plan.hpp hoist_args)
inline int ksntt_mac_status(bool have_ctx, uint32_t n, const void *c_hat, const void *a_hat,
                            const void *b_hat, const uint32_t *k, uint32_t rots, size_t batch,
                            uint32_t terms, uint32_t comps, uint32_t kv[NTTMUL_HOIST_MAX_ROTS]) {
  return hoist_args(have_ctx, n, c_hat, a_hat, b_hat, k, rots, batch, terms, comps, kv);
}

// The shape of modup's sub-batches.  The scratch holds y [cnt][L][n] (above n = 4096 twice: the
// inverse rows' lazy words and the canonical y).  The column-passed sums t are as large as the
// output, dnum (L + K) limbs per polynomial:
//   t_in_scratch = false  (what the library does) they pass through up_hat itself and the row
//                         pass runs in place on it: only y bounds the sub-batch;
//   t_in_scratch = true   a scratch buffer of their own, bounded as every buffer is, so that the
//                         sub-batch shrinks to what dnum (L + K) limbs allow.
// Never less than one polynomial.
struct KsnttShape {
  size_t y_bytes, t_bytes;     // per polynomial: L n words; dnum (L + K) n words or 0
  size_t in_words, out_words;  // per polynomial of x_hat (L n) and of up_hat (dnum (L + K) n)
  size_t chunk, subs;
};
inline KsnttShape ksntt_shape(size_t limit, uint32_t n, uint32_t L, uint32_t K, uint32_t alpha,
                              int word_bits, size_t batch, bool t_in_scratch = false) {
  KsnttShape S;
  const size_t wb = (size_t)word_bits / 8;
  S.in_words = (size_t)L * n;
  S.out_words = (size_t)ksntt_digits(L, alpha) * ((size_t)L + K) * n;
  S.y_bytes = S.in_words * wb;
  S.t_bytes = n > 4096 && t_in_scratch ? S.out_words * wb : 0;
  S.chunk = mp_chunk(limit, S.y_bytes, S.t_bytes, batch);
  S.subs = batch ? mp_subs(batch, S.chunk) : 0;
  return S;
}

// Words of mac's operands: c_hat [batch][rots][comps], a_hat [batch][terms],
// b_hat [rots][comps][terms], each times (L + K) n (subbatch.hpp mp_unit_words)
inline void ksntt_mac_words(uint32_t limbs, uint32_t n, size_t batch, uint32_t terms,
                            uint32_t rots, uint32_t comps, size_t words[3]) {
  mp_unit_words(limbs, n, batch, terms, rots, comps, words);
}

}  // namespace nttmul
