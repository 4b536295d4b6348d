// mdntt_plan.hpp — the host-only part of include/nttmul_mdntt.h: what create and a call decide
// before any device access, and the sub-batch arithmetic of a call.  Plain C++ with no HIP
// header, so that a CPU build can run it under sanitizers (tests/sanitize/mdntt_san.cpp, with
// basis.cpp and planner.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "basis.hpp"
#include "nttmul_rns.h"
#include "subbatch.hpp"

namespace nttmul {

// nttmul_mdntt_create's status: nttmul_ks_create's (ks_plan.cpp ks_validate) without the digit
// width, in the same order -- every EINVAL of either basis, the extended basis' limb count, then
// the unsupported shapes and word classes.  On success B holds the params and the word class.
inline int mdntt_validate(const nttmul_params *caller, size_t size, const uint64_t *q, uint32_t L,
                          const uint64_t *p, uint32_t K, BasisRequest *B) {
  const uint64_t *const bases[2] = {q, p};
  const uint32_t limbs[2] = {L, K};
  // a degree above 65536 is valid and unsupported
  if (const int st = basis_invalid(caller, size, bases, limbs, 2, 1u << 30, B)) return st;
  // the extended basis is one nttmul_rns / nttmul_rnsmp context's
  if (L + K > NTTMUL_RNS_MAX_LIMBS) return NTTMUL_EINVAL;
  // (p3_fold: what nttmul_rns_create asks of a 32-bit basis at n = 4096)
  return basis_unsupported(B, 256, 65536, true);
}

// A call's status before any device access
inline int mdntt_call_status(bool have_ctx, const void *out, const void *x_hat, size_t batch) {
  if (!have_ctx) return NTTMUL_EINVAL;
  if (batch && (!out || !x_hat)) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

// The shape of a call's sub-batches: no scratch buffer of a sub-batch ([cnt][K][n] and, above
// n = 4096, [cnt][L][n] words) exceeds `limit` bytes; never less than one polynomial
struct MdShape {
  size_t y_bytes, t_bytes;    // per polynomial: K n words, L n words
  size_t in_words, out_words; // per polynomial of x_hat ((L + K) n) and of out (L n)
  size_t chunk, subs;
};
inline MdShape mdntt_shape(size_t limit, uint32_t n, uint32_t L, uint32_t K, int word_bits,
                           size_t batch) {
  MdShape S;
  const size_t wb = (size_t)word_bits / 8;
  S.y_bytes = (size_t)K * n * wb;
  S.t_bytes = n > 4096 ? (size_t)L * n * wb : 0;
  S.in_words = ((size_t)L + K) * n;
  S.out_words = (size_t)L * n;
  S.chunk = mp_chunk(limit, S.y_bytes, S.t_bytes, batch);
  S.subs = batch ? mp_subs(batch, S.chunk) : 0;
  return S;
}

}  // namespace nttmul
