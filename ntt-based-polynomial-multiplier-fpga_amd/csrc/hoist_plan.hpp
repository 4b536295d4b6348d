// hoist_plan.hpp — what the calls of include/nttmul_hoist.h decide on the host before any device
// access: the status of their arguments (the sub-batches of a multi-pass context are
// subbatch.hpp's, over output units).  No device header, so that a
// CPU build can run it under sanitizers (tests/sanitize/hoist_san.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "nttmul_hoist.h"
#include "subbatch.hpp"

namespace nttmul {

// an automorphism of degree n (a power of two): odd and below 2n (galois_plan.hpp galois_k_ok)
inline bool hoist_k_ok(uint32_t n, uint32_t k) { return (k & 1u) && (uint64_t)k < 2ull * n; }

// The order of the header.  have_ctx: the handle is not NULL; n: its degree (unread without a
// context).  batch = 0 is a successful no-op, also with NULL operands; k is read all the same.
// On success kv[0 .. 16) holds the rotations as the kernels take them: k[r] itself, 1 from rots on
inline int hoist_args(bool have_ctx, uint32_t n, const void *c, const void *a_hat,
                      const void *b_hat, const uint32_t *k, uint32_t rots, size_t batch,
                      uint32_t terms, uint32_t comps, uint32_t kv[NTTMUL_HOIST_MAX_ROTS]) {
  if (!have_ctx || !terms || !comps || comps > NTTMUL_MACN_MAX_COMPS) return NTTMUL_EINVAL;
  if (!rots || rots > NTTMUL_HOIST_MAX_ROTS || !k) return NTTMUL_EINVAL;
  for (uint32_t r = 0; r < NTTMUL_HOIST_MAX_ROTS; r++) {
    if (r < rots && !hoist_k_ok(n, k[r])) return NTTMUL_EINVAL;
    kv[r] = r < rots ? k[r] : 1;
  }
  if (batch && (!c || !a_hat || !b_hat)) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

// Output unit u of a call is (p, r) = (u / rots, u mod rots); a sub-batch is a run of consecutive
// units.  Its size and the operands' words are subbatch.hpp's mp_unit_chunk and mp_unit_words with
// upb = rots, the functions rnsmp.cpp run_units itself calls.

}  // namespace nttmul
