// macn_plan.hpp — what the calls of include/nttmul_macn.h decide on the host before any device
// access: the status of their arguments (the operands' sizes are rns.hpp op_words', the sub-batches
// of a multi-pass context subbatch.hpp's).  No device header, so that a CPU build can run it under
// sanitizers (tests/sanitize/macn_san.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "nttmul_macn.h"

namespace nttmul {

// have_ctx: the handle is not NULL.  batch = 0 is a successful no-op, also with NULL operands
inline int macn_args(bool have_ctx, const void *c, const void *a, const void *b_hat, size_t batch,
                     uint32_t terms, uint32_t comps) {
  if (!have_ctx || !terms || !comps || comps > NTTMUL_MACN_MAX_COMPS) return NTTMUL_EINVAL;
  if (batch && (!c || !a || !b_hat)) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

}  // namespace nttmul
