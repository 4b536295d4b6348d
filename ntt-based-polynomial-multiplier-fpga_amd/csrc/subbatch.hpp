// subbatch.hpp — the sub-batch rule of a multi-pass context (rnsmp.cpp run, for every operation of
// include/nttmul_rnsmp.h and for the mac against several operands of include/nttmul_macn.h).
// Plain arithmetic with no device header, so that a CPU build can run it under sanitizers
// (tests/sanitize/macn_san.cpp).
#pragma once
#include <stddef.h>

#include <algorithm>

namespace nttmul {

// The sub-batch of a multi-pass call: the largest polynomial count for which neither the
// column-passed a (in_bytes per batch entry: all limbs, for a mac all terms) nor the row pass's
// output (out_bytes per batch entry: all limbs, all components) exceeds `limit` bytes; never less
// than one polynomial (the scratch then grows to hold it), never more than the batch
inline size_t mp_chunk(size_t limit, size_t in_bytes, size_t out_bytes, size_t batch) {
  return std::max<size_t>(1, std::min(batch, limit / std::max(in_bytes, out_bytes)));
}

// Sub-batch k of a call: cnt polynomials from polynomial p; the byte offsets of its c, a and b are
// p times the operand's bytes per batch entry
struct MpSub {
  size_t p, cnt;
};
inline size_t mp_subs(size_t batch, size_t chunk) { return (batch + chunk - 1) / chunk; }
inline MpSub mp_sub(size_t batch, size_t chunk, size_t k) {
  return MpSub{k * chunk, std::min(chunk, batch - k * chunk)};
}

}  // namespace nttmul
