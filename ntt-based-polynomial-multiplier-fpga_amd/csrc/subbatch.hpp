// subbatch.hpp — the sub-batch rule of a multi-pass context (rnsmp.cpp run, for every operation of
// include/nttmul_rnsmp.h and for the mac against several operands of include/nttmul_macn.h; rnsmp.cpp
// run_units, for the hoisted rotations of include/nttmul_hoist.h).
// Plain arithmetic with no device header, so that a CPU build can run it under sanitizers
// (tests/sanitize/macn_san.cpp, hoist_san.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

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

// ---- calls whose output is `upb` units per batch entry of `comps` polynomials each, and whose a
// is read from caller memory (rnsmp.cpp run_units; include/nttmul_hoist.h: a unit is a rotation) ----

// The sub-batch of such a call, in units: the largest count whose count * comps polynomials of
// poly_bytes (all limbs) fit `limit`, never less than one, never more than `units`.  Only the
// output passes through the scratch
inline size_t mp_unit_chunk(size_t limit, size_t poly_bytes, uint32_t comps, size_t units) {
  return mp_chunk(limit, 0, poly_bytes * comps, units);
}

// Words of the call's operands: c [batch][upb][comps], a [batch][terms], b [upb][comps][terms],
// each times limbs * n
inline void mp_unit_words(uint32_t limbs, uint32_t n, size_t batch, uint32_t terms, uint32_t upb,
                          uint32_t comps, size_t words[3]) {
  const size_t poly = (size_t)limbs * n;
  words[0] = batch * upb * comps * poly;
  words[1] = batch * terms * poly;
  words[2] = (size_t)upb * comps * terms * poly;
}

}  // namespace nttmul
