// ctlin_plan.hpp — the host-only part of include/nttmul_ctlin.h: what create and a call decide
// before any device access, the plain constants of a context and the grid arithmetic of the two
// launches.  Plain C++ with no HIP header, so that a CPU build can run it under sanitizers
// (tests/sanitize/ctlin_san.cpp, with basis.cpp and planner.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "basis.hpp"
#include "ctmul_plan.hpp"
#include "nttmul_ctlin.h"
#include "planner.hpp"

namespace nttmul {

enum ClOp { kClCombine = 0, kClTensor = 1 };

// The plain constants of a context
struct ClPlan {
  uint32_t n = 0, logn = 0, L = 0, flags = 0;
  int word_bits = 0;
  nttmul_params prm = {};        // the caller's params, zero-extended (create: the devices)
  std::vector<uint64_t> m;       // [L]: q_0 .. q_{L-1}
  std::vector<uint64_t> r1, r2;  // [L]: R mod q_l and R^2 mod q_l, R = 2^word_bits
};

// nttmul_ctlin_create's status: nttmul_galois_create's, in its order
inline int ctlin_validate(const nttmul_params *caller, size_t size, const uint64_t *q, uint32_t L,
                          ClPlan *P) {
  BasisRequest B;
  // a degree above 65536 is valid and unsupported
  if (const int st = basis_invalid(caller, size, &q, &L, 1, 1u << 30, &B)) return st;
  if (const int st = basis_unsupported(&B, 256, 65536, false)) return st;
  P->prm = B.prm;
  P->n = B.prm.n;
  P->logn = (uint32_t)__builtin_ctz(P->n);
  P->L = L;
  P->flags = B.prm.flags;
  P->word_bits = B.word_bits;
  P->m.assign(q, q + L);
  return NTTMUL_OK;
}

// r1 and r2 of a validated plan
inline void ctlin_constants(ClPlan *P) {
  P->r1.assign(P->L, 0);
  P->r2.assign(P->L, 0);
  for (uint32_t l = 0; l < P->L; l++) {
    P->r1[l] = (uint64_t)(((unsigned __int128)1 << P->word_bits) % P->m[l]);
    P->r2[l] = mulmod(P->r1[l], P->r1[l], P->m[l]);
  }
}

// combine's status before any device access, in this order: a NULL context; nterms 0 or above
// NTTMUL_CTLIN_MAX_TERMS; comps 0 or above NTTMUL_CTLIN_MAX_COMPS; NULL terms; per term in index
// order a kind above 2, a non-zero reserved, ONE with a w, SCALAR or PLAIN without one, ONE
// without an x; a NULL out with batch > 0
inline int ctlin_combine_status(bool have_ctx, const void *out, const nttmul_ctlin_term *terms,
                                uint32_t nterms, size_t batch, uint32_t comps) {
  if (!have_ctx) return NTTMUL_EINVAL;
  if (!nterms || nterms > NTTMUL_CTLIN_MAX_TERMS) return NTTMUL_EINVAL;
  if (!comps || comps > NTTMUL_CTLIN_MAX_COMPS) return NTTMUL_EINVAL;
  if (!terms) return NTTMUL_EINVAL;
  for (uint32_t i = 0; i < nterms; i++) {
    const nttmul_ctlin_term &t = terms[i];
    if (t.kind > NTTMUL_CTLIN_PLAIN) return NTTMUL_EINVAL;
    if (t.reserved) return NTTMUL_EINVAL;
    if (t.kind == NTTMUL_CTLIN_ONE && t.w) return NTTMUL_EINVAL;
    if (t.kind != NTTMUL_CTLIN_ONE && !t.w) return NTTMUL_EINVAL;
    if (t.kind == NTTMUL_CTLIN_ONE && !t.x) return NTTMUL_EINVAL;
  }
  if (batch && !out) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

// tensor's: nttmul_ctmul_high's
inline int ctlin_tensor_status(bool have_ctx, const void *d_hat, const void *x_hat,
                               const void *y_hat, size_t batch, uint32_t pairs) {
  return ctmul_high_status(have_ctx, d_hat, x_hat, y_hat, batch, pairs);
}

// The grid of both launches, (wgx, L): k_ctmul_high's.  A lane takes the vector of
// ctmul_vec_words consecutive words at one slot of one batch entry, in every component
inline CtHighGrid ctlin_grid(size_t batch, uint32_t logn, int word_bits) {
  return ctmul_high_grid(batch, logn, word_bits);
}

// Words of combine's operands: out and every x [batch][comps][L][n]; a SCALAR's w [L], a PLAIN's
// [L][n]
inline void ctlin_combine_words(uint32_t L, uint32_t n, size_t batch, uint32_t comps,
                                size_t words[3]) {
  words[0] = batch * comps * L * n;
  words[1] = L;
  words[2] = (size_t)L * n;
}

// Words of tensor's: d_hat [batch][3][L][n], x_hat and y_hat [batch][pairs][2][L][n]
inline void ctlin_tensor_words(uint32_t L, uint32_t n, size_t batch, uint32_t pairs,
                               size_t words[2]) {
  words[0] = batch * 3 * L * n;
  words[1] = batch * pairs * 2 * L * n;
}

// The first word of component c of batch entry p, limb l, in a [..][comps][L][n] operand
inline size_t ctlin_word_offset(size_t p, uint32_t comps, uint32_t c, uint32_t L, uint32_t l,
                                uint32_t logn) {
  return ((p * comps + c) * L + l) << logn;
}

}  // namespace nttmul
