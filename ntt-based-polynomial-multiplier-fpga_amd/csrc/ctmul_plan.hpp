// ctmul_plan.hpp — the host-only part of include/nttmul_ctmul.h: what create and a call decide
// before any device access, the plain constants of a context and the grid arithmetic of the two
// launches.  Plain C++ with no HIP header, so that a CPU build can run it under sanitizers
// (tests/sanitize/ctmul_san.cpp, with basis.cpp and planner.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "lintrans_plan.hpp"
#include "nttmul_ctmul.h"

namespace nttmul {

enum CtOp { kCtHigh = 0, kCtRelin = 1 };

// The plain constants of a context.  M = L + K, the extended basis ordered Q then P
struct CtPlan {
  uint32_t n = 0, logn = 0, L = 0, K = 0, flags = 0;
  int word_bits = 0;
  nttmul_params prm = {};          // the caller's params, zero-extended (create: the devices)
  std::vector<uint64_t> m;         // [M]: q_0 .. q_{L-1}, p_0 .. p_{K-1}
  std::vector<uint64_t> r1;        // [M]: R mod m_l, R = 2^word_bits
  std::vector<uint64_t> pr;        // [L]: P R mod q_l
};

// nttmul_ctmul_create's status: nttmul_lintrans_create's, in its order
inline int ctmul_validate(const nttmul_params *caller, size_t size, const uint64_t *q, uint32_t L,
                          const uint64_t *p, uint32_t K, CtPlan *P) {
  LtPlan T;
  if (const int st = lintrans_validate(caller, size, q, L, p, K, &T)) return st;
  P->prm = T.prm;
  P->n = T.n;
  P->logn = T.logn;
  P->L = T.L;
  P->K = T.K;
  P->flags = T.flags;
  P->word_bits = T.word_bits;
  P->m = T.m;
  return NTTMUL_OK;
}

// r1 and pr of a validated plan
inline void ctmul_constants(CtPlan *P) {
  const uint32_t M = P->L + P->K;
  P->r1.assign(M, 0);
  P->pr.assign(P->L, 0);
  for (uint32_t l = 0; l < M; l++)
    P->r1[l] = (uint64_t)(((unsigned __int128)1 << P->word_bits) % P->m[l]);
  for (uint32_t l = 0; l < P->L; l++) {
    uint64_t v = P->r1[l];
    for (uint32_t j = 0; j < P->K; j++) v = mulmod(v, P->m[P->L + j] % P->m[l], P->m[l]);
    P->pr[l] = v;
  }
}

// high's status before any device access, in this order: a NULL context; pairs = 0; a NULL
// d2_hat, x_hat or y_hat with batch > 0
inline int ctmul_high_status(bool have_ctx, const void *d2_hat, const void *x_hat,
                             const void *y_hat, size_t batch, uint32_t pairs) {
  if (!have_ctx || !pairs) return NTTMUL_EINVAL;
  if (batch && (!d2_hat || !x_hat || !y_hat)) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

// relin's: a NULL context; pairs = 0; terms = 0; a NULL c_hat, up_hat, key_hat, x_hat or y_hat
// with batch > 0
inline int ctmul_relin_status(bool have_ctx, const void *c_hat, const void *up_hat,
                              const void *key_hat, const void *x_hat, const void *y_hat,
                              size_t batch, uint32_t pairs, uint32_t terms) {
  if (!have_ctx || !pairs || !terms) return NTTMUL_EINVAL;
  if (batch && (!c_hat || !up_hat || !key_hat || !x_hat || !y_hat)) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

// batch entries a k_ctmul_relin workgroup takes: k_lintrans's (the same 256 slots of V consecutive
// batch entries)
constexpr uint32_t kCtSlices = kLtSlices;
// The one switch of the A/B library (Makefile ab-ctmul, measured by tools/bench_ctmul.py --lib):
// another count for the 64-bit class; the library itself is built without it
#ifdef NTTMUL_CTMUL_V64
constexpr uint32_t kCtSlices64 = NTTMUL_CTMUL_V64;
#else
constexpr uint32_t kCtSlices64 = kCtSlices;
#endif
constexpr uint32_t ctmul_slices(int word_bits) {
  return word_bits == 64 ? kCtSlices64 : kCtSlices;
}

// relin's grid, (wgx, M): lintrans_grid's batch-sliced form
inline LtGrid ctmul_relin_grid(size_t batch, uint32_t logn, uint32_t v = kCtSlices) {
  return lintrans_grid(batch, logn, false, v);
}

// Words of one 128-bit access of k_ctmul_high
constexpr uint32_t ctmul_vec_words(int word_bits) { return 128u / (uint32_t)word_bits; }

// high's grid, (wgx, L).  A lane takes one vector of vec consecutive words of one limb's stream
// [batch][n], a workgroup 256 consecutive vectors: per = max(1, 256 vec / n) whole polynomials
// (n <= 512 on 32-bit words, n = 256 on 64-bit words), or one of n / (256 vec) parts of one.
// vectors = batch n / vec, wgx = ceil(vectors / 256); tail: the vectors of the last, partial
// workgroup (0: it is whole; lanes past the end do nothing).  ok: wgx fits a grid dimension
struct CtHighGrid {
  size_t vectors, wgx;
  uint32_t vec, per, tail;
  bool ok;
};
inline CtHighGrid ctmul_high_grid(size_t batch, uint32_t logn, int word_bits) {
  CtHighGrid G;
  G.vec = ctmul_vec_words(word_bits);
  const uint32_t pv = (1u << logn) / G.vec;  // vectors of a polynomial: 64 .. 32768
  G.per = pv < 256 ? 256 / pv : 1;
  G.vectors = batch * pv;
  G.wgx = G.vectors / 256 + (G.vectors % 256 != 0);
  G.tail = (uint32_t)(G.vectors % 256);
  G.ok = G.wgx <= 0x7FFFFFFFull;
  return G;
}

// Words of high's operands: d2_hat [batch][L][n], x_hat and y_hat [batch][pairs][2][L][n]
inline void ctmul_high_words(uint32_t L, uint32_t n, size_t batch, uint32_t pairs,
                             size_t words[2]) {
  words[0] = batch * L * n;
  words[1] = batch * pairs * 2 * L * n;
}

// Words of relin's: c_hat [batch][2][M][n], up_hat [batch][terms][M][n], key_hat [2][terms][M][n],
// x_hat and y_hat [batch][pairs][2][L][n]
inline void ctmul_relin_words(uint32_t L, uint32_t K, uint32_t n, size_t batch, uint32_t pairs,
                              uint32_t terms, size_t words[4]) {
  const size_t poly = ((size_t)L + K) * n;
  words[0] = batch * 2 * poly;
  words[1] = batch * terms * poly;
  words[2] = (size_t)2 * terms * poly;
  words[3] = batch * pairs * 2 * L * n;
}

}  // namespace nttmul
