// lintrans_plan.hpp — the host-only part of include/nttmul_lintrans.h: what create and a call
// decide before any device access, the plain constants of a context and the grid arithmetic of
// the one launch.  Plain C++ with no HIP header, so that a CPU build can run it under sanitizers
// (tests/sanitize/lintrans_san.cpp, with basis.cpp and planner.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "basis.hpp"
#include "hoist_plan.hpp"
#include "nttmul_lintrans.h"
#include "planner.hpp"

namespace nttmul {

// The plain constants of a context.  M = L + K, the extended basis ordered Q then P
struct LtPlan {
  uint32_t n = 0, logn = 0, L = 0, K = 0, flags = 0;
  int word_bits = 0;
  nttmul_params prm = {};          // the caller's params, zero-extended (create: the devices)
  std::vector<uint64_t> m;         // [M]: q_0 .. q_{L-1}, p_0 .. p_{K-1}
  std::vector<uint64_t> r1, r2;    // [M]: R mod m_l and R^2 mod m_l, R = 2^word_bits
  std::vector<uint64_t> pq;        // [L]: P mod q_l
};

// nttmul_lintrans_create's status: nttmul_ksntt_create's in its order (ks_plan.cpp ks_validate)
// without the digit width's checks
inline int lintrans_validate(const nttmul_params *caller, size_t size, const uint64_t *q,
                             uint32_t L, const uint64_t *p, uint32_t K, LtPlan *P) {
  const uint64_t *const bases[2] = {q, p};
  const uint32_t limbs[2] = {L, K};
  BasisRequest B;
  // a degree above 65536 is valid and unsupported
  if (const int st = basis_invalid(caller, size, bases, limbs, 2, 1u << 30, &B)) return st;
  if (L + K > NTTMUL_RNS_MAX_LIMBS) return NTTMUL_EINVAL;
  if (const int st = basis_unsupported(&B, 256, 65536, true)) return st;
  P->prm = B.prm;
  P->n = B.prm.n;
  P->logn = (uint32_t)__builtin_ctz(P->n);
  P->L = L;
  P->K = K;
  P->flags = B.prm.flags;
  P->word_bits = B.word_bits;
  P->m.assign(q, q + L);
  P->m.insert(P->m.end(), p, p + K);
  return NTTMUL_OK;
}

// r1, r2 and pq of a validated plan
inline void lintrans_constants(LtPlan *P) {
  const uint32_t M = P->L + P->K;
  P->r1.assign(M, 0);
  P->r2.assign(M, 0);
  P->pq.assign(P->L, 0);
  for (uint32_t l = 0; l < M; l++) {
    P->r1[l] = (uint64_t)(((unsigned __int128)1 << P->word_bits) % P->m[l]);
    P->r2[l] = mulmod(P->r1[l], P->r1[l], P->m[l]);
  }
  for (uint32_t l = 0; l < P->L; l++) {
    uint64_t v = 1;
    for (uint32_t j = 0; j < P->K; j++) v = mulmod(v, P->m[P->L + j] % P->m[l], P->m[l]);
    P->pq[l] = v;
  }
}

// apply's status before any device access: nttmul_ksntt_mac_device's, in its order
// (hoist_plan.hpp hoist_args).  w_hat and c0_hat may be NULL and are not looked at
inline int lintrans_apply_status(bool have_ctx, uint32_t n, const void *c_hat, const void *a_hat,
                                 const void *b_hat, const uint32_t *k, uint32_t rots, size_t batch,
                                 uint32_t terms, uint32_t comps,
                                 uint32_t kv[NTTMUL_HOIST_MAX_ROTS]) {
  return hoist_args(have_ctx, n, c_hat, a_hat, b_hat, k, rots, batch, terms, comps, kv);
}

// batch entries a k_lintrans workgroup takes (the V slices of the kernel's header comment: the
// same 256 slots of V consecutive batch entries)
constexpr uint32_t kLtSlices = 4;

// The grid of the one launch, (wgx, M).  Batch-sliced (the library's form): a unit is a batch
// entry, groups = ceil(batch / V) runs of V entries, one workgroup per (run, range of 256 slots),
// the range the faster index.  Slot-sliced (k_ksntt_mac's form, kept for the A/B): a unit is a slice
// of 256 slots of one polynomial, batch n / 256 of them, V consecutive ones per workgroup.
// tail: the units of the last, partial run (0: every run is full).  ok: wgx fits a grid dimension
struct LtGrid {
  size_t units, groups, wgx;
  uint32_t tail;
  bool ok;
};
inline LtGrid lintrans_grid(size_t batch, uint32_t logn, bool slot_sliced = false,
                            uint32_t v = kLtSlices) {
  LtGrid G;
  const uint32_t lgs = logn - 8;
  G.units = slot_sliced ? batch << lgs : batch;
  G.groups = G.units / v + (G.units % v != 0);
  G.wgx = slot_sliced ? G.groups : G.groups << lgs;
  G.tail = (uint32_t)(G.units % v);
  G.ok = G.groups <= (0x7FFFFFFFull >> (slot_sliced ? 0 : lgs));
  return G;
}

// Words of apply's operands: c_hat [batch][comps][M][n], a_hat [batch][terms][M][n],
// b_hat [rots][comps][terms][M][n], w_hat [rots][M][n], c0_hat [batch][L][n]
inline void lintrans_words(uint32_t L, uint32_t K, uint32_t n, size_t batch, uint32_t terms,
                           uint32_t rots, uint32_t comps, size_t words[5]) {
  const size_t poly = ((size_t)L + K) * n;
  words[0] = batch * comps * poly;
  words[1] = batch * terms * poly;
  words[2] = (size_t)rots * comps * terms * poly;
  words[3] = (size_t)rots * poly;
  words[4] = batch * L * n;
}

}  // namespace nttmul
