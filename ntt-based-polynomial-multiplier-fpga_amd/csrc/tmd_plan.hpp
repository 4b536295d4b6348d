// tmd_plan.hpp — the host-only part of include/nttmul_tmd.h: what create and a call decide
// before any device access, the plain constants of a context (nttmul_tmd_plan returns them,
// create derives its device tables from the same values) and the sub-batch arithmetic of a call.
// Plain C++ with no HIP header, so that a CPU build can run it under sanitizers
// (tests/sanitize/tmd_san.cpp, with basis.cpp and planner.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "mdntt_plan.hpp"
#include "planner.hpp"

namespace nttmul {

// The plaintext modulus of a word class: odd, 3 <= t < tmd_t_bound.  The bound is the target
// modulus bound of BconvArith<W>'s range contract (the base conversion's kernel header:
// c <= 2^31 - 1, c <= 2^62 - 1), which the mod-t accumulator takes t through; it also keeps
// |u| <= (t - 1) / 2 inside the contract's operand range.
constexpr uint64_t tmd_t_bound(int word_bits) {
  return word_bits == 32 ? (uint64_t)1 << 31 : (uint64_t)1 << 62;
}

// The plain constants of a context
struct TmPlan {
  uint32_t n = 0, logn = 0, L = 0, K = 0, flags = 0;
  int word_bits = 0;
  uint64_t t = 0;                  // the plaintext modulus
  uint64_t msg_factor = 0;         // P^-1 mod t
  nttmul_params prm = {};          // the caller's params, zero-extended (create: the devices)
  std::vector<uint64_t> q, p;      // Q [L], P [K]
  std::vector<uint64_t> yscale;    // [K]: Ph_j^-1 mod p_j
  std::vector<uint64_t> g;         // [K]: -p_j^-1 mod t
  std::vector<uint64_t> w;         // [K + 2][L]: Ph_j mod q_l; row K: P mod q_l; row K + 1: -P mod q_l
  std::vector<uint64_t> v;         // [L]: P^-1 mod q_l
  // the m-th modulus of the extended basis q_0 .. q_{L-1}, p_0 .. p_{K-1}
  uint64_t modulus(uint32_t m) const { return m < L ? q[m] : p[m - L]; }
};

// nttmul_tmd_create's status: nttmul_mdntt_create's, in the same order (mdntt_plan.hpp
// mdntt_validate); then the plaintext modulus: below 3 (EINVAL), even (EUNSUPPORTED), at or above
// the class bound (EINVAL), 0 modulo some p_j or q_l (EINVAL).  On success n .. word_bits, t, q
// and p are set
inline int tmd_validate(const nttmul_params *caller, size_t size, const uint64_t *q, uint32_t L,
                        const uint64_t *p, uint32_t K, uint64_t t, TmPlan *P) {
  BasisRequest B;
  if (const int st = mdntt_validate(caller, size, q, L, p, K, &B)) return st;
  if (t < 3) return NTTMUL_EINVAL;
  if (!(t & 1)) return NTTMUL_EUNSUPPORTED;
  if (t >= tmd_t_bound(B.word_bits)) return NTTMUL_EINVAL;
  for (uint32_t j = 0; j < K; j++)
    if (t % p[j] == 0) return NTTMUL_EINVAL;
  for (uint32_t l = 0; l < L; l++)
    if (t % q[l] == 0) return NTTMUL_EINVAL;
  P->prm = B.prm;
  P->n = B.prm.n;
  P->logn = (uint32_t)__builtin_ctz(P->n);
  P->L = L;
  P->K = K;
  P->flags = B.prm.flags;
  P->word_bits = B.word_bits;
  P->t = t;
  P->q.assign(q, q + L);
  P->p.assign(p, p + K);
  return NTTMUL_OK;
}

// a^-1 mod m for gcd(a, m) = 1, m >= 2 (t is not prime in general: extended Euclid, the
// coefficient of a kept modulo m)
inline uint64_t tmd_invmod(uint64_t a, uint64_t m) {
  uint64_t r0 = m, r1 = a % m;
  uint64_t s0 = 0, s1 = 1;  // r_i = s_i a (mod m)
  while (r1) {
    const uint64_t k = r0 / r1, r2 = r0 - k * r1;
    const uint64_t ks = mulmod(k % m, s1, m), s2 = s0 >= ks ? s0 - ks : s0 + (m - ks);
    r0 = r1, r1 = r2;
    s0 = s1, s1 = s2;
  }
  return s0;  // r0 = 1
}

// yscale .. msg_factor of a validated plan
inline void tmd_constants(TmPlan *P) {
  const uint32_t L = P->L, K = P->K;
  const uint64_t t = P->t;
  // the product of P's moduli without p_skip (skip >= K: of all of them), mod m
  const auto prod = [&](uint32_t skip, uint64_t m) {
    uint64_t r = 1 % m;
    for (uint32_t j = 0; j < K; j++)
      if (j != skip) r = mulmod(r, P->p[j] % m, m);
    return r;
  };
  P->yscale.assign(K, 0);
  P->g.assign(K, 0);
  P->w.assign((size_t)(K + 2) * L, 0);
  P->v.assign(L, 0);
  for (uint32_t j = 0; j < K; j++) {
    const uint64_t pj = P->p[j];
    P->yscale[j] = powmod(prod(j, pj), pj - 2, pj);  // p_j prime
    P->g[j] = (t - tmd_invmod(pj % t, t)) % t;       // p_j does not divide t: coprime
  }
  for (uint32_t l = 0; l < L; l++) {
    const uint64_t ql = P->q[l], Pm = prod(K, ql);
    for (uint32_t j = 0; j < K; j++) P->w[(size_t)j * L + l] = prod(j, ql);
    P->w[(size_t)K * L + l] = Pm;
    P->w[(size_t)(K + 1) * L + l] = (ql - Pm) % ql;
    P->v[l] = powmod(Pm, ql - 2, ql);
  }
  P->msg_factor = tmd_invmod(prod(K, t), t);
}

// A call's status before any device access
inline int tmd_call_status(bool have_ctx, const void *out, const void *x_hat, size_t batch) {
  return mdntt_call_status(have_ctx, out, x_hat, batch);
}

// The shape of a call's sub-batches: mdntt_shape's (the scratch holds y [cnt][K][n] and, above
// n = 4096, the column-passed sums [cnt][L][n])
inline MdShape tmd_shape(size_t limit, uint32_t n, uint32_t L, uint32_t K, int word_bits,
                         size_t batch) {
  return mdntt_shape(limit, n, L, K, word_bits, batch);
}

}  // namespace nttmul
