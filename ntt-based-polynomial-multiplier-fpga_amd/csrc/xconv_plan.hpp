// xconv_plan.hpp — the host-only part of include/nttmul_xconv.h: what create and a call decide
// before any device access, the plain constants of a context (nttmul_xconv_plan returns them,
// create derives its device tables from the same values) and the sub-batch arithmetic of a call.
// Plain C++ with no HIP header, so that a CPU build can run it under sanitizers
// (tests/sanitize/xconv_san.cpp, with basis.cpp and planner.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "mdntt_plan.hpp"
#include "planner.hpp"

namespace nttmul {

enum XcOp { kXcExtend = 0, kXcModdown = 1 };

// The guard band of a = floor(phi + 1/2) is eps = K 2^-kXcBandLog2 (the kernels' header and
// DESIGN.md section 4 derive it)
constexpr uint32_t kXcBandLog2 = 46;

// The plain constants of a context
struct XcPlan {
  uint32_t n = 0, logn = 0, L = 0, K = 0, flags = 0;
  int word_bits = 0;
  uint64_t scale = 0;              // t
  nttmul_params prm = {};          // the caller's params, zero-extended (create: the devices)
  std::vector<uint64_t> q, p;      // Q [L], P [K]
  std::vector<uint64_t> yscale;    // [K]: t Ph_j^-1 mod p_j
  std::vector<uint64_t> w_ext;     // [K + 1][L]: Ph_j mod q_l; row K: -P mod q_l
  std::vector<uint64_t> w_md;      // [K + 1][L]: Ph_j t^-1 mod q_l; row K: -P t^-1 mod q_l
  std::vector<uint64_t> v;         // [L]: t P^-1 mod q_l
  // the m-th modulus of the extended basis q_0 .. q_{L-1}, p_0 .. p_{K-1}
  uint64_t modulus(uint32_t m) const { return m < L ? q[m] : p[m - L]; }
};

// nttmul_xconv_create's status: nttmul_mdntt_create's, in the same order (mdntt_plan.hpp
// mdntt_validate); then the scale: 0, 2^62 or above, or 0 modulo some q_l.  On success n ..
// word_bits, scale, q and p are set
inline int xconv_validate(const nttmul_params *caller, size_t size, const uint64_t *q, uint32_t L,
                          const uint64_t *p, uint32_t K, uint64_t scale, XcPlan *P) {
  BasisRequest B;
  if (const int st = mdntt_validate(caller, size, q, L, p, K, &B)) return st;
  if (scale == 0 || scale >= ((uint64_t)1 << 62)) return NTTMUL_EINVAL;
  for (uint32_t l = 0; l < L; l++)
    if (scale % q[l] == 0) return NTTMUL_EINVAL;
  P->prm = B.prm;
  P->n = B.prm.n;
  P->logn = (uint32_t)__builtin_ctz(P->n);
  P->L = L;
  P->K = K;
  P->flags = B.prm.flags;
  P->word_bits = B.word_bits;
  P->scale = scale;
  P->q.assign(q, q + L);
  P->p.assign(p, p + K);
  return NTTMUL_OK;
}

// yscale .. v of a validated plan
inline void xconv_constants(XcPlan *P) {
  const uint32_t L = P->L, K = P->K;
  const auto inv = [](uint64_t a, uint64_t m) { return powmod(a % m, m - 2, m); };  // m prime
  // the product of P's moduli without p_skip (skip >= K: of all of them), mod m
  const auto prod = [&](uint32_t skip, uint64_t m) {
    uint64_t r = 1 % m;
    for (uint32_t j = 0; j < K; j++)
      if (j != skip) r = mulmod(r, P->p[j] % m, m);
    return r;
  };
  P->yscale.assign(K, 0);
  P->w_ext.assign((size_t)(K + 1) * L, 0);
  P->w_md.assign((size_t)(K + 1) * L, 0);
  P->v.assign(L, 0);
  for (uint32_t j = 0; j < K; j++) {
    const uint64_t pj = P->p[j];
    P->yscale[j] = mulmod(P->scale % pj, inv(prod(j, pj), pj), pj);
  }
  for (uint32_t l = 0; l < L; l++) {
    const uint64_t ql = P->q[l], tinv = inv(P->scale, ql), Pm = prod(K, ql);
    for (uint32_t j = 0; j < K; j++) {
      const uint64_t ph = prod(j, ql);
      P->w_ext[(size_t)j * L + l] = ph;
      P->w_md[(size_t)j * L + l] = mulmod(ph, tinv, ql);
    }
    const uint64_t negP = (ql - Pm) % ql;
    P->w_ext[(size_t)K * L + l] = negP;
    P->w_md[(size_t)K * L + l] = mulmod(negP, tinv, ql);
    P->v[l] = mulmod(P->scale % ql, inv(Pm, ql), ql);
  }
}

// A call's status before any device access
inline int xconv_call_status(bool have_ctx, const void *out, const void *in, size_t batch) {
  if (!have_ctx) return NTTMUL_EINVAL;
  if (batch && (!out || !in)) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

// The shape of a call's sub-batches: mdntt_shape's (the scratch holds y [cnt][K][n] and, above
// n = 4096, the column-passed sums [cnt][L][n]); extend's input has the K limbs of P only
inline MdShape xconv_shape(size_t limit, uint32_t n, uint32_t L, uint32_t K, int word_bits,
                           size_t batch, int op) {
  MdShape S = mdntt_shape(limit, n, L, K, word_bits, batch);
  if (op == kXcExtend) S.in_words = (size_t)K * n;
  return S;
}

}  // namespace nttmul
