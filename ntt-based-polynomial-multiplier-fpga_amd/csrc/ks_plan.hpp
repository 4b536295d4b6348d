// ks_plan.hpp — what ks.cpp shares with the host-only entry point of include/nttmul_ks.h
// (ks_plan.cpp): the validation of a key-switch basis and its plain constants.  Plain C++: no HIP
// header.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "nttmul.h"

namespace nttmul {

// The plain constants of a key-switch context (nttmul_ks_plan)
struct KsPlan {
  uint32_t n = 0, logn = 0, L = 0, K = 0, alpha = 0, dnum = 0, flags = 0;
  int word_bits = 0;
  nttmul_params prm = {};               // the caller's params, zero-extended (create: the devices)
  std::vector<uint64_t> q, p;           // Q [L], P [K]
  std::vector<uint64_t> inv, w, gadget; // [L], [L][L + K], [dnum][L + K]
  std::vector<uint64_t> pinv, pw, Pinv; // [K], [K][L], [L]: the converter from = P, to = Q
  // the m-th modulus of the extended basis q_0 .. q_{L-1}, p_0 .. p_{K-1}
  uint64_t modulus(uint32_t m) const { return m < L ? q[m] : p[m - L]; }
};

// What create and plan decide before any device access; on success n .. word_bits, q and p are set
int ks_validate(const nttmul_params *caller, size_t size, const uint64_t *q, uint32_t L,
                const uint64_t *p, uint32_t K, uint32_t digit_limbs, KsPlan *P);
// inv .. Pinv of a validated plan
void ks_constants(KsPlan *P);

}  // namespace nttmul
