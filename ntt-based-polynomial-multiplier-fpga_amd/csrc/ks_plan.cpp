// ks_plan.cpp — the host-only part of include/nttmul_ks.h (lib/libnttmul_ks.so only):
// nttmul_ks_plan, and the validation and plain constants ks.cpp shares with it.  The constants
// come from the planner's modular arithmetic (planner.hpp mulmod / powmod) in 128-bit host
// integers.  The checks every limb-aware library makes are basis.cpp's; ks_validate keeps the
// digit width's between their two steps.  Plain C++ without a HIP header, so
// tests/sanitize/ks_san.cpp builds this file as it stands (with basis.cpp and planner.cpp) under
// ASan / UBSan.
#include "ks_plan.hpp"

#include <string.h>

#include "basis.hpp"
#include "nttmul_ks.h"
#include "planner.hpp"

namespace nttmul {

// In nttmul_galois_create's order (basis.hpp): every EINVAL of either basis and of the digit width
// first, then the unsupported shapes, then the word classes
int ks_validate(const nttmul_params *caller, size_t size, const uint64_t *q, uint32_t L,
                const uint64_t *p, uint32_t K, uint32_t digit_limbs, KsPlan *P) {
  const uint64_t *const bases[2] = {q, p};
  const uint32_t limbs[2] = {L, K};
  BasisRequest B;
  // a degree above 65536 is valid and unsupported
  if (const int st = basis_invalid(caller, size, bases, limbs, 2, 1u << 30, &B)) return st;
  // the extended basis is one nttmul_rns / nttmul_rnsmp context's
  if (digit_limbs == 0 || digit_limbs > L || L + K > NTTMUL_RNS_MAX_LIMBS) return NTTMUL_EINVAL;
  // (p3_fold: what nttmul_rns_create asks of a 32-bit basis at n = 4096)
  if (const int st = basis_unsupported(&B, 256, 65536, true)) return st;
  P->prm = B.prm;
  P->n = B.prm.n;
  P->logn = (uint32_t)__builtin_ctz(P->n);
  P->L = L;
  P->K = K;
  P->alpha = digit_limbs;
  P->dnum = (L + digit_limbs - 1) / digit_limbs;
  P->flags = B.prm.flags;
  P->word_bits = B.word_bits;
  P->q.assign(q, q + L);
  P->p.assign(p, p + K);
  return NTTMUL_OK;
}

namespace {

uint64_t invmod(uint64_t a, uint64_t m) { return powmod(a % m, m - 2, m); }  // m prime

// the product of b[lo .. hi) without b[skip] (skip >= hi: of all of them), mod m
uint64_t prod_mod(const std::vector<uint64_t> &b, uint32_t lo, uint32_t hi, uint32_t skip,
                  uint64_t m) {
  uint64_t v = 1 % m;
  for (uint32_t i = lo; i < hi; i++)
    if (i != skip) v = mulmod(v, b[i] % m, m);
  return v;
}

}  // namespace

void ks_constants(KsPlan *P) {
  const uint32_t L = P->L, K = P->K, M = L + K, a = P->alpha;
  P->inv.assign(L, 0);
  P->w.assign((size_t)L * M, 0);
  P->gadget.assign((size_t)P->dnum * M, 0);
  P->pinv.assign(K, 0);
  P->pw.assign((size_t)K * L, 0);
  P->Pinv.assign(L, 0);
  for (uint32_t i = 0; i < L; i++) {
    // Dh_i = D_d / q_i over the limbs of i's digit
    const uint32_t lo = i / a * a, hi = lo + a < L ? lo + a : L;
    P->inv[i] = invmod(prod_mod(P->q, lo, hi, i, P->q[i]), P->q[i]);
    for (uint32_t m = 0; m < M; m++)
      P->w[(size_t)i * M + m] = prod_mod(P->q, lo, hi, i, P->modulus(m));
  }
  // G_d = P (Q / D_d) ((Q / D_d)^-1 mod D_d).  (Q / D_d) t with t = (Q / D_d)^-1 mod D_d is 1 mod
  // every q_m of the digit and 0 mod every other q_m, whatever representative t is; and P is 0
  // mod every p_j.  So G_d is P mod q_m on the digit's own limbs and 0 on all others.
  for (uint32_t d = 0; d < P->dnum; d++)
    for (uint32_t m = d * a; m < (d + 1) * a && m < L; m++)
      P->gadget[(size_t)d * M + m] = prod_mod(P->p, 0, K, K, P->q[m]);
  for (uint32_t j = 0; j < K; j++) {
    P->pinv[j] = invmod(prod_mod(P->p, 0, K, j, P->p[j]), P->p[j]);
    for (uint32_t i = 0; i < L; i++) P->pw[(size_t)j * L + i] = prod_mod(P->p, 0, K, j, P->q[i]);
  }
  for (uint32_t i = 0; i < L; i++) P->Pinv[i] = invmod(prod_mod(P->p, 0, K, K, P->q[i]), P->q[i]);
}

}  // namespace nttmul

using namespace nttmul;

extern "C" {

int nttmul_ks_plan(const nttmul_params *params, size_t size, const uint64_t *q, uint32_t q_limbs,
                   const uint64_t *p, uint32_t p_limbs, uint32_t digit_limbs, uint64_t *inv,
                   uint64_t *w, uint64_t *gadget, uint64_t *pinv, uint64_t *pw, uint64_t *Pinv) {
  KsPlan P;
  if (const int st = ks_validate(params, size, q, q_limbs, p, p_limbs, digit_limbs, &P)) return st;
  ks_constants(&P);
  const auto copy = [](uint64_t *dst, const std::vector<uint64_t> &src) {
    if (dst) memcpy(dst, src.data(), sizeof(uint64_t) * src.size());
  };
  copy(inv, P.inv);
  copy(w, P.w);
  copy(gadget, P.gadget);
  copy(pinv, P.pinv);
  copy(pw, P.pw);
  copy(Pinv, P.Pinv);
  return NTTMUL_OK;
}

}  // extern "C"
