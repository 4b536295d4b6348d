// galois_plan.cpp — the host-only part of include/nttmul_galois.h (lib/libnttmul_galois.so only):
// nttmul_galois_element, nttmul_galois_plan and the index arithmetic galois.cpp shares with them.
// Plain C++ without a HIP header, so tests/sanitize/galois_san.cpp builds this file as it stands
// under ASan / UBSan.
#include "galois_plan.hpp"
#include "nttmul_galois.h"

namespace {

// a power of two in 256 .. 65536, and its log2
bool degree_ok(uint32_t n, uint32_t *logn) {
  if (n < 256 || n > 65536 || (n & (n - 1))) return false;
  uint32_t l = 0;
  while ((1u << l) < n) l++;
  *logn = l;
  return true;
}

// reversal of the low logn bits
uint32_t brv(uint32_t x, uint32_t logn) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < logn; i++) r |= ((x >> i) & 1u) << (logn - 1 - i);
  return r;
}

}  // namespace

namespace nttmul {

bool galois_k_ok(uint32_t n, uint32_t k) { return (k & 1) && k < 2 * n; }

// k^-1 mod 2n for odd k (2n a power of two <= 2^17): Newton's iteration doubles the correct low
// bits, 3 -> 6 -> 12 -> 24; unsigned wrap-around is the arithmetic mod 2^32
uint32_t galois_inv_mod_2n(uint32_t n, uint32_t k) {
  uint32_t x = k;  // k k = 1 mod 8
  for (int i = 0; i < 3; i++) x *= 2u - k * x;
  return x & (2 * n - 1);
}

}  // namespace nttmul

using namespace nttmul;

extern "C" {

int nttmul_galois_element(uint32_t n, int64_t step, int conjugate, uint32_t *k) {
  uint32_t logn;
  if (!k || !degree_ok(n, &logn)) return NTTMUL_EINVAL;
  const uint32_t mask = 2 * n - 1;
  // 5 has order n / 2 in the odd residues mod 2n: reduce the step to [0, n / 2)
  const int64_t ord = n / 2;
  int64_t e = step % ord;
  if (e < 0) e += ord;
  uint32_t r = 1, b = 5;
  for (; e; e >>= 1) {
    if (e & 1) r = (r * b) & mask;
    b = (b * b) & mask;
  }
  if (conjugate) r = (r * mask) & mask;
  *k = r;
  return NTTMUL_OK;
}

int nttmul_galois_plan(uint32_t n, uint32_t k, uint32_t *coeff_src, uint8_t *coeff_neg,
                       uint32_t *ntt_src) {
  uint32_t logn;
  if (!degree_ok(n, &logn) || !galois_k_ok(n, k)) return NTTMUL_EINVAL;
  const uint32_t mask = 2 * n - 1, kinv = galois_inv_mod_2n(n, k);
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t i0 = (j * kinv) & mask;
    if (coeff_src) coeff_src[j] = i0 & (n - 1);
    if (coeff_neg) coeff_neg[j] = i0 >= n;
    if (ntt_src) {
      const uint32_t e = (k * (2 * brv(j, logn) + 1)) & mask;
      ntt_src[j] = brv(e >> 1, logn);
    }
  }
  return NTTMUL_OK;
}

}  // extern "C"
