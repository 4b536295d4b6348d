// basis.cpp — the create-time checks of the limb-aware libraries (basis.hpp).  Host only.
#include "basis.hpp"

#include <string.h>

#include "nttmul_rns.h"
#include "planner.hpp"

namespace nttmul {

int basis_invalid(const nttmul_params *caller, size_t size, const uint64_t *const *q,
                  const uint32_t *limbs, int bases, uint32_t max_degree, BasisRequest *R) {
  if (!caller || size < NTTMUL_PARAMS_BASE_SIZE || size > sizeof(nttmul_params))
    return NTTMUL_EINVAL;
  nttmul_params &p = R->prm;
  memset(&p, 0, sizeof(p));
  memcpy(&p, caller, size);
  for (int i = 0; i < bases; i++)
    if (!q[i] || limbs[i] == 0 || limbs[i] > NTTMUL_RNS_MAX_LIMBS) return NTTMUL_EINVAL;
  if (p.q || p.psi) return NTTMUL_EINVAL;
  const uint32_t n = p.n;
  if (n < 256 || n > max_degree || (n & (n - 1))) return NTTMUL_EINVAL;
  R->all.clear();
  for (int i = 0; i < bases; i++) R->all.insert(R->all.end(), q[i], q[i] + limbs[i]);
  for (size_t l = 0; l < R->all.size(); l++) {
    const uint64_t m = R->all[l];
    if (m < 3 || m >= (1ull << 62) || (m - 1) % (2ull * n) || !is_prime(m)) return NTTMUL_EINVAL;
    for (size_t k = 0; k < l; k++)
      if (R->all[k] == m) return NTTMUL_EINVAL;
  }
  return NTTMUL_OK;
}

int basis_unsupported(BasisRequest *R, uint32_t min_n, uint32_t max_n, bool p3_fold) {
  const uint32_t n = R->prm.n;
  if (n < min_n || n > max_n || (R->prm.flags & NTTMUL_FLAG_CYCLIC)) return NTTMUL_EUNSUPPORTED;
  // one word class per context: every q < 2^31 (32-bit words) or every q >= 2^32 (64-bit)
  const bool small = R->all[0] < (1ull << 31);
  for (const uint64_t m : R->all) {
    if (m >= (1ull << 31) && m < (1ull << 32)) return NTTMUL_EUNSUPPORTED;
    if ((m < (1ull << 31)) != small) return NTTMUL_EUNSUPPORTED;
    if (p3_fold && small && n == 4096 && !p3_fold_ok(m)) return NTTMUL_EUNSUPPORTED;
  }
  R->word_bits = small ? 32 : 64;
  return NTTMUL_OK;
}

}  // namespace nttmul
