// basis.hpp — what every limb-aware create (and the host-only *_plan entry points) decides about
// its moduli before any device access, once: rns.cpp, bconv.cpp, rnsmp.cpp, galois.cpp and
// ks_plan.cpp differ only in the bounds they pass.  Two steps, so that a library's own EINVALs
// (ks_plan.cpp: the digit width) stand between every shared EINVAL and every EUNSUPPORTED.
// Plain C++: no HIP header (tests/sanitize/ks_san.cpp builds basis.cpp under ASan / UBSan).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "nttmul.h"

namespace nttmul {

struct BasisRequest {
  nttmul_params prm;          // the caller's params, zero-extended to the size this build knows
  std::vector<uint64_t> all;  // the moduli of the one or two bases, taken together
  int word_bits = 0;          // set by basis_unsupported: 32 (every q < 2^31) or 64 (every q >= 2^32)
};

// Step 1, the EINVALs in this order: the params size; a null basis, a limb count of 0 or above
// NTTMUL_RNS_MAX_LIMBS, params q or psi set; a degree that is no power of two in 256 .. max_degree;
// then per modulus, over the `bases` (1 or 2) lists q[i] of limbs[i] moduli taken together: out of
// [3, 2^62), not 1 mod 2n, not prime (what planner.cpp make_plan refuses; psi = 0 always finds a
// root then), or equal to an earlier one.
int basis_invalid(const nttmul_params *caller, size_t size, const uint64_t *const *q,
                  const uint32_t *limbs, int bases, uint32_t max_degree, BasisRequest *R);

// Step 2, the EUNSUPPORTEDs in this order: a degree outside min_n .. max_n or
// NTTMUL_FLAG_CYCLIC; then per modulus: in the gap 2^31 .. 2^32, of another word class than the
// first, or (p3_fold, 32-bit words at n = 4096) failing Arith32P3's fold (arith_select.hpp
// p3_fold_ok: holds for every q < 2^31, kept as a checked assumption).
int basis_unsupported(BasisRequest *R, uint32_t min_n, uint32_t max_n, bool p3_fold);

}  // namespace nttmul
