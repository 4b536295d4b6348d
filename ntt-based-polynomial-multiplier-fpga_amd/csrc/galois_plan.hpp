// galois_plan.hpp — the index arithmetic galois.cpp shares with the host-only entry points of
// include/nttmul_galois.h (galois_plan.cpp).  Plain C++: no HIP header.
#pragma once
#include <stdint.h>

namespace nttmul {

// an automorphism of degree n: odd and below 2n
bool galois_k_ok(uint32_t n, uint32_t k);
// k^-1 mod 2n for such a k (n a power of two, 2n <= 2^17)
uint32_t galois_inv_mod_2n(uint32_t n, uint32_t k);

}  // namespace nttmul
