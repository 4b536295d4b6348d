// ctlin.hpp — internal interface between the host entry points of include/nttmul_ctlin.h
// (ctlin.cpp) and the launchers of ctlin.hip.  lib/libnttmul_ctlin.so only.
#pragma once
#include "ctlin_plan.hpp"
#include "ctmul.hpp"

namespace nttmul {

// The constant of one limb beyond its BconvTo entry: R^2 mod q_l (the canonical word), so that
// mont(s, r2) = s R is the form in which mont(x, s R) = x s carries no power of R
template <class W>
struct ClLimb {
  W r2;
};

// Per-device view of a context: what a launch needs (pointers are device memory)
struct ClTables {
  uint32_t logn = 0, L = 0;
  int word_bits = 0;
  const void *to = nullptr;    // BconvTo<W>[bconv_pad(L)]: q, -q^-1, R mod q, the pair of R mod q
  const void *limb = nullptr;  // ClLimb<W>[L]
};

// The terms of one combine as the kernel takes them, by value in its arguments
struct ClTerms {
  const void *x[NTTMUL_CTLIN_MAX_TERMS];
  const void *w[NTTMUL_CTLIN_MAX_TERMS];
  uint32_t kind[NTTMUL_CTLIN_MAX_TERMS];
  uint32_t nterms;
  uint32_t plain;  // some term is PLAIN with an x: the accumulator at scale R^-1 is in use
};

// combine: every x [batch][comps][L][n] -> out [batch][comps][L][n]
hipError_t launch_ctlin_combine(const ClTables &T, void *out, const ClTerms &terms, size_t batch,
                                uint32_t comps, hipStream_t s);
// tensor: x_hat, y_hat [batch][pairs][2][L][n] -> d_hat [batch][3][L][n]
hipError_t launch_ctlin_tensor(const ClTables &T, void *d_hat, const void *x_hat,
                               const void *y_hat, size_t batch, uint32_t pairs, hipStream_t s);
// "k_ctlin_combine<Arith64,u64,2>" / "k_ctlin_tensor<Arith64,u64>": the dry run of the launching
// statement itself
hipError_t describe_ctlin(const ClTables &T, int op, uint32_t comps, std::string *out);

}  // namespace nttmul
