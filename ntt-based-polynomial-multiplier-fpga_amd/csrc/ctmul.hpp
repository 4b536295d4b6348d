// ctmul.hpp — internal interface between the host entry points of include/nttmul_ctmul.h
// (ctmul.cpp) and the launchers of ctmul.hip.  lib/libnttmul_ctmul.so only.
#pragma once
#include "ctmul_plan.hpp"
#include "ksntt.hpp"

namespace nttmul {

// The constant of one limb of Q beyond its BconvTo entry: P R mod q_l in the form mont takes (the
// canonical word), so that mont(e, pr) = P e R^-1 carries the power of R the key sum carries
template <class W>
struct CtLimb {
  W pr;
};

// Per-device view of a context: what a launch needs (pointers are device memory).  M = L + K.
struct CtTables {
  uint32_t logn = 0, L = 0, K = 0;
  int word_bits = 0;
  const void *to = nullptr;    // BconvTo<W>[bconv_pad(M)]: m, -m^-1, R mod m, the pair of R mod m
  const void *limb = nullptr;  // CtLimb<W>[L]
};

// high: x_hat, y_hat [batch][pairs][2][L][n] -> d2_hat [batch][L][n]
hipError_t launch_ctmul_high(const CtTables &T, void *d2_hat, const void *x_hat, const void *y_hat,
                             size_t batch, uint32_t pairs, hipStream_t s);
// relin: up_hat [batch][terms][M][n], key_hat [2][terms][M][n], x_hat, y_hat as above
// -> c_hat [batch][2][M][n]
hipError_t launch_ctmul_relin(const CtTables &T, void *c_hat, const void *up_hat,
                              const void *key_hat, const void *x_hat, const void *y_hat,
                              size_t batch, uint32_t pairs, uint32_t terms, hipStream_t s);
// "k_ctmul_high<Arith64,u64>" / "k_ctmul_relin<Arith64,u64>": the dry run of the launching
// statement itself
hipError_t describe_ctmul(const CtTables &T, int op, std::string *out);

// relin with key_hat viewed (ksntt.hpp KsnttViewed's shape): `check` in place of its range check,
// `launch` in place of launch_ctmul_relin, key_words the whole viewed operand (what the host form
// stages)
struct CtViewed {
  const LevelAddr *addr;
  size_t key_words;
  LevelCheck check;
  hipError_t (*launch)(const CtTables &T, void *c_hat, const void *up_hat, const void *key_hat,
                       const void *x_hat, const void *y_hat, size_t batch, uint32_t pairs,
                       uint32_t terms, const LevelAddr &A, hipStream_t s);
};
// nttmul_ctmul_relin (host != 0; dev and stream unused) or nttmul_ctmul_relin_device with V for
// key_hat: the same argument checks, device selection, range checks of the other operands and
// error text
int ctmul_relin_viewed(nttmul_ctmul *h, const CtViewed &V, void *c_hat, const void *up_hat,
                       const void *key_hat, const void *x_hat, const void *y_hat, size_t batch,
                       uint32_t pairs, uint32_t terms, int host, int dev, void *stream);

}  // namespace nttmul
