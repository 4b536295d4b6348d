// tmd.hpp — internal interface between the host entry points of include/nttmul_tmd.h (tmd.cpp)
// and the launchers of tmd.hip.  lib/libnttmul_tmd.so only.
#pragma once
#include "mdntt.hpp"
#include "tmd_plan.hpp"

namespace nttmul {

// Per-device view of a context: what a sub-batch's launches need (pointers are device memory).
struct TmTables {
  uint32_t logn = 0, L = 0, K = 0;
  int word_bits = 0;
  const void *tab_fwd = nullptr;  // KParams<A>[L + K], make_params: the forward kernels read l < L
  const void *tab_inv = nullptr;  // KParams<A>[K], P's limbs with the scale n^-1 Ph_j^-1
  const void *tw = nullptr;       // the L + K limbs' twiddles: fw of limb l at pair 2 l n, iw after it
  const void *to = nullptr;       // BconvTo<W>[bconv_pad(L)], its factor P^-1 mod q_l
  const void *w = nullptr;        // W[K + 2][bconv_pad(L)]: Ph_j R, then P R and -P R, mod q_l
  const void *tt = nullptr;       // BconvTo<W>[bconv_pad(1)]: the plaintext modulus' entry
  const void *g = nullptr;        // W[K][bconv_pad(1)]: g_j R mod t in column 0
};

// The launches of one sub-batch on stream s, through mdntt.hpp's scratch buffers:
// x_hat [cnt][L + K][n] -> out [cnt][L][n]
hipError_t launch_tmd(const TmTables &T, void *out, const void *x_hat, size_t cnt,
                      void *const *scr, hipStream_t s);
// The kernels launch_tmd launches for T, joined by " + ": the dry run of the launching statements
// themselves (kernels_dev.hpp Emit)
hipError_t describe_tmd(const TmTables &T, std::string *out);

}  // namespace nttmul
