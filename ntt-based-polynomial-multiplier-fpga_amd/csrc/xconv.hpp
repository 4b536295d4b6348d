// xconv.hpp — internal interface between the host entry points of include/nttmul_xconv.h
// (xconv.cpp) and the launchers of xconv.hip.  lib/libnttmul_xconv.so only.
#pragma once
#include "mdntt.hpp"
#include "xconv_plan.hpp"

namespace nttmul {

// Per-device view of a context: what a sub-batch's launches need (pointers are device memory).
struct XcTables {
  uint32_t logn = 0, L = 0, K = 0;
  int word_bits = 0;
  const void *tab_fwd = nullptr;  // KParams<A>[L + K], make_params: the forward kernels read l < L
  const void *tab_inv = nullptr;  // KParams<A>[K], P's limbs with the scale n^-1 Ph_j^-1 t
  const void *tw = nullptr;       // the L + K limbs' twiddles: fw of limb l at pair 2 l n, iw after it
  const void *to = nullptr;       // BconvTo<W>[bconv_pad(L)], its factor t P^-1 mod q_l
  const void *w[2] = {nullptr, nullptr};  // per XcOp, W[K + 1][bconv_pad(L)]: the weights R mod q_l
  const double *ip = nullptr;     // [K]: 1 / p_j
};

// The launches of one sub-batch of `op` on stream s, through mdntt.hpp's scratch buffers:
// kXcExtend p_hat [cnt][K][n] -> out [cnt][L][n]; kXcModdown x_hat [cnt][L + K][n] -> out
// [cnt][L][n]
hipError_t launch_xconv(const XcTables &T, int op, void *out, const void *in, size_t cnt,
                        void *const *scr, hipStream_t s);
// The kernels launch_xconv launches for (T, op), joined by " + ": the dry run of the launching
// statements themselves (kernels_dev.hpp Emit)
hipError_t describe_xconv(const XcTables &T, int op, std::string *out);

}  // namespace nttmul
