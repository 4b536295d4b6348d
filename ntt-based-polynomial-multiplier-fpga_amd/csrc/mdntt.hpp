// mdntt.hpp — internal interface between the host entry points of include/nttmul_mdntt.h
// (mdntt.cpp) and the launchers of mdntt.hip.  lib/libnttmul_mdntt.so only.
#pragma once
#include "bconv.hpp"
#include "rnsmp.hpp"

namespace nttmul {

// Per-device view of a context: what a sub-batch's launches need (pointers are device memory).
struct MdTables {
  uint32_t logn = 0, L = 0, K = 0;
  int word_bits = 0;
  const void *tab_fwd = nullptr;  // KParams<A>[L + K], make_params: the forward kernels read l < L
  const void *tab_inv = nullptr;  // KParams<A>[K], P's limbs with the scale n^-1 Ph_j^-1
  const void *tw = nullptr;       // the L + K limbs' twiddles: fw of limb l at pair 2 l n, iw after it
  const void *to = nullptr;       // BconvTo<W>[bconv_pad(L)], from = P, to = Q
  const void *w = nullptr;        // W[K][bconv_pad(L)]: Ph_j R mod q_l
};

// The scratch buffers a sub-batch of cnt polynomials uses, in words of the context's class
enum MdScratch { kMdY = 0, kMdYLazy = 1, kMdT = 2, kMdScratch = 3 };
//   n <= 4096   scr[kMdY]      y [cnt][K][n]
//   n  > 4096   scr[kMdYLazy]  the inverse rows' lazy output [cnt][K][n]
//               scr[kMdY]      y [cnt][K][n]
//               scr[kMdT]      the column-passed r [cnt][L][n]

// The launches of one sub-batch on stream s: x_hat [cnt][L + K][n] -> out [cnt][L][n]
hipError_t launch_mdntt(const MdTables &T, void *out, const void *x_hat, size_t cnt,
                        void *const *scr, hipStream_t s);
// The inverse half of launch_mdntt alone: the limbs L .. L + K - 1 of x_hat [cnt][L + K][n] -> y
// [cnt][K][n] in scr[kMdY], coefficient order, canonical, scaled by what tab_inv folds
// (k_mdntt_inv, or k_mdntt_inv_rows through scr[kMdYLazy] and k_rnsmp_cols_inv).  L = 0 reads a
// compact [cnt][K][n] operand: what the ModUp of include/nttmul_ksntt.h inverts (ksntt.cpp).
// With `describe` set nothing is launched and the kernels' names are appended to it.
hipError_t launch_mdntt_inverse(const MdTables &T, const void *x_hat, size_t cnt,
                                void *const *scr, hipStream_t s, std::string *describe);
// The last launch of launch_mdntt above n = 4096 alone: k_mdntt_rows on the column-passed sums in
// scr[kMdT] ([cnt][L][n], lazy words), with the epilogue's factor read from T.to.  What the
// rounded ModDown of include/nttmul_xconv.h ends in (xconv.hip), its T.to carrying t P^-1.
// With `describe` set nothing is launched and the kernel's name is appended to it.
hipError_t launch_mdntt_rows(const MdTables &T, void *out, const void *x_hat, size_t cnt,
                             void *const *scr, hipStream_t s, std::string *describe);
// The kernels launch_mdntt launches for T, joined by " + ": the dry run of the launching
// statements themselves (kernels_dev.hpp Emit)
hipError_t describe_mdntt(const MdTables &T, std::string *out);

}  // namespace nttmul
