// ksntt.hpp — internal interface between the host entry points of include/nttmul_ksntt.h
// (ksntt.cpp) and the launchers of ksntt.hip.  lib/libnttmul_ksntt.so only.
#pragma once
#include "hoist.hpp"
#include "mdntt.hpp"
#include "nttmul_ksntt.h"

namespace nttmul {

enum KsnttOp { kKsnttModup = 0, kKsnttMac = 1 };

// Per-device view of a context: what a launch needs (pointers are device memory).  M = L + K.
struct KsnttTables {
  uint32_t logn = 0, L = 0, K = 0, alpha = 0, dnum = 0;
  int word_bits = 0;
  const void *tab_fwd = nullptr;  // KParams<A>[M], make_params, the extended basis Q u P
  const void *tab_inv = nullptr;  // KParams<A>[L], Q's limbs with the scale n^-1 Dh_i^-1
  const void *tw = nullptr;       // the M limbs' twiddles: fw of limb l at pair 2 l n, iw after it
  const void *to = nullptr;       // BconvTo<W>[bconv_pad(M)]: c, -c^-1, R mod c, the pair of R mod c
  const void *w = nullptr;        // W[L][bconv_pad(M)]: Dh_i R mod m
};

// modup's scratch is mdntt.hpp's MdScratch: scr[kMdY] y [cnt][L][n], and above n = 4096
// scr[kMdYLazy] the inverse rows' lazy words [cnt][L][n].  scr[kMdT] is not used: the
// column-passed sums go through up_hat (ksntt_dev.hpp).

// The launches of one sub-batch of modup on stream s: x_hat [cnt][L][n] ->
// up_hat [cnt][dnum][M][n]
hipError_t launch_ksntt_modup(const KsnttTables &T, void *up_hat, const void *x_hat, size_t cnt,
                              void *const *scr, hipStream_t s);
// The one launch of mac: a_hat [batch][terms][M][n], b_hat [rots][comps][terms][M][n] ->
// c_hat [batch][rots][comps][M][n]
hipError_t launch_ksntt_mac(const KsnttTables &T, void *c_hat, const void *a_hat,
                            const void *b_hat, const HoistArgs &H, size_t batch, uint32_t terms,
                            hipStream_t s);
// The kernels a sub-batch of `op` launches for T, joined by " + ": the dry run of the launching
// statements themselves (kernels_dev.hpp Emit)
hipError_t describe_ksntt(const KsnttTables &T, int op, uint32_t comps, std::string *out);

// A key operand read through a level view (include/nttmul_level.h, lib/libnttmul_level.so): its
// address arithmetic (level_plan.hpp) and the range check over exactly the words the view selects.
// level.cpp supplies the functions; they are not in this library.
struct LevelAddr;
using LevelCheck = int (*)(char *err, int *flag, const uint64_t *q, int word_bits, const void *op,
                           const LevelAddr &A, size_t outer, uint32_t terms, bool has_terms,
                           const char *msg, hipStream_t s);
// mac with b_hat viewed: `check` in place of the range check of b_hat, `launch` in place of
// launch_ksntt_mac, b_words the whole viewed operand (what the host form stages)
struct KsnttViewed {
  const LevelAddr *addr;
  size_t b_words;
  LevelCheck check;
  hipError_t (*launch)(const KsnttTables &T, void *c_hat, const void *a_hat, const void *b_hat,
                       const HoistArgs &H, size_t batch, uint32_t terms, const LevelAddr &A,
                       hipStream_t s);
};
// nttmul_ksntt_mac (host != 0; dev and stream unused) or nttmul_ksntt_mac_device with V for b_hat:
// the same argument checks, device selection, range check of a_hat and error text
int ksntt_mac_viewed(nttmul_ksntt *h, const KsnttViewed &V, void *c_hat, const void *a_hat,
                     const void *b_hat, const uint32_t *k, uint32_t rots, size_t batch,
                     uint32_t terms, uint32_t comps, int host, int dev, void *stream);

}  // namespace nttmul
