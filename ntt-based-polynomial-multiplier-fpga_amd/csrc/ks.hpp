// ks.hpp — internal interface between the host entry points of include/nttmul_ks.h (ks.cpp) and
// the launcher of ks.hip.  lib/libnttmul_ks.so only.
#pragma once
#include "bconv.hpp"

namespace nttmul {

enum KsOp { kKsModup = 0, kKsModdown = 1 };

// Per-device view of a key-switch context's ModUp: what a launch needs (pointers are device
// memory).  The tables are k_bconv's (bconv.hpp), over the extended basis of M = L + K limbs.
struct KsTables {
  uint32_t logn = 0, q_limbs = 0, p_limbs = 0, digit_limbs = 0, digits = 0;
  int word_bits = 0;
  const void *from = nullptr;  // BconvFrom<W>[L]: q_i and Dh_i^-1 mod q_i (a limb is in one digit)
  const void *to = nullptr;    // BconvTo<W>[bconv_pad(M)], the padding repeats the last
  const void *w = nullptr;     // W[L][bconv_pad(M)]: Dh_i R mod m-th modulus, padding 0
};

// One launch on stream s: in [batch][L][n] -> out [batch][dnum][M][n], grid = (workgroups, dnum)
hipError_t launch_ks_modup(const KsTables &T, void *out, const void *in, size_t batch,
                           hipStream_t s);
// The kernel launch_ks_modup launches for T, as "k_ks_modup<u32>": the dry run of the launching
// statement itself (kernels_dev.hpp Emit)
hipError_t describe_ks_modup(const KsTables &T, std::string *out);

}  // namespace nttmul
