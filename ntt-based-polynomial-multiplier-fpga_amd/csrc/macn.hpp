// macn.hpp — internal interface between the host entry points of include/nttmul_macn.h (macn.cpp)
// and the launchers of macn.hip.  lib/libnttmul_macn.so only.  The launchers have the shapes
// rns.cpp and rnsmp.cpp call in place of their own (rns.hpp RnsMacLaunch, rnsmp.hpp MpMacLaunch).
#pragma once
#include "rnsmp.hpp"

namespace nttmul {

// One launch, k_rns_macn<.., comps> (macn_dev.hpp), grid (blocks over the batch, limbs):
// a [batch][terms][limbs][n], b = b_hat [batch or 1][comps][terms][limbs][n],
// c [batch][comps][limbs][n]; n <= 4096, comps >= 2
hipError_t launch_rns_macn(const RnsTables &T, void *c, const void *a, const void *b, size_t batch,
                           uint32_t terms, uint32_t comps, int shared, hipStream_t s,
                           const void *aux);
// "k_rns_macn<Arith32P,u32,12,2>": the dry run of the launching statement itself
hipError_t describe_rns_macn(const RnsTables &T, uint32_t comps, std::string *out);

// Three launches over one sub-batch, 4096 < n <= 65536, comps >= 2: k_rnsmp_cols_fwd<.., 1> over
// batch terms units into scr[0], k_rnsmp_macn<.., comps> into scr[2] ([batch comps][limbs][n]),
// k_rnsmp_cols_inv over batch comps units into c
hipError_t launch_rnsmp_macn(const RnsTables &T, void *c, const void *a, const void *b,
                             size_t batch, uint32_t terms, uint32_t comps, int shared,
                             void *const *scr, hipStream_t s);
// the three names joined by " + "
hipError_t describe_rnsmp_macn(const RnsTables &T, uint32_t comps, std::string *out);

}  // namespace nttmul
