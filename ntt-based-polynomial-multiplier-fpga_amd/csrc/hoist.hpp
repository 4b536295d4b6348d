// hoist.hpp — internal interface between the host entry points of include/nttmul_hoist.h
// (hoist.cpp) and the launchers of hoist.hip.  lib/libnttmul_hoist.so only.  The launchers have
// the shapes rns.cpp and rnsmp.cpp call in place of their own (rns.hpp RnsMacLaunch, rnsmp.hpp
// MpUnitsLaunch), with a HoistArgs behind their `aux`.
#pragma once
#include "galois.hpp"
#include "rnsmp.hpp"

namespace nttmul {

// what a call passes through the context's runtime to its launcher
struct HoistArgs {
  GaloisKs ks;           // the rotations k_r themselves (not their inverses); 1 from rots on
  uint32_t rots, comps;
};

// One launch, k_rns_hoist<.., comps> (hoist_dev.hpp), grid (blocks over the batch times rots,
// limbs): a = a_hat [batch][terms][limbs][n], b = b_hat [rots][comps][terms][limbs][n],
// c [batch][rots][comps][limbs][n]; n <= 4096.  comps_all = rots comps (what the context's
// runtime sizes c and b_hat by), shared != 0, aux: the call's HoistArgs
hipError_t launch_rns_hoist(const RnsTables &T, void *c, const void *a, const void *b,
                            size_t batch, uint32_t terms, uint32_t comps_all, int shared,
                            hipStream_t s, const void *aux);
// "k_rns_hoist<Arith32P,u32,12,2>": the dry run of the launching statement itself
hipError_t describe_rns_hoist(const RnsTables &T, uint32_t comps, std::string *out);

// Two launches over the sub-batch of output units [u0, u0 + cnt) of a call, 4096 < n <= 65536:
// k_rnsmp_hoist<.., comps> into scr[2] ([cnt comps][limbs][n]) and k_rnsmp_cols_inv over
// cnt comps units into c, which addresses the sub-batch's first word.  a and b address the whole
// operands.  aux: the call's HoistArgs
hipError_t launch_rnsmp_hoist(const RnsTables &T, void *c, const void *a, const void *b, size_t u0,
                              size_t cnt, uint32_t terms, const void *aux, void *const *scr,
                              hipStream_t s);
// the two names joined by " + "
hipError_t describe_rnsmp_hoist(const RnsTables &T, uint32_t comps, std::string *out);

}  // namespace nttmul
