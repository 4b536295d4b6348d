// rnsmp.hpp — internal interface between the host entry points of include/nttmul_rnsmp.h
// (rnsmp.cpp) and the launchers of rnsmp.hip.  lib/libnttmul_rnsmp.so only.  The kernel families,
// the operation numbers and the per-device view of a context are rns.hpp's (RnsFamily, RnsOp,
// RnsTables), with logn in 13 .. 16 here.
#pragma once
#include "rns.hpp"

namespace nttmul {

// The entry of family `fam` for one limb of a multi-pass context (logn 13 .. 16), written to host
// memory at dst; rns_entry_bytes(word_bits) bytes.  kRnsProduct is product_params of the row
// pass's class (plain Arith32P or Arith64: no Arith32P3 above n = 4096).
hipError_t rnsmp_fill_entry(const LaunchTables &T, int fam, void *dst);

// The launches of one operation over `batch` polynomials of a [batch][limbs][n] operand set on
// stream s (rnsmp_dev.hpp; grid = (blocks, limbs) each):
//   kRnsMultiply   k_rnsmp_cols_fwd<.., 2> + k_rnsmp_rows + k_rnsmp_cols_inv   scr[0], scr[1], scr[2]
//   kRnsForward    k_rnsmp_cols_fwd<.., 1> + k_rnsmp_xform<.., 0>              scr[0]
//   kRnsInverseOp  k_rnsmp_xform<.., 1> + k_rnsmp_cols_inv                     scr[0]
//   kRnsMac        k_rnsmp_cols_fwd<.., 1> over batch terms units + k_rnsmp_mac + k_rnsmp_cols_inv
//                  scr[0] (batch terms polynomials), scr[2]
// scr: device buffers of batch * limbs * n words each (scr[0] of the mac: times terms).
hipError_t launch_rnsmp(const RnsTables &T, int op, void *c, const void *a, const void *b,
                        size_t batch, uint32_t terms, int shared, void *const *scr, hipStream_t s);
// The kernels launch_rnsmp launches for (T, op), joined by " + ": the dry run of the launching
// statements themselves (kernels_dev.hpp Emit)
hipError_t describe_rnsmp(const RnsTables &T, int op, std::string *out);

}  // namespace nttmul
