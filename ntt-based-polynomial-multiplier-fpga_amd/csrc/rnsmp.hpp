// rnsmp.hpp — internal interface between the host entry points of include/nttmul_rnsmp.h
// (rnsmp.cpp) and the launchers of rnsmp.hip.  lib/libnttmul_rnsmp.so only.  The kernel families,
// the operation numbers and the per-device view of a context are rns.hpp's (RnsFamily, RnsOp,
// RnsTables), with logn in 13 .. 16 here.
#pragma once
#include "rns.hpp"

struct nttmul_rnsmp;  // include/nttmul_rnsmp.h; defined in rnsmp.cpp

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

// ---- for a sibling library that adds a row pass on the same context (macn.hip, macn.cpp) --------

// The mac's column passes alone, as launch_rnsmp launches them (tab kRnsTransform): dir 0
// k_rnsmp_cols_fwd<.., 1> over `units` polynomials of caller memory `in` to the scratch `out`,
// dir 1 k_rnsmp_cols_inv over `units` polynomials of the scratch `in` to caller memory `out`.
// With `describe` set nothing is launched and the kernel's name is appended to it, " + " between
// names.
hipError_t launch_rnsmp_cols(const RnsTables &T, int dir, void *out, const void *in, size_t units,
                             hipStream_t s, std::string *describe);

// launch_rnsmp's place in a sub-batch: c [batch][comps][limbs][n], b = b_hat
// [batch or 1][comps][terms][limbs][n]; scr[0] holds batch terms polynomials, scr[2] batch comps
using MpMacLaunch = hipError_t (*)(const RnsTables &T, void *c, const void *a, const void *b,
                                   size_t batch, uint32_t terms, uint32_t comps, int shared,
                                   void *const *scr, hipStream_t s);
// nttmul_rnsmp_mac_ntt (host != 0; dev and stream unused) or nttmul_rnsmp_mac_ntt_device with
// `comps` operands per term and `launch` for a sub-batch's launches: the same argument checks,
// device selection, range check (over all of b_hat), scratch hand-over and error text.  The
// sub-batch (subbatch.hpp mp_chunk) also keeps comps output polynomials per batch entry within
// scratch_mb.
int rnsmp_mac_comps(nttmul_rnsmp *r, MpMacLaunch launch, void *c, const void *a, const void *b_hat,
                    size_t batch, uint32_t terms, uint32_t comps, int shared, int host, int dev,
                    void *stream);

// ---- for a sibling library whose row pass reads a from caller memory (no forward column pass) ----

// One sub-batch of a call whose output is `upb` units per batch entry of `comps` polynomials each:
// the units [u0, u0 + cnt) of the batch upb units of the call, c at the sub-batch's first word
// ([cnt][comps][limbs][n]), a and b the call's whole operands; scr[2] holds cnt comps
// polynomials and is the only scratch buffer the call may use.  aux: the caller's own, unread
using MpUnitsLaunch = hipError_t (*)(const RnsTables &T, void *c, const void *a, const void *b,
                                     size_t u0, size_t cnt, uint32_t terms, const void *aux,
                                     void *const *scr, hipStream_t s);
// A call c [batch][upb][comps][limbs][n] = f(a [batch][terms][limbs][n],
// b [upb][comps][terms][limbs][n]) (host != 0: host buffers; dev and stream unused) with the
// context's device selection, range check (over all of a and of b), scratch hand-over and error
// text.  The sub-batch is the largest count of units whose cnt comps polynomials fit scratch_mb
// (subbatch.hpp mp_chunk with no input buffer), never less than one.  The caller has checked the
// arguments: r, and with batch > 0 the operands, are not NULL; terms, upb, comps > 0.
int rnsmp_units_op(nttmul_rnsmp *r, MpUnitsLaunch launch, const void *aux, void *c, const void *a,
                   const void *b, size_t batch, uint32_t terms, uint32_t upb, uint32_t comps,
                   int host, int dev, void *stream);

}  // namespace nttmul
