// rns.hpp — internal interface between the host entry points of include/nttmul_rns.h (rns.cpp)
// and the launchers of rns.hip, and the host pieces rns.cpp shares with rnsmp.cpp.
// lib/libnttmul_rns.so only.
#pragma once
#include <vector>

#include "launch.hpp"

struct nttmul_rns;  // include/nttmul_rns.h; defined in rns.cpp

namespace nttmul {

// The kernel families of an RNS context.  Each reads its own per-device table of KParams<A>, one
// entry per limb, because the scale folded into the last inverse stage differs:
//   kRnsProduct    F 2^D  (kernels_dev.hpp product_params; D = 3 at n = 4096 with 32-bit words)
//   kRnsTransform  F      (make_params: the mac's inverse; the forward transform reads no scale)
//   kRnsInverse    n^-1   (the fi / wfi pairs of the standalone inverse)
enum RnsFamily { kRnsProduct = 0, kRnsTransform = 1, kRnsInverse = 2, kRnsFamilies = 3 };
enum RnsOp { kRnsMultiply = 0, kRnsForward = 1, kRnsInverseOp = 2, kRnsMac = 3 };

// Per-device view of an RNS context: what a launch needs (pointers are device memory).
struct RnsTables {
  uint32_t logn = 0, limbs = 0;
  int word_bits = 0;                 // 32: every q_l < 2^31 (Arith32P / Arith32P3), 64: Arith64
  const void *tab[kRnsFamilies] = {nullptr, nullptr, nullptr};  // KParams<A>[limbs] each
  // the limbs' twiddle (value, companion) pairs in one allocation: fw of limb l at pair 2 l n,
  // iw at pair (2 l + 1) n (the pointers the table entries hold as well)
  const void *tw = nullptr;
  const uint64_t *q = nullptr;       // the moduli, [limbs] (range check)
};

// bytes of one table entry for words of word_bits (every class of a word size has one layout)
size_t rns_entry_bytes(int word_bits);
// The entry of family `fam` for one limb, from that limb's LaunchTables (fw / iw are the limb's
// device twiddle tables), written to host memory at dst.  hipErrorNotSupported for a modulus the
// family's arithmetic class does not take (Arith32P3's fold at n = 4096: arith_select.hpp
// p3_fold_ok, true for every q < 2^31 and checked all the same).
hipError_t rns_fill_entry(const LaunchTables &T, int fam, void *dst);

// One launch over a [batch][limbs][n] operand set on stream s (rns_dev.hpp), grid = (blocks over
// the batch, limbs).  op kRnsMultiply: c = a * b;  kRnsForward / kRnsInverseOp: c = transform(a),
// c == a allowed;  kRnsMac: a [batch][terms][limbs][n], b = b_hat [batch or 1][terms][limbs][n].
hipError_t launch_rns(const RnsTables &T, int op, void *c, const void *a, const void *b,
                      size_t batch, uint32_t terms, int shared, hipStream_t s);
// The kernel launch_rns launches for (T, op), as "k_rns_rows<Arith32P3,u32,12>": the dry run of
// the launching statement itself (kernels_dev.hpp Emit)
hipError_t describe_rns(const RnsTables &T, int op, std::string *out);
// *bad |= 1 when a word i < total of a is >= q[(i / n) mod limbs]
hipError_t launch_rns_check(const RnsTables &T, const void *a, size_t total, int *bad,
                            hipStream_t s);

// ---- host side, shared by rns.cpp (which defines it) and rnsmp.cpp ------------------------------

struct Plan;     // planner.hpp
struct LimbDev;  // limb_ctx.hpp

// One limb's LaunchTables from its plan; fw / iw: the limb's device twiddle tables
LaunchTables limb_tables(const Plan &P, const void *fw, const void *iw);
// The view of one device of a context, from the fields both contexts keep
RnsTables tables_for(uint32_t logn, uint32_t limbs, int word_bits, const void *tw,
                     void *const tab[kRnsFamilies], const uint64_t *q);
// What a call decides before any device access (have_ctx: the handle is not NULL)
int op_args(bool have_ctx, int op, const void *c, const void *a, const void *b, size_t batch,
            uint32_t terms);
// words of the operands of one call: c, a, b (b 0 for the transforms).  comps: the mac's b_hat
// components per term, each with an output polynomial of its own (1 but for macn.cpp)
void op_words(uint32_t limbs, uint32_t n, int op, size_t batch, uint32_t terms, int shared,
              size_t words[3], uint32_t comps = 1);
// One device's stream, moduli, flag and tables at create: the limbs' twiddles in one allocation
// *tw (fw, iw of limb 0, fw, iw of limb 1, ...), then the three KParams tables tab[] that `fill`
// (rns_fill_entry or rnsmp_fill_entry) builds from pointers into it
int upload_limb_tables(char *err, const std::vector<Plan> &plan, int word_bits, LimbDev &d,
                       void **tw, void *tab[kRnsFamilies],
                       hipError_t (*fill)(const LaunchTables &, int, void *));


// ---- for a sibling library that adds a mac kernel on the same context (macn.cpp and later) ------

// launch_rns's place in a call: c [batch][comps][limbs][n], b = b_hat
// [batch or 1][comps][terms][limbs][n].  aux: the caller's own, passed through unread.
// Convention for a sibling whose output has more structure than components (hoist.cpp: rots
// rotations of comps components against one shared b_hat [rots][comps][terms][limbs][n]): it
// passes comps = rots comps and shared = 1, so that op_words sizes c as
// [batch][rots comps][limbs][n] and b_hat as [rots comps][terms][limbs][n] for the range check and
// the host form, and carries the split (rots, comps, the rotations) behind aux for its launcher
using RnsMacLaunch = hipError_t (*)(const RnsTables &T, void *c, const void *a, const void *b,
                                    size_t batch, uint32_t terms, uint32_t comps, int shared,
                                    hipStream_t s, const void *aux);
// nttmul_rns_mac_ntt (host != 0; dev and stream unused) or nttmul_rns_mac_ntt_device with `comps`
// operands per term and `launch` for the launch: the same argument checks, device selection,
// range check (over all of b_hat) and error text
int rns_mac_comps(nttmul_rns *r, RnsMacLaunch launch, void *c, const void *a, const void *b_hat,
                  size_t batch, uint32_t terms, uint32_t comps, int shared, int host, int dev,
                  void *stream, const void *aux = nullptr);

}  // namespace nttmul
