// macn.cpp — host entry points of include/nttmul_macn.h (lib/libnttmul_macn.so only): the mac
// against `comps` NTT-domain operands on the existing contexts nttmul_rns and nttmul_rnsmp.  It has
// no handle and no state of its own.  The status of the arguments is macn_plan.hpp's; everything
// after it -- the device selection, the range check, the staged host form, the multi-pass
// context's sub-batches and scratch hand-over, the error text -- is the context's own mac_ntt
// path (rns.cpp rns_mac_comps, rnsmp.cpp rnsmp_mac_comps) with macn.hip's launches in place of
// its own.  comps = 1 is the context's mac_ntt itself.
#include <hip/hip_runtime.h>

#include <string>

#include "limb_ctx.hpp"
#include "macn.hpp"
#include "macn_plan.hpp"

using namespace nttmul;

namespace {

// what a dry run reads of a context: its degree and word class
RnsTables name_view(uint32_t logn, uint32_t limbs, uint32_t word_bits) {
  RnsTables T;
  T.logn = logn;
  T.limbs = limbs;
  T.word_bits = (int)word_bits;
  return T;
}

}  // namespace

extern "C" {

int nttmul_rns_macn_ntt_device(nttmul_rns *r, void *c, const void *a, const void *b_hat,
                               size_t batch, uint32_t terms, uint32_t comps, int shared, int dev,
                               void *stream) {
  if (const int st = macn_args(r != nullptr, c, a, b_hat, batch, terms, comps)) return st;
  if (comps == 1)
    return nttmul_rns_mac_ntt_device(r, c, a, b_hat, batch, terms, shared, dev, stream);
  return rns_mac_comps(r, launch_rns_macn, c, a, b_hat, batch, terms, comps, shared, 0, dev,
                       stream);
}

int nttmul_rnsmp_macn_ntt_device(nttmul_rnsmp *r, void *c, const void *a, const void *b_hat,
                                 size_t batch, uint32_t terms, uint32_t comps, int shared, int dev,
                                 void *stream) {
  if (const int st = macn_args(r != nullptr, c, a, b_hat, batch, terms, comps)) return st;
  if (comps == 1)
    return nttmul_rnsmp_mac_ntt_device(r, c, a, b_hat, batch, terms, shared, dev, stream);
  return rnsmp_mac_comps(r, launch_rnsmp_macn, c, a, b_hat, batch, terms, comps, shared, 0, dev,
                         stream);
}

int nttmul_rns_macn_ntt(nttmul_rns *r, void *c, const void *a, const void *b_hat, size_t batch,
                        uint32_t terms, uint32_t comps, int shared) {
  if (const int st = macn_args(r != nullptr, c, a, b_hat, batch, terms, comps)) return st;
  if (comps == 1) return nttmul_rns_mac_ntt(r, c, a, b_hat, batch, terms, shared);
  return rns_mac_comps(r, launch_rns_macn, c, a, b_hat, batch, terms, comps, shared, 1, 0,
                       nullptr);
}

int nttmul_rnsmp_macn_ntt(nttmul_rnsmp *r, void *c, const void *a, const void *b_hat, size_t batch,
                          uint32_t terms, uint32_t comps, int shared) {
  if (const int st = macn_args(r != nullptr, c, a, b_hat, batch, terms, comps)) return st;
  if (comps == 1) return nttmul_rnsmp_mac_ntt(r, c, a, b_hat, batch, terms, shared);
  return rnsmp_mac_comps(r, launch_rnsmp_macn, c, a, b_hat, batch, terms, comps, shared, 1, 0,
                         nullptr);
}

int nttmul_rns_macn_kernel_name(const nttmul_rns *r, uint32_t comps, char *buf, size_t cap) {
  if (!r || !comps || comps > NTTMUL_MACN_MAX_COMPS || (cap && !buf)) return NTTMUL_EINVAL;
  if (comps == 1) return nttmul_rns_kernel_name(r, kRnsMac, buf, cap);
  nttmul_rns_info info;
  if (const int st = nttmul_rns_get_info(r, &info)) return st;
  std::string name;
  if (describe_rns_macn(name_view(info.logn, info.limbs, info.word_bits), comps, &name) !=
      hipSuccess)
    return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

int nttmul_rnsmp_macn_kernel_name(const nttmul_rnsmp *r, uint32_t comps, char *buf, size_t cap) {
  if (!r || !comps || comps > NTTMUL_MACN_MAX_COMPS || (cap && !buf)) return NTTMUL_EINVAL;
  if (comps == 1) return nttmul_rnsmp_kernel_name(r, kRnsMac, buf, cap);
  nttmul_rnsmp_info info;
  if (const int st = nttmul_rnsmp_get_info(r, &info)) return st;
  std::string name;
  if (describe_rnsmp_macn(name_view(info.logn, info.limbs, info.word_bits), comps, &name) !=
      hipSuccess)
    return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

}  // extern "C"
