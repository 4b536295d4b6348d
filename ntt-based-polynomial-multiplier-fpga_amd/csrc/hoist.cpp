// hoist.cpp — host entry points of include/nttmul_hoist.h (lib/libnttmul_hoist.so only): the
// hoisted rotations on the existing contexts nttmul_rns and nttmul_rnsmp.  It has no handle and no
// state of its own.  The status of the arguments is hoist_plan.hpp's; everything after it -- the
// device selection, the range check, the staged host form, the multi-pass context's sub-batches
// and scratch hand-over, the error text -- is the context's own (rns.cpp rns_mac_comps with
// rots comps components of one shared b_hat; rnsmp.cpp rnsmp_units_op) with hoist.hip's launches.
#include <hip/hip_runtime.h>

#include <string>

#include "hoist.hpp"
#include "hoist_plan.hpp"
#include "limb_ctx.hpp"

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

uint32_t degree(const nttmul_rns *r) {
  nttmul_rns_info info;
  return r && nttmul_rns_get_info(r, &info) == NTTMUL_OK ? info.n : 0;
}
uint32_t degree(const nttmul_rnsmp *r) {
  nttmul_rnsmp_info info;
  return r && nttmul_rnsmp_get_info(r, &info) == NTTMUL_OK ? info.n : 0;
}

template <class Ctx>
int hoist_call(Ctx *r, void *c, const void *a_hat, const void *b_hat, const uint32_t *k,
               uint32_t rots, size_t batch, uint32_t terms, uint32_t comps, HoistArgs *H) {
  H->rots = rots;
  H->comps = comps;
  return hoist_args(r != nullptr, degree(r), c, a_hat, b_hat, k, rots, batch, terms, comps,
                    H->ks.k);
}

int rns_hoist(nttmul_rns *r, void *c, const void *a_hat, const void *b_hat, const uint32_t *k,
              uint32_t rots, size_t batch, uint32_t terms, uint32_t comps, int host, int dev,
              void *stream) {
  HoistArgs H;
  if (const int st = hoist_call(r, c, a_hat, b_hat, k, rots, batch, terms, comps, &H)) return st;
  return rns_mac_comps(r, launch_rns_hoist, c, a_hat, b_hat, batch, terms, rots * comps, 1, host,
                       dev, stream, &H);
}

int rnsmp_hoist(nttmul_rnsmp *r, void *c, const void *a_hat, const void *b_hat, const uint32_t *k,
                uint32_t rots, size_t batch, uint32_t terms, uint32_t comps, int host, int dev,
                void *stream) {
  HoistArgs H;
  if (const int st = hoist_call(r, c, a_hat, b_hat, k, rots, batch, terms, comps, &H)) return st;
  return rnsmp_units_op(r, launch_rnsmp_hoist, &H, c, a_hat, b_hat, batch, terms, rots, comps,
                        host, dev, stream);
}

}  // namespace

extern "C" {

int nttmul_rns_hoist_ntt_device(nttmul_rns *r, void *c, const void *a_hat, const void *b_hat,
                                const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                                uint32_t comps, int dev, void *stream) {
  return rns_hoist(r, c, a_hat, b_hat, k, rots, batch, terms, comps, 0, dev, stream);
}

int nttmul_rnsmp_hoist_ntt_device(nttmul_rnsmp *r, void *c, const void *a_hat, const void *b_hat,
                                  const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                                  uint32_t comps, int dev, void *stream) {
  return rnsmp_hoist(r, c, a_hat, b_hat, k, rots, batch, terms, comps, 0, dev, stream);
}

int nttmul_rns_hoist_ntt(nttmul_rns *r, void *c, const void *a_hat, const void *b_hat,
                         const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                         uint32_t comps) {
  return rns_hoist(r, c, a_hat, b_hat, k, rots, batch, terms, comps, 1, 0, nullptr);
}

int nttmul_rnsmp_hoist_ntt(nttmul_rnsmp *r, void *c, const void *a_hat, const void *b_hat,
                           const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                           uint32_t comps) {
  return rnsmp_hoist(r, c, a_hat, b_hat, k, rots, batch, terms, comps, 1, 0, nullptr);
}

int nttmul_rns_hoist_kernel_name(const nttmul_rns *r, uint32_t comps, char *buf, size_t cap) {
  if (!r || !comps || comps > NTTMUL_MACN_MAX_COMPS || (cap && !buf)) return NTTMUL_EINVAL;
  nttmul_rns_info info;
  if (const int st = nttmul_rns_get_info(r, &info)) return st;
  std::string name;
  if (describe_rns_hoist(name_view(info.logn, info.limbs, info.word_bits), comps, &name) !=
      hipSuccess)
    return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

int nttmul_rnsmp_hoist_kernel_name(const nttmul_rnsmp *r, uint32_t comps, char *buf, size_t cap) {
  if (!r || !comps || comps > NTTMUL_MACN_MAX_COMPS || (cap && !buf)) return NTTMUL_EINVAL;
  nttmul_rnsmp_info info;
  if (const int st = nttmul_rnsmp_get_info(r, &info)) return st;
  std::string name;
  if (describe_rnsmp_hoist(name_view(info.logn, info.limbs, info.word_bits), comps, &name) !=
      hipSuccess)
    return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

}  // extern "C"
