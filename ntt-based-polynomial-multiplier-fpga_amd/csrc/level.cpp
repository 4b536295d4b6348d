// level.cpp — host entry points of include/nttmul_level.h (lib/libnttmul_level.so only): mac, apply
// and relin with their key operands read through a level view, on the existing contexts
// nttmul_ksntt, nttmul_lintrans and nttmul_ctmul.  It has no handle and no state of its own.  The
// status of the arguments is the dense call's, then level_plan.hpp's; everything after it -- the
// device selection, the range checks of the dense operands, the staged host form, the error text
// -- is the context's own path (ksntt.cpp ksntt_mac_viewed, lintrans.cpp lintrans_apply_viewed,
// ctmul.cpp ctmul_relin_viewed) with level.hip's launches and strided range check in place of its
// own.
#include <hip/hip_runtime.h>

#include <string>

#include "level.hpp"
#include "limb_ctx.hpp"

using namespace nttmul;

namespace {

// limb_ctx.cpp's check_range over the words a view selects (ksntt.hpp LevelCheck)
int check_view(char *err, int *flag, const uint64_t *q, int word_bits, const void *op,
               const LevelAddr &A, size_t outer, uint32_t terms, bool has_terms, const char *msg,
               hipStream_t s) {
  LIMB_TRY(err, hipMemsetAsync(flag, 0, sizeof(int), s));
  LIMB_TRY(err, launch_level_check(op, q, word_bits, A, outer, terms, has_terms, flag, s));
  int bad = 0;
  LIMB_TRY(err, hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, s));
  LIMB_TRY(err, hipStreamSynchronize(s));
  if (bad) {
    set_err(err, msg);
    return NTTMUL_ERANGE;
  }
  return NTTMUL_OK;
}

int mac_view(nttmul_ksntt *h, void *c_hat, const void *a_hat, const void *b_hat, const uint32_t *k,
             uint32_t rots, size_t batch, uint32_t terms, uint32_t comps,
             const nttmul_level_view *view, int host, int dev, void *stream) {
  nttmul_ksntt_info info = {};
  if (h) (void)nttmul_ksntt_get_info(h, &info);
  uint32_t kv[NTTMUL_HOIST_MAX_ROTS];
  if (const int st = ksntt_mac_status(h != nullptr, info.n, c_hat, a_hat, b_hat, k, rots, batch,
                                      terms, comps, kv))
    return st;
  if (const int st = level_view_status(view, info.q_limbs, info.p_limbs, terms)) return st;
  const LevelAddr A = level_addr(info.q_limbs, info.p_limbs, info.logn, *view);
  const KsnttViewed V = {&A, level_key_words(A, (size_t)rots * comps), check_view,
                         launch_level_mac};
  return ksntt_mac_viewed(h, V, c_hat, a_hat, b_hat, k, rots, batch, terms, comps, host, dev,
                          stream);
}

int apply_view(nttmul_lintrans *h, void *c_hat, const void *a_hat, const void *b_hat,
               const void *w_hat, const void *c0_hat, const uint32_t *k, uint32_t rots,
               size_t batch, uint32_t terms, uint32_t comps, const nttmul_level_view *view,
               int host, int dev, void *stream) {
  nttmul_lintrans_info info = {};
  if (h) (void)nttmul_lintrans_get_info(h, &info);
  uint32_t kv[NTTMUL_HOIST_MAX_ROTS];
  if (const int st = lintrans_apply_status(h != nullptr, info.n, c_hat, a_hat, b_hat, k, rots,
                                           batch, terms, comps, kv))
    return st;
  if (const int st = level_view_status(view, info.q_limbs, info.p_limbs, terms)) return st;
  const LevelAddr A = level_addr(info.q_limbs, info.p_limbs, info.logn, *view);
  const LtViewed V = {&A, level_key_words(A, (size_t)rots * comps), level_diag_words(A, rots),
                      check_view, launch_level_lintrans};
  return lintrans_apply_viewed(h, V, c_hat, a_hat, b_hat, w_hat, c0_hat, k, rots, batch, terms,
                               comps, host, dev, stream);
}

int relin_view(nttmul_ctmul *h, void *c_hat, const void *up_hat, const void *key_hat,
               const void *x_hat, const void *y_hat, size_t batch, uint32_t pairs, uint32_t terms,
               const nttmul_level_view *view, int host, int dev, void *stream) {
  if (const int st = ctmul_relin_status(h != nullptr, c_hat, up_hat, key_hat, x_hat, y_hat, batch,
                                        pairs, terms))
    return st;
  nttmul_ctmul_info info = {};
  (void)nttmul_ctmul_get_info(h, &info);
  if (const int st = level_view_status(view, info.q_limbs, info.p_limbs, terms)) return st;
  const LevelAddr A = level_addr(info.q_limbs, info.p_limbs, info.logn, *view);
  const CtViewed V = {&A, level_key_words(A, 2), check_view, launch_level_relin};
  return ctmul_relin_viewed(h, V, c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs, terms, host,
                            dev, stream);
}

}  // namespace

extern "C" {

int nttmul_ksntt_mac_view_device(nttmul_ksntt *h, void *c_hat, const void *a_hat,
                                 const void *b_hat, const uint32_t *k, uint32_t rots, size_t batch,
                                 uint32_t terms, uint32_t comps, const nttmul_level_view *view,
                                 int dev, void *stream) {
  return mac_view(h, c_hat, a_hat, b_hat, k, rots, batch, terms, comps, view, 0, dev, stream);
}

int nttmul_ksntt_mac_view(nttmul_ksntt *h, void *c_hat, const void *a_hat, const void *b_hat,
                          const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                          uint32_t comps, const nttmul_level_view *view) {
  return mac_view(h, c_hat, a_hat, b_hat, k, rots, batch, terms, comps, view, 1, 0, nullptr);
}

int nttmul_lintrans_apply_view_device(nttmul_lintrans *h, void *c_hat, const void *a_hat,
                                      const void *b_hat, const void *w_hat, const void *c0_hat,
                                      const uint32_t *k, uint32_t rots, size_t batch,
                                      uint32_t terms, uint32_t comps,
                                      const nttmul_level_view *view, int dev, void *stream) {
  return apply_view(h, c_hat, a_hat, b_hat, w_hat, c0_hat, k, rots, batch, terms, comps, view, 0,
                    dev, stream);
}

int nttmul_lintrans_apply_view(nttmul_lintrans *h, void *c_hat, const void *a_hat,
                               const void *b_hat, const void *w_hat, const void *c0_hat,
                               const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                               uint32_t comps, const nttmul_level_view *view) {
  return apply_view(h, c_hat, a_hat, b_hat, w_hat, c0_hat, k, rots, batch, terms, comps, view, 1,
                    0, nullptr);
}

int nttmul_ctmul_relin_view_device(nttmul_ctmul *h, void *c_hat, const void *up_hat,
                                   const void *key_hat, const void *x_hat, const void *y_hat,
                                   size_t batch, uint32_t pairs, uint32_t terms,
                                   const nttmul_level_view *view, int dev, void *stream) {
  return relin_view(h, c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs, terms, view, 0, dev,
                    stream);
}

int nttmul_ctmul_relin_view(nttmul_ctmul *h, void *c_hat, const void *up_hat,
                            const void *key_hat, const void *x_hat, const void *y_hat,
                            size_t batch, uint32_t pairs, uint32_t terms,
                            const nttmul_level_view *view) {
  return relin_view(h, c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs, terms, view, 1, 0,
                    nullptr);
}

int nttmul_level_kernel_name(int op, uint32_t logn, uint32_t word_bits, uint32_t comps,
                             int weighted, char *buf, size_t cap) {
  if ((cap && !buf) || op < NTTMUL_LEVEL_MAC || op > NTTMUL_LEVEL_RELIN || logn < 8 ||
      logn > 16 || (word_bits != 32 && word_bits != 64))
    return NTTMUL_EINVAL;
  if (op != NTTMUL_LEVEL_RELIN && (!comps || comps > NTTMUL_MACN_MAX_COMPS)) return NTTMUL_EINVAL;
  std::string name;
  if (describe_level(op, logn, (int)word_bits, op == NTTMUL_LEVEL_RELIN ? 1 : comps,
                     weighted != 0, &name) != hipSuccess)
    return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

}  // extern "C"
