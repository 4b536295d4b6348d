// ctmul.cpp — host runtime behind include/nttmul_ctmul.h (lib/libnttmul_ctmul.so only): a context
// of the bases Q and P for one degree 256 <= n <= 65536 and the one launch each of high and relin
// (ctmul.hip).  The create-time checks, the plain constants and the grid arithmetic are
// ctmul_plan.hpp's (basis.cpp's checks between them), the context runtime limb_ctx.cpp's, the
// conversion table's device form bconv.hpp's build_tables.  This file keeps its handle and what
// only it has: the per-limb table of P R mod q_l.  No twiddles, no scratch, no CPU fallback.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "ctmul.hpp"
#include "limb_ctx.hpp"
#include "nttmul_ctmul.h"

using namespace nttmul;

namespace {

struct CtDev {
  LimbDev base;                         // q: q_0 .. q_{L-1}, p_0 .. p_{K-1}
  void *to = nullptr, *limb = nullptr;  // CtTables
};

}  // namespace

struct nttmul_ctmul {
  CtPlan plan;
  int ndev = 0;
  CtDev dev[kMaxDev];
  char err[kErrBytes] = {0};
};

namespace {

const char *const kRangeMsg = "operand word >= its limb's modulus";

CtTables view(const nttmul_ctmul *h, const CtDev &d) {
  CtTables T;
  T.logn = h->plan.logn;
  T.L = h->plan.L;
  T.K = h->plan.K;
  T.word_bits = h->plan.word_bits;
  T.to = d.to;
  T.limb = d.limb;
  return T;
}

template <class W>
std::vector<uint8_t> limb_table(const CtPlan &P) {
  std::vector<uint8_t> host(sizeof(CtLimb<W>) * P.L, 0);
  CtLimb<W> *E = (CtLimb<W> *)host.data();
  for (size_t l = 0; l < P.L; l++) E[l].pr = (W)P.pr[l];
  return host;
}

int setup_device(nttmul_ctmul *h, CtDev &d) {
  const CtPlan &P = h->plan;
  LIMB_TRY(h->err, hipSetDevice(d.base.id));
  LIMB_TRY(h->err, hipStreamCreateWithFlags(&d.base.stream, hipStreamNonBlocking));
  LIMB_TRY(h->err, hipMalloc((void **)&d.base.flag, sizeof(int)));
  // the table k_ksntt_mac reads: the `to` entries over Q u P with R mod m as their factor; no
  // `from` limbs and no weights
  std::vector<uint8_t> from, to, w;
  build_tables(P.word_bits, {}, {}, P.m, P.r1, {}, &from, &to, &w);
  const std::vector<uint8_t> limb =
      P.word_bits == 32 ? limb_table<uint32_t>(P) : limb_table<uint64_t>(P);
  if (const int st = upload(h->err, &d.to, to.data(), to.size())) return st;
  if (const int st = upload(h->err, &d.limb, limb.data(), limb.size())) return st;
  return upload(h->err, (void **)&d.base.q, P.m.data(), sizeof(uint64_t) * P.m.size());
}

// x_hat and y_hat over the limbs of Q; the square is checked once
int check_pairs(nttmul_ctmul *h, CtDev &d, const void *x, const void *y, size_t words,
                hipStream_t s) {
  const CtPlan &P = h->plan;
  return check_range(h->err, d.base.flag, d.base.q, P.L, P.logn, P.word_bits, x, words, y,
                     y == x ? 0 : words, kRangeMsg, s);
}

// on d (the current device), stream s: the range check of every operand, then the one launch
int run_high(nttmul_ctmul *h, CtDev &d, void *d2, const void *x, const void *y, size_t batch,
             uint32_t pairs, hipStream_t s) {
  if (!batch) return NTTMUL_OK;
  const CtPlan &P = h->plan;
  if (P.flags & NTTMUL_FLAG_VALIDATE) {
    size_t words[2];
    ctmul_high_words(P.L, P.n, batch, pairs, words);
    if (const int st = check_pairs(h, d, x, y, words[1], s)) return st;
  }
  const hipError_t e = launch_ctmul_high(view(h, d), d2, x, y, batch, pairs, s);
  return e == hipSuccess ? NTTMUL_OK : fail(h->err, e, "high launch");
}

// V: key_hat is viewed (ctmul.hpp CtViewed), its check and the launch are V's
int run_relin(nttmul_ctmul *h, CtDev &d, void *c, const void *up, const void *key, const void *x,
              const void *y, size_t batch, uint32_t pairs, uint32_t terms, hipStream_t s,
              const CtViewed *V = nullptr) {
  if (!batch) return NTTMUL_OK;
  const CtPlan &P = h->plan;
  if (P.flags & NTTMUL_FLAG_VALIDATE) {
    size_t words[4];
    ctmul_relin_words(P.L, P.K, P.n, batch, pairs, terms, words);
    if (const int st = check_range(h->err, d.base.flag, d.base.q, P.L + P.K, P.logn, P.word_bits,
                                   up, words[1], key, V ? 0 : words[2], kRangeMsg, s))
      return st;
    if (V)
      if (const int st = V->check(h->err, d.base.flag, d.base.q, P.word_bits, key, *V->addr, 2,
                                  terms, true, kRangeMsg, s))
        return st;
    if (const int st = check_pairs(h, d, x, y, words[3], s)) return st;
  }
  const hipError_t e =
      V ? V->launch(view(h, d), c, up, key, x, y, batch, pairs, terms, *V->addr, s)
        : launch_ctmul_relin(view(h, d), c, up, key, x, y, batch, pairs, terms, s);
  return e == hipSuccess ? NTTMUL_OK : fail(h->err, e, "relin launch");
}

// nttmul_ctmul_relin_device; V: key_hat viewed
int relin_device(nttmul_ctmul *h, void *c_hat, const void *up_hat, const void *key_hat,
                 const void *x_hat, const void *y_hat, size_t batch, uint32_t pairs,
                 uint32_t terms, int dev, void *stream, const CtViewed *V) {
  if (const int st = ctmul_relin_status(h != nullptr, c_hat, up_hat, key_hat, x_hat, y_hat, batch,
                                        pairs, terms))
    return st;
  return on_device(h->err, h->dev, h->ndev, dev, [&](CtDev &d) {
    return run_relin(h, d, c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs, terms,
                     (hipStream_t)stream, V);
  });
}

// nttmul_ctmul_relin; V: key_hat viewed, staged whole
int relin_host(nttmul_ctmul *h, void *c_hat, const void *up_hat, const void *key_hat,
               const void *x_hat, const void *y_hat, size_t batch, uint32_t pairs, uint32_t terms,
               const CtViewed *V) {
  if (const int st = ctmul_relin_status(h != nullptr, c_hat, up_hat, key_hat, x_hat, y_hat, batch,
                                        pairs, terms))
    return st;
  if (!batch) return NTTMUL_OK;
  CtDev &d = h->dev[0];
  size_t words[4];
  ctmul_relin_words(h->plan.L, h->plan.K, h->plan.n, batch, pairs, terms, words);
  if (V) words[2] = V->key_words;
  const size_t wb = (size_t)h->plan.word_bits / 8;
  const bool square = y_hat == x_hat;
  const Staged ops[5] = {{nullptr, c_hat, words[0] * wb},
                         {up_hat, nullptr, words[1] * wb},
                         {key_hat, nullptr, words[2] * wb},
                         {x_hat, nullptr, words[3] * wb},
                         {y_hat, nullptr, square ? 0 : words[3] * wb}};
  DeviceGuard guard;
  LIMB_TRY(h->err, hipSetDevice(d.base.id));
  void *buf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int st = staged_begin(h->err, d.base, "ctmul", ops, 5, buf);
  if (!st) st = run_relin(h, d, buf[0], buf[1], buf[2], buf[3], square ? buf[3] : buf[4], batch,
                          pairs, terms, d.base.stream, V);
  return staged_end(h->err, d.base, "ctmul", ops, 5, buf, st);
}

}  // namespace

namespace nttmul {

int ctmul_relin_viewed(nttmul_ctmul *h, const CtViewed &V, void *c_hat, const void *up_hat,
                       const void *key_hat, const void *x_hat, const void *y_hat, size_t batch,
                       uint32_t pairs, uint32_t terms, int host, int dev, void *stream) {
  if (host) return relin_host(h, c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs, terms, &V);
  return relin_device(h, c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs, terms, dev, stream,
                      &V);
}

}  // namespace nttmul

extern "C" {

int nttmul_ctmul_create(nttmul_ctmul **out, const nttmul_params *params, size_t size,
                        const uint64_t *q, uint32_t q_limbs, const uint64_t *p,
                        uint32_t p_limbs) {
  if (!out) return NTTMUL_EINVAL;
  *out = nullptr;
  nttmul_ctmul *h = new (std::nothrow) nttmul_ctmul();
  if (!h) return NTTMUL_ENOMEM;
  if (const int st = ctmul_validate(params, size, q, q_limbs, p, p_limbs, &h->plan)) {
    delete h;
    return st;
  }
  ctmul_constants(&h->plan);
  DevRange R;
  if (const int st = select_devices(h->plan.prm, &R)) {
    delete h;
    return st;
  }
  DeviceGuard guard;
  for (int i = 0; i < R.ndev; i++) {
    CtDev &d = h->dev[i];
    d.base.id = R.id(i);
    h->ndev = i + 1;
    if (const int st = setup_device(h, d)) {
      const int ret = create_failed("nttmul_ctmul", h->err, st);
      nttmul_ctmul_destroy(h);
      return ret;
    }
  }
  *out = h;
  return NTTMUL_OK;
}

void nttmul_ctmul_destroy(nttmul_ctmul *h) {
  if (!h) return;
  destroy_devices(h->dev, h->ndev,
                  [](CtDev &d) { free_each({d.to, d.limb, d.base.q, d.base.flag}); });
  delete h;
}

const char *nttmul_ctmul_last_error(const nttmul_ctmul *h) { return h ? h->err : ""; }

int nttmul_ctmul_get_info(const nttmul_ctmul *h, nttmul_ctmul_info *info) {
  if (!h || !info) return NTTMUL_EINVAL;
  info->n = h->plan.n;
  info->logn = h->plan.logn;
  info->q_limbs = h->plan.L;
  info->p_limbs = h->plan.K;
  info->word_bits = (uint32_t)h->plan.word_bits;
  info->ndev = h->ndev;
  return NTTMUL_OK;
}

int nttmul_ctmul_high_device(nttmul_ctmul *h, void *d2_hat, const void *x_hat, const void *y_hat,
                             size_t batch, uint32_t pairs, int dev, void *stream) {
  if (const int st = ctmul_high_status(h != nullptr, d2_hat, x_hat, y_hat, batch, pairs))
    return st;
  return on_device(h->err, h->dev, h->ndev, dev, [&](CtDev &d) {
    return run_high(h, d, d2_hat, x_hat, y_hat, batch, pairs, (hipStream_t)stream);
  });
}

int nttmul_ctmul_high(nttmul_ctmul *h, void *d2_hat, const void *x_hat, const void *y_hat,
                      size_t batch, uint32_t pairs) {
  if (const int st = ctmul_high_status(h != nullptr, d2_hat, x_hat, y_hat, batch, pairs))
    return st;
  if (!batch) return NTTMUL_OK;
  CtDev &d = h->dev[0];
  size_t words[2];
  ctmul_high_words(h->plan.L, h->plan.n, batch, pairs, words);
  const size_t wb = (size_t)h->plan.word_bits / 8;
  // (the square: one buffer, and the same pointer twice reaches the launch)
  const bool square = y_hat == x_hat;
  const Staged ops[3] = {{nullptr, d2_hat, words[0] * wb},
                         {x_hat, nullptr, words[1] * wb},
                         {y_hat, nullptr, square ? 0 : words[1] * wb}};
  DeviceGuard guard;
  LIMB_TRY(h->err, hipSetDevice(d.base.id));
  void *buf[3] = {nullptr, nullptr, nullptr};
  int st = staged_begin(h->err, d.base, "ctmul", ops, 3, buf);
  if (!st) st = run_high(h, d, buf[0], buf[1], square ? buf[1] : buf[2], batch, pairs,
                         d.base.stream);
  return staged_end(h->err, d.base, "ctmul", ops, 3, buf, st);
}

int nttmul_ctmul_relin_device(nttmul_ctmul *h, void *c_hat, const void *up_hat,
                              const void *key_hat, const void *x_hat, const void *y_hat,
                              size_t batch, uint32_t pairs, uint32_t terms, int dev,
                              void *stream) {
  return relin_device(h, c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs, terms, dev, stream,
                      nullptr);
}

int nttmul_ctmul_relin(nttmul_ctmul *h, void *c_hat, const void *up_hat, const void *key_hat,
                       const void *x_hat, const void *y_hat, size_t batch, uint32_t pairs,
                       uint32_t terms) {
  return relin_host(h, c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs, terms, nullptr);
}

int nttmul_ctmul_kernel_name(const nttmul_ctmul *h, int op, char *buf, size_t cap) {
  if (!h || (cap && !buf) || (op != kCtHigh && op != kCtRelin)) return NTTMUL_EINVAL;
  std::string name;
  if (describe_ctmul(view(h, h->dev[0]), op, &name) != hipSuccess) return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

}  // extern "C"
