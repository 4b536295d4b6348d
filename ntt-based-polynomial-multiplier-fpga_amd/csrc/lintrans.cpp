// lintrans.cpp — host runtime behind include/nttmul_lintrans.h (lib/libnttmul_lintrans.so only): a
// context of the bases Q and P for one degree 256 <= n <= 65536 and the one launch of apply
// (lintrans.hip).  The create-time checks, the plain constants and the grid arithmetic are
// lintrans_plan.hpp's (basis.cpp's checks between them), the context runtime limb_ctx.cpp's, the
// conversion table's device form bconv.hpp's build_tables.  This file keeps its handle and what
// only it has: the per-limb table of R^2 mod m and P mod q_l.  No twiddles, no scratch, no CPU
// fallback.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "limb_ctx.hpp"
#include "lintrans.hpp"
#include "nttmul_lintrans.h"

using namespace nttmul;

namespace {

struct LtDev {
  LimbDev base;                         // q: q_0 .. q_{L-1}, p_0 .. p_{K-1}
  void *to = nullptr, *limb = nullptr;  // LtTables
};

}  // namespace

struct nttmul_lintrans {
  LtPlan plan;
  int ndev = 0;
  LtDev dev[kMaxDev];
  char err[kErrBytes] = {0};
};

namespace {

LtTables view(const nttmul_lintrans *h, const LtDev &d) {
  LtTables T;
  T.logn = h->plan.logn;
  T.L = h->plan.L;
  T.K = h->plan.K;
  T.word_bits = h->plan.word_bits;
  T.to = d.to;
  T.limb = d.limb;
  return T;
}

template <class W>
std::vector<uint8_t> limb_table(const LtPlan &P) {
  std::vector<uint8_t> host(sizeof(LtLimb<W>) * P.m.size(), 0);
  LtLimb<W> *E = (LtLimb<W> *)host.data();
  for (size_t l = 0; l < P.m.size(); l++) {
    mul_pair<W>(P.r2[l], P.m[l], &E[l].r2, &E[l].r2s);
    E[l].pq = l < P.L ? (W)P.pq[l] : 0;
  }
  return host;
}

int setup_device(nttmul_lintrans *h, LtDev &d) {
  const LtPlan &P = h->plan;
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

// on d (the current device), stream s: the range check of every operand that is given over its
// limbs, then the one launch.  V: b_hat and w_hat are viewed (lintrans.hpp LtViewed), their checks
// and the launch are V's
int run(nttmul_lintrans *h, LtDev &d, void *c, const void *a, const void *b, const void *w,
        const void *c0, const HoistArgs &H, size_t batch, uint32_t terms, hipStream_t s,
        const LtViewed *V = nullptr) {
  if (!batch) return NTTMUL_OK;
  const LtPlan &P = h->plan;
  if (P.flags & NTTMUL_FLAG_VALIDATE) {
    size_t words[5];
    lintrans_words(P.L, P.K, P.n, batch, terms, H.rots, H.comps, words);
    const char *msg = "operand word >= its limb's modulus";
    if (const int st = check_range(h->err, d.base.flag, d.base.q, P.L + P.K, P.logn, P.word_bits,
                                   a, words[1], b, V ? 0 : words[2], msg, s))
      return st;
    if (V)
      if (const int st = V->check(h->err, d.base.flag, d.base.q, P.word_bits, b, *V->addr,
                                  (size_t)H.rots * H.comps, terms, true, msg, s))
        return st;
    if (w)
      if (const int st = V ? V->check(h->err, d.base.flag, d.base.q, P.word_bits, w, *V->addr,
                                      H.rots, 1, false, msg, s)
                           : check_range(h->err, d.base.flag, d.base.q, P.L + P.K, P.logn,
                                         P.word_bits, w, words[3], nullptr, 0, msg, s))
        return st;
    if (c0)
      if (const int st = check_range(h->err, d.base.flag, d.base.q, P.L, P.logn, P.word_bits, c0,
                                     words[4], nullptr, 0, msg, s))
        return st;
  }
  const hipError_t e = V ? V->launch(view(h, d), c, a, b, w, c0, H, batch, terms, *V->addr, s)
                         : launch_lintrans(view(h, d), c, a, b, w, c0, H, batch, terms, s);
  return e == hipSuccess ? NTTMUL_OK : fail(h->err, e, "apply launch");
}

int apply_call(nttmul_lintrans *h, void *c, const void *a, const void *b, const uint32_t *k,
               uint32_t rots, size_t batch, uint32_t terms, uint32_t comps, HoistArgs *H) {
  H->rots = rots;
  H->comps = comps;
  return lintrans_apply_status(h != nullptr, h ? h->plan.n : 0, c, a, b, k, rots, batch, terms,
                               comps, H->ks.k);
}

// nttmul_lintrans_apply_device; V: b_hat and w_hat viewed
int apply_device(nttmul_lintrans *h, void *c_hat, const void *a_hat, const void *b_hat,
                 const void *w_hat, const void *c0_hat, const uint32_t *k, uint32_t rots,
                 size_t batch, uint32_t terms, uint32_t comps, int dev, void *stream,
                 const LtViewed *V) {
  HoistArgs H;
  if (const int st = apply_call(h, c_hat, a_hat, b_hat, k, rots, batch, terms, comps, &H))
    return st;
  return on_device(h->err, h->dev, h->ndev, dev, [&](LtDev &d) {
    return run(h, d, c_hat, a_hat, b_hat, w_hat, c0_hat, H, batch, terms, (hipStream_t)stream, V);
  });
}

// nttmul_lintrans_apply; V: b_hat and w_hat viewed, staged whole
int apply_host(nttmul_lintrans *h, void *c_hat, const void *a_hat, const void *b_hat,
               const void *w_hat, const void *c0_hat, const uint32_t *k, uint32_t rots,
               size_t batch, uint32_t terms, uint32_t comps, const LtViewed *V) {
  HoistArgs H;
  if (const int st = apply_call(h, c_hat, a_hat, b_hat, k, rots, batch, terms, comps, &H))
    return st;
  if (!batch) return NTTMUL_OK;
  LtDev &d = h->dev[0];
  size_t words[5];
  lintrans_words(h->plan.L, h->plan.K, h->plan.n, batch, terms, rots, comps, words);
  if (V) {
    words[2] = V->b_words;
    words[3] = V->w_words;
  }
  const size_t wb = (size_t)h->plan.word_bits / 8;
  // (a NULL w_hat or c0_hat: no bytes, no buffer, and the NULL reaches the launch)
  const Staged ops[5] = {{nullptr, c_hat, words[0] * wb},
                         {a_hat, nullptr, words[1] * wb},
                         {b_hat, nullptr, words[2] * wb},
                         {w_hat, nullptr, w_hat ? words[3] * wb : 0},
                         {c0_hat, nullptr, c0_hat ? words[4] * wb : 0}};
  DeviceGuard guard;
  LIMB_TRY(h->err, hipSetDevice(d.base.id));
  void *buf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int st = staged_begin(h->err, d.base, "lintrans", ops, 5, buf);
  if (!st)
    st = run(h, d, buf[0], buf[1], buf[2], buf[3], buf[4], H, batch, terms, d.base.stream, V);
  return staged_end(h->err, d.base, "lintrans", ops, 5, buf, st);
}

}  // namespace

namespace nttmul {

int lintrans_apply_viewed(nttmul_lintrans *h, const LtViewed &V, void *c_hat, const void *a_hat,
                          const void *b_hat, const void *w_hat, const void *c0_hat,
                          const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                          uint32_t comps, int host, int dev, void *stream) {
  if (host)
    return apply_host(h, c_hat, a_hat, b_hat, w_hat, c0_hat, k, rots, batch, terms, comps, &V);
  return apply_device(h, c_hat, a_hat, b_hat, w_hat, c0_hat, k, rots, batch, terms, comps, dev,
                      stream, &V);
}

}  // namespace nttmul

extern "C" {

int nttmul_lintrans_create(nttmul_lintrans **out, const nttmul_params *params, size_t size,
                           const uint64_t *q, uint32_t q_limbs, const uint64_t *p,
                           uint32_t p_limbs) {
  if (!out) return NTTMUL_EINVAL;
  *out = nullptr;
  nttmul_lintrans *h = new (std::nothrow) nttmul_lintrans();
  if (!h) return NTTMUL_ENOMEM;
  if (const int st = lintrans_validate(params, size, q, q_limbs, p, p_limbs, &h->plan)) {
    delete h;
    return st;
  }
  lintrans_constants(&h->plan);
  DevRange R;
  if (const int st = select_devices(h->plan.prm, &R)) {
    delete h;
    return st;
  }
  DeviceGuard guard;
  for (int i = 0; i < R.ndev; i++) {
    LtDev &d = h->dev[i];
    d.base.id = R.id(i);
    h->ndev = i + 1;
    if (const int st = setup_device(h, d)) {
      const int ret = create_failed("nttmul_lintrans", h->err, st);
      nttmul_lintrans_destroy(h);
      return ret;
    }
  }
  *out = h;
  return NTTMUL_OK;
}

void nttmul_lintrans_destroy(nttmul_lintrans *h) {
  if (!h) return;
  destroy_devices(h->dev, h->ndev,
                  [](LtDev &d) { free_each({d.to, d.limb, d.base.q, d.base.flag}); });
  delete h;
}

const char *nttmul_lintrans_last_error(const nttmul_lintrans *h) { return h ? h->err : ""; }

int nttmul_lintrans_get_info(const nttmul_lintrans *h, nttmul_lintrans_info *info) {
  if (!h || !info) return NTTMUL_EINVAL;
  info->n = h->plan.n;
  info->logn = h->plan.logn;
  info->q_limbs = h->plan.L;
  info->p_limbs = h->plan.K;
  info->word_bits = (uint32_t)h->plan.word_bits;
  info->ndev = h->ndev;
  return NTTMUL_OK;
}

int nttmul_lintrans_apply_device(nttmul_lintrans *h, void *c_hat, const void *a_hat,
                                 const void *b_hat, const void *w_hat, const void *c0_hat,
                                 const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                                 uint32_t comps, int dev, void *stream) {
  return apply_device(h, c_hat, a_hat, b_hat, w_hat, c0_hat, k, rots, batch, terms, comps, dev,
                      stream, nullptr);
}

int nttmul_lintrans_apply(nttmul_lintrans *h, void *c_hat, const void *a_hat, const void *b_hat,
                          const void *w_hat, const void *c0_hat, const uint32_t *k, uint32_t rots,
                          size_t batch, uint32_t terms, uint32_t comps) {
  return apply_host(h, c_hat, a_hat, b_hat, w_hat, c0_hat, k, rots, batch, terms, comps, nullptr);
}

int nttmul_lintrans_kernel_name(const nttmul_lintrans *h, uint32_t comps, int weighted, char *buf,
                                size_t cap) {
  if (!h || (cap && !buf) || !comps || comps > NTTMUL_MACN_MAX_COMPS) return NTTMUL_EINVAL;
  std::string name;
  if (describe_lintrans(view(h, h->dev[0]), comps, weighted != 0, &name) != hipSuccess)
    return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

}  // extern "C"
