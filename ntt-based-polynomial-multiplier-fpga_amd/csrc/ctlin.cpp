// ctlin.cpp — host runtime behind include/nttmul_ctlin.h (lib/libnttmul_ctlin.so only): a context
// of one basis for one degree 256 <= n <= 65536 and the one launch each of combine and tensor
// (ctlin.hip).  The create-time checks, the argument checks, the plain constants and the grid
// arithmetic are ctlin_plan.hpp's (basis.cpp's checks between them), the context runtime
// limb_ctx.cpp's, the limb table's device form bconv.hpp's build_tables.  This file keeps its
// handle and what only it has: the per-limb table of R^2 mod q_l.  No twiddles, no scratch, no CPU
// fallback.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "ctlin.hpp"
#include "limb_ctx.hpp"
#include "nttmul_ctlin.h"

using namespace nttmul;

namespace {

struct ClDev {
  LimbDev base;                         // q: q_0 .. q_{L-1}
  void *to = nullptr, *limb = nullptr;  // ClTables
};

}  // namespace

struct nttmul_ctlin {
  ClPlan plan;
  int ndev = 0;
  ClDev dev[kMaxDev];
  char err[kErrBytes] = {0};
};

namespace {

const char *const kRangeMsg = "operand word >= its limb's modulus";

ClTables view(const nttmul_ctlin *h, const ClDev &d) {
  ClTables T;
  T.logn = h->plan.logn;
  T.L = h->plan.L;
  T.word_bits = h->plan.word_bits;
  T.to = d.to;
  T.limb = d.limb;
  return T;
}

template <class W>
std::vector<uint8_t> limb_table(const ClPlan &P) {
  std::vector<uint8_t> host(sizeof(ClLimb<W>) * P.L, 0);
  ClLimb<W> *E = (ClLimb<W> *)host.data();
  for (size_t l = 0; l < P.L; l++) E[l].r2 = (W)P.r2[l];
  return host;
}

int setup_device(nttmul_ctlin *h, ClDev &d) {
  const ClPlan &P = h->plan;
  LIMB_TRY(h->err, hipSetDevice(d.base.id));
  LIMB_TRY(h->err, hipStreamCreateWithFlags(&d.base.stream, hipStreamNonBlocking));
  LIMB_TRY(h->err, hipMalloc((void **)&d.base.flag, sizeof(int)));
  // the `to` entries over the basis with R mod q as their factor; no `from` limbs and no weights
  std::vector<uint8_t> from, to, w;
  build_tables(P.word_bits, {}, {}, P.m, P.r1, {}, &from, &to, &w);
  const std::vector<uint8_t> limb =
      P.word_bits == 32 ? limb_table<uint32_t>(P) : limb_table<uint64_t>(P);
  if (const int st = upload(h->err, &d.to, to.data(), to.size())) return st;
  if (const int st = upload(h->err, &d.limb, limb.data(), limb.size())) return st;
  return upload(h->err, (void **)&d.base.q, P.m.data(), sizeof(uint64_t) * P.m.size());
}

// the kernel's form of checked terms
ClTerms pack(const nttmul_ctlin_term *terms, uint32_t nterms) {
  ClTerms T = {};
  T.nterms = nterms;
  for (uint32_t i = 0; i < nterms; i++) {
    T.x[i] = terms[i].x;
    T.w[i] = terms[i].w;
    T.kind[i] = terms[i].kind;
    if (terms[i].kind == NTTMUL_CTLIN_PLAIN && terms[i].x) T.plain = 1;
  }
  return T;
}

// on d (the current device), stream s: the range check of every x and w, then the one launch
int run_combine(nttmul_ctlin *h, ClDev &d, void *out, const ClTerms &T, size_t batch,
                uint32_t comps, hipStream_t s) {
  if (!batch) return NTTMUL_OK;
  const ClPlan &P = h->plan;
  if (P.flags & NTTMUL_FLAG_VALIDATE) {
    size_t words[3];
    ctlin_combine_words(P.L, P.n, batch, comps, words);
    for (uint32_t i = 0; i < T.nterms; i++) {
      // a SCALAR's [L] words: one word per limb, q[i mod L]
      const bool scalar = T.kind[i] == NTTMUL_CTLIN_SCALAR;
      if (T.x[i])
        if (const int st = check_range(h->err, d.base.flag, d.base.q, P.L, P.logn, P.word_bits,
                                       T.x[i], words[0], nullptr, 0, kRangeMsg, s))
          return st;
      if (T.w[i])
        if (const int st = check_range(h->err, d.base.flag, d.base.q, P.L, scalar ? 0 : P.logn,
                                       P.word_bits, T.w[i], scalar ? words[1] : words[2], nullptr,
                                       0, kRangeMsg, s))
          return st;
    }
  }
  const hipError_t e = launch_ctlin_combine(view(h, d), out, T, batch, comps, s);
  return e == hipSuccess ? NTTMUL_OK : fail(h->err, e, "combine launch");
}

int run_tensor(nttmul_ctlin *h, ClDev &d, void *dh, const void *x, const void *y, size_t batch,
               uint32_t pairs, hipStream_t s) {
  if (!batch) return NTTMUL_OK;
  const ClPlan &P = h->plan;
  if (P.flags & NTTMUL_FLAG_VALIDATE) {
    size_t words[2];
    ctlin_tensor_words(P.L, P.n, batch, pairs, words);
    // (the square is checked once)
    if (const int st = check_range(h->err, d.base.flag, d.base.q, P.L, P.logn, P.word_bits, x,
                                   words[1], y, y == x ? 0 : words[1], kRangeMsg, s))
      return st;
  }
  const hipError_t e = launch_ctlin_tensor(view(h, d), dh, x, y, batch, pairs, s);
  return e == hipSuccess ? NTTMUL_OK : fail(h->err, e, "tensor launch");
}

// the host form's input buffer of a (pointer, size): an earlier term's, or a new one (buffer 0
// is out)
int staged_index(Staged *ops, int *count, const void *src, size_t bytes) {
  for (int i = 1; i < *count; i++)
    if (ops[i].src == src && ops[i].bytes == bytes) return i;
  ops[*count] = Staged{src, nullptr, bytes};
  return (*count)++;
}

}  // namespace

extern "C" {

int nttmul_ctlin_create(nttmul_ctlin **out, const nttmul_params *params, size_t size,
                        const uint64_t *q, uint32_t limbs) {
  if (!out) return NTTMUL_EINVAL;
  *out = nullptr;
  nttmul_ctlin *h = new (std::nothrow) nttmul_ctlin();
  if (!h) return NTTMUL_ENOMEM;
  if (const int st = ctlin_validate(params, size, q, limbs, &h->plan)) {
    delete h;
    return st;
  }
  ctlin_constants(&h->plan);
  DevRange R;
  if (const int st = select_devices(h->plan.prm, &R)) {
    delete h;
    return st;
  }
  DeviceGuard guard;
  for (int i = 0; i < R.ndev; i++) {
    ClDev &d = h->dev[i];
    d.base.id = R.id(i);
    h->ndev = i + 1;
    if (const int st = setup_device(h, d)) {
      const int ret = create_failed("nttmul_ctlin", h->err, st);
      nttmul_ctlin_destroy(h);
      return ret;
    }
  }
  *out = h;
  return NTTMUL_OK;
}

void nttmul_ctlin_destroy(nttmul_ctlin *h) {
  if (!h) return;
  destroy_devices(h->dev, h->ndev,
                  [](ClDev &d) { free_each({d.to, d.limb, d.base.q, d.base.flag}); });
  delete h;
}

const char *nttmul_ctlin_last_error(const nttmul_ctlin *h) { return h ? h->err : ""; }

int nttmul_ctlin_get_info(const nttmul_ctlin *h, nttmul_ctlin_info *info) {
  if (!h || !info) return NTTMUL_EINVAL;
  info->n = h->plan.n;
  info->logn = h->plan.logn;
  info->limbs = h->plan.L;
  info->word_bits = (uint32_t)h->plan.word_bits;
  info->ndev = h->ndev;
  return NTTMUL_OK;
}

int nttmul_ctlin_combine_device(nttmul_ctlin *h, void *out, const nttmul_ctlin_term *terms,
                                uint32_t nterms, size_t batch, uint32_t comps, int dev,
                                void *stream) {
  if (const int st = ctlin_combine_status(h != nullptr, out, terms, nterms, batch, comps))
    return st;
  const ClTerms T = pack(terms, nterms);
  return on_device(h->err, h->dev, h->ndev, dev, [&](ClDev &d) {
    return run_combine(h, d, out, T, batch, comps, (hipStream_t)stream);
  });
}

int nttmul_ctlin_combine(nttmul_ctlin *h, void *out, const nttmul_ctlin_term *terms,
                         uint32_t nterms, size_t batch, uint32_t comps) {
  if (const int st = ctlin_combine_status(h != nullptr, out, terms, nterms, batch, comps))
    return st;
  if (!batch) return NTTMUL_OK;
  ClDev &d = h->dev[0];
  size_t words[3];
  ctlin_combine_words(h->plan.L, h->plan.n, batch, comps, words);
  const size_t wb = (size_t)h->plan.word_bits / 8;
  // buffer 0 is out (copied in too when it is one of the x); one buffer per distinct x and w
  constexpr int kOps = 1 + 2 * NTTMUL_CTLIN_MAX_TERMS;
  Staged ops[kOps];
  int count = 1;
  ops[0] = Staged{nullptr, out, words[0] * wb};
  ClTerms T = pack(terms, nterms);
  int xi[NTTMUL_CTLIN_MAX_TERMS], wi[NTTMUL_CTLIN_MAX_TERMS];
  for (uint32_t i = 0; i < nterms; i++) {
    xi[i] = wi[i] = -1;
    if (terms[i].x == out) {
      ops[0].src = out;
      xi[i] = 0;
    } else if (terms[i].x) {
      xi[i] = staged_index(ops, &count, terms[i].x, words[0] * wb);
    }
    if (terms[i].w)
      wi[i] = staged_index(ops, &count, terms[i].w,
                           words[terms[i].kind == NTTMUL_CTLIN_SCALAR ? 1 : 2] * wb);
  }
  DeviceGuard guard;
  LIMB_TRY(h->err, hipSetDevice(d.base.id));
  void *buf[kOps] = {nullptr};
  int st = staged_begin(h->err, d.base, "ctlin", ops, count, buf);
  if (!st) {
    for (uint32_t i = 0; i < nterms; i++) {
      T.x[i] = xi[i] < 0 ? nullptr : buf[xi[i]];
      T.w[i] = wi[i] < 0 ? nullptr : buf[wi[i]];
    }
    st = run_combine(h, d, buf[0], T, batch, comps, d.base.stream);
  }
  return staged_end(h->err, d.base, "ctlin", ops, count, buf, st);
}

int nttmul_ctlin_tensor_device(nttmul_ctlin *h, void *d_hat, const void *x_hat, const void *y_hat,
                               size_t batch, uint32_t pairs, int dev, void *stream) {
  if (const int st = ctlin_tensor_status(h != nullptr, d_hat, x_hat, y_hat, batch, pairs))
    return st;
  return on_device(h->err, h->dev, h->ndev, dev, [&](ClDev &d) {
    return run_tensor(h, d, d_hat, x_hat, y_hat, batch, pairs, (hipStream_t)stream);
  });
}

int nttmul_ctlin_tensor(nttmul_ctlin *h, void *d_hat, const void *x_hat, const void *y_hat,
                        size_t batch, uint32_t pairs) {
  if (const int st = ctlin_tensor_status(h != nullptr, d_hat, x_hat, y_hat, batch, pairs))
    return st;
  if (!batch) return NTTMUL_OK;
  ClDev &d = h->dev[0];
  size_t words[2];
  ctlin_tensor_words(h->plan.L, h->plan.n, batch, pairs, words);
  const size_t wb = (size_t)h->plan.word_bits / 8;
  // (the square: one buffer, and the same pointer twice reaches the launch)
  const bool square = y_hat == x_hat;
  const Staged ops[3] = {{nullptr, d_hat, words[0] * wb},
                         {x_hat, nullptr, words[1] * wb},
                         {y_hat, nullptr, square ? 0 : words[1] * wb}};
  DeviceGuard guard;
  LIMB_TRY(h->err, hipSetDevice(d.base.id));
  void *buf[3] = {nullptr, nullptr, nullptr};
  int st = staged_begin(h->err, d.base, "ctlin", ops, 3, buf);
  if (!st) st = run_tensor(h, d, buf[0], buf[1], square ? buf[1] : buf[2], batch, pairs,
                           d.base.stream);
  return staged_end(h->err, d.base, "ctlin", ops, 3, buf, st);
}

int nttmul_ctlin_kernel_name(const nttmul_ctlin *h, int op, uint32_t comps, char *buf,
                             size_t cap) {
  if (!h || (cap && !buf) || (op != kClCombine && op != kClTensor)) return NTTMUL_EINVAL;
  if (op == kClCombine && (!comps || comps > NTTMUL_CTLIN_MAX_COMPS)) return NTTMUL_EINVAL;
  std::string name;
  if (describe_ctlin(view(h, h->dev[0]), op, comps, &name) != hipSuccess)
    return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

}  // extern "C"
