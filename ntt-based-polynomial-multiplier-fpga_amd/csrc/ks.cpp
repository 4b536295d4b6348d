// ks.cpp — host runtime behind include/nttmul_ks.h (lib/libnttmul_ks.so only): a context of the
// bases Q and P and a digit width for one degree 256 <= n <= 65536, and the one launch per call:
// k_ks_modup (ks.hip) for ModUp, and for ModDown the k_bconv<W,1> of bconv.hip through
// launch_bconv with tables built for from = P, to = Q.  The validation and the plain constants
// are in ks_plan.cpp (host only); the device tables are derived here from the same values, with
// bconv.hpp's build_tables.  A context keeps the tables, the moduli and the range check's flag per
// device: no scratch, no state between calls, no CPU fallback.
// The context runtime is limb_ctx.cpp's.  This file keeps its handle, its two sets of tables and
// its run.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "ks.hpp"
#include "ks_plan.hpp"
#include "limb_ctx.hpp"
#include "nttmul_ks.h"

using namespace nttmul;

namespace {

struct KsDev {
  LimbDev base;                  // q: q_0 .. q_{L-1}, p_0 .. p_{K-1}
  void *up_from = nullptr, *up_to = nullptr, *up_w = nullptr;  // ModUp: digits of Q -> Q u P
  void *dn_from = nullptr, *dn_to = nullptr, *dn_w = nullptr;  // ModDown: P -> Q
};

}  // namespace

struct nttmul_ks {
  KsPlan plan;
  int ndev = 0;
  KsDev dev[kMaxDev];
  char err[kErrBytes] = {0};
};

namespace {

KsTables up_tables(const nttmul_ks *h, const KsDev &d) {
  KsTables T;
  T.logn = h->plan.logn;
  T.q_limbs = h->plan.L;
  T.p_limbs = h->plan.K;
  T.digit_limbs = h->plan.alpha;
  T.digits = h->plan.dnum;
  T.word_bits = h->plan.word_bits;
  T.from = d.up_from;
  T.to = d.up_to;
  T.w = d.up_w;
  return T;
}

// ModDown is nttmul_bconv_moddown with from = P and to = Q
BconvTables down_tables(const nttmul_ks *h, const KsDev &d) {
  BconvTables T;
  T.logn = h->plan.logn;
  T.from_limbs = h->plan.K;
  T.to_limbs = h->plan.L;
  T.word_bits = h->plan.word_bits;
  T.from = d.dn_from;
  T.to = d.dn_to;
  T.w = d.dn_w;
  T.q = d.base.q;
  return T;
}

int setup_device(nttmul_ks *h, KsDev &d) {
  const KsPlan &P = h->plan;
  LIMB_TRY(h->err, hipSetDevice(d.base.id));
  LIMB_TRY(h->err, hipStreamCreateWithFlags(&d.base.stream, hipStreamNonBlocking));
  LIMB_TRY(h->err, hipMalloc((void **)&d.base.flag, sizeof(int)));
  std::vector<uint64_t> ext(P.q);
  ext.insert(ext.end(), P.p.begin(), P.p.end());
  // ModUp's `to` entries carry no epilogue factor: the pair of 1
  const std::vector<uint64_t> one(ext.size(), 1);
  std::vector<uint8_t> from, to, w;
  build_tables(P.word_bits, P.q, P.inv, ext, one, P.w, &from, &to, &w);
  if (const int st = upload(h->err, &d.up_from, from.data(), from.size())) return st;
  if (const int st = upload(h->err, &d.up_to, to.data(), to.size())) return st;
  if (const int st = upload(h->err, &d.up_w, w.data(), w.size())) return st;
  build_tables(P.word_bits, P.p, P.pinv, P.q, P.Pinv, P.pw, &from, &to, &w);
  if (const int st = upload(h->err, &d.dn_from, from.data(), from.size())) return st;
  if (const int st = upload(h->err, &d.dn_to, to.data(), to.size())) return st;
  if (const int st = upload(h->err, &d.dn_w, w.data(), w.size())) return st;
  return upload(h->err, (void **)&d.base.q, ext.data(), sizeof(uint64_t) * ext.size());
}

// what is decided before any device access
int op_args(const nttmul_ks *h, const void *out, const void *in, size_t batch) {
  if (!h) return NTTMUL_EINVAL;
  if (batch && (!out || !in)) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

uint32_t in_limbs(const nttmul_ks *h, int op) {
  return op == kKsModdown ? h->plan.L + h->plan.K : h->plan.L;
}
uint32_t out_limbs(const nttmul_ks *h, int op) {
  return op == kKsModdown ? h->plan.L : h->plan.dnum * (h->plan.L + h->plan.K);
}

// on d (the current device), stream s: the range check, then the launch
int run(nttmul_ks *h, KsDev &d, int op, void *out, const void *in, size_t batch, hipStream_t s) {
  if (!batch) return NTTMUL_OK;
  if (h->plan.flags & NTTMUL_FLAG_VALIDATE) {
    // k_rns_check_range over the input's own limbs: the first L of the moduli list for modup's,
    // all L + K for moddown's
    const uint32_t limbs = in_limbs(h, op);
    if (const int st = check_range(h->err, d.base.flag, d.base.q, limbs, h->plan.logn,
                                   h->plan.word_bits, in, (batch * limbs) << h->plan.logn, nullptr,
                                   0, "input word >= its limb's modulus", s))
      return st;
  }
  if (op == kKsModdown)
    LIMB_TRY(h->err, launch_bconv(down_tables(h, d), kBconvModdown, out, in, batch, s));
  else
    LIMB_TRY(h->err, launch_ks_modup(up_tables(h, d), out, in, batch, s));
  return NTTMUL_OK;
}

int device_op(nttmul_ks *h, int op, void *out, const void *in, size_t batch, int dev,
              void *stream) {
  if (const int st = op_args(h, out, in, batch)) return st;
  return on_device(h->err, h->dev, h->ndev, dev, [&](KsDev &d) {
    return run(h, d, op, out, in, batch, (hipStream_t)stream);
  });
}

// Host buffers: dev[0], device buffers owned by the call, the device path, copy back, synchronise
int host_op(nttmul_ks *h, int op, void *out, const void *in, size_t batch) {
  if (const int st = op_args(h, out, in, batch)) return st;
  if (!batch) return NTTMUL_OK;
  KsDev &d = h->dev[0];
  const size_t wb = (size_t)h->plan.word_bits / 8, poly = (batch << h->plan.logn) * wb;
  const Staged ops[2] = {{nullptr, out, poly * out_limbs(h, op)},
                         {in, nullptr, poly * in_limbs(h, op)}};
  return staged_op(h->err, d.base, "ks", ops, 2, [&](void *const *buf) {
    return run(h, d, op, buf[0], buf[1], batch, d.base.stream);
  });
}

}  // namespace

extern "C" {

int nttmul_ks_create(nttmul_ks **out, const nttmul_params *params, size_t size, const uint64_t *q,
                     uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs, uint32_t digit_limbs) {
  if (!out) return NTTMUL_EINVAL;
  *out = nullptr;
  nttmul_ks *h = new (std::nothrow) nttmul_ks();
  if (!h) return NTTMUL_ENOMEM;
  if (const int st = ks_validate(params, size, q, q_limbs, p, p_limbs, digit_limbs, &h->plan)) {
    delete h;
    return st;
  }
  ks_constants(&h->plan);
  DevRange R;
  if (const int st = select_devices(h->plan.prm, &R)) {
    delete h;
    return st;
  }
  DeviceGuard guard;
  for (int i = 0; i < R.ndev; i++) {
    KsDev &d = h->dev[i];
    d.base.id = R.id(i);
    h->ndev = i + 1;
    const int st = setup_device(h, d);
    if (st) {
      const int ret = create_failed("nttmul_ks", h->err, st);
      nttmul_ks_destroy(h);
      return ret;
    }
  }
  *out = h;
  return NTTMUL_OK;
}

void nttmul_ks_destroy(nttmul_ks *h) {
  if (!h) return;
  destroy_devices(h->dev, h->ndev, [](KsDev &d) {
    free_each({d.up_from, d.up_to, d.up_w, d.dn_from, d.dn_to, d.dn_w, d.base.q, d.base.flag});
  });
  delete h;
}

const char *nttmul_ks_last_error(const nttmul_ks *h) { return h ? h->err : ""; }

int nttmul_ks_get_info(const nttmul_ks *h, nttmul_ks_info *info) {
  if (!h || !info) return NTTMUL_EINVAL;
  info->n = h->plan.n;
  info->logn = h->plan.logn;
  info->q_limbs = h->plan.L;
  info->p_limbs = h->plan.K;
  info->digit_limbs = h->plan.alpha;
  info->digits = h->plan.dnum;
  info->word_bits = (uint32_t)h->plan.word_bits;
  info->ndev = h->ndev;
  return NTTMUL_OK;
}

int nttmul_ks_modup_device(nttmul_ks *h, void *out, const void *in, size_t batch, int dev,
                           void *stream) {
  return device_op(h, kKsModup, out, in, batch, dev, stream);
}
int nttmul_ks_moddown_device(nttmul_ks *h, void *out, const void *in, size_t batch, int dev,
                             void *stream) {
  return device_op(h, kKsModdown, out, in, batch, dev, stream);
}

int nttmul_ks_modup(nttmul_ks *h, void *out, const void *in, size_t batch) {
  return host_op(h, kKsModup, out, in, batch);
}
int nttmul_ks_moddown(nttmul_ks *h, void *out, const void *in, size_t batch) {
  return host_op(h, kKsModdown, out, in, batch);
}

int nttmul_ks_kernel_name(const nttmul_ks *h, int op, char *buf, size_t cap) {
  if (!h || op < kKsModup || op > kKsModdown || (cap && !buf)) return NTTMUL_EINVAL;
  std::string name;
  const hipError_t e = op == kKsModdown
                           ? describe_bconv(down_tables(h, h->dev[0]), kBconvModdown, &name)
                           : describe_ks_modup(up_tables(h, h->dev[0]), &name);
  if (e != hipSuccess) return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

}  // extern "C"
