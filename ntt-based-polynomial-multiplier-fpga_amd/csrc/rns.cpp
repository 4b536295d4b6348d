// rns.cpp — host runtime behind include/nttmul_rns.h (lib/libnttmul_rns.so only): a context of
// several moduli for one degree n <= 4096, and one launch per operation over [batch][limbs][n]
// operands (rns.hip).  It plans each limb with the planner of the plain contexts (planner.hpp) and
// keeps, per device, the limbs' twiddle tables and one table of kernel constants per kernel family
// (rns.hpp).  No resident server, no issue-priority rule, no CPU fallback.
// The create-time checks are basis.cpp's and the context runtime (devices, error text, the device
// and host forms of a call) limb_ctx.cpp's.  This file keeps its handle, its run, and the pieces
// rnsmp.cpp takes from it (rns.hpp): the limbs' tables and their upload, op_args and op_words.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "basis.hpp"
#include "limb_ctx.hpp"
#include "nttmul_rns.h"
#include "planner.hpp"
#include "rns.hpp"

using namespace nttmul;

namespace {

struct RnsDev {
  LimbDev base;
  void *tw = nullptr;                         // fw, iw of limb 0, fw, iw of limb 1, ...
  void *tab[kRnsFamilies] = {nullptr, nullptr, nullptr};
};

}  // namespace

struct nttmul_rns {
  uint32_t n = 0, logn = 0, limbs = 0, flags = 0;
  int word_bits = 0, ndev = 0;
  std::vector<Plan> plan;                     // per limb (twiddle vectors released after upload)
  RnsDev dev[kMaxDev];
  char err[kErrBytes] = {0};
};

namespace nttmul {

LaunchTables limb_tables(const Plan &P, const void *fw, const void *iw) {
  LaunchTables T;
  T.logn = P.logn;
  T.word_bits = P.word_bits;
  T.q = P.q;
  T.qinv_neg = P.qinv_neg;
  T.f = P.f; T.fs = P.fs; T.wf = P.wf; T.wfs = P.wfs;
  T.f4 = P.f4; T.f4s = P.f4s; T.wf4 = P.wf4; T.wf4s = P.wf4s;
  T.f8 = P.f8; T.f8s = P.f8s; T.wf8 = P.wf8; T.wf8s = P.wf8s;
  T.fi = P.fi; T.fis = P.fis; T.wfi = P.wfi; T.wfis = P.wfis; T.r2 = P.r2;
  T.fw = fw;
  T.iw = iw;
  T.tw_bytes = P.fw.size();
  T.cus = 0;
  return T;
}

RnsTables tables_for(uint32_t logn, uint32_t limbs, int word_bits, const void *tw,
                     void *const tab[kRnsFamilies], const uint64_t *q) {
  RnsTables T;
  T.logn = logn;
  T.limbs = limbs;
  T.word_bits = word_bits;
  for (int f = 0; f < kRnsFamilies; f++) T.tab[f] = tab[f];
  T.tw = tw;
  T.q = q;
  return T;
}

int upload_limb_tables(char *err, const std::vector<Plan> &plan, int word_bits, LimbDev &d,
                       void **tw, void *tab[kRnsFamilies],
                       hipError_t (*fill)(const LaunchTables &, int, void *)) {
  const size_t tbytes = plan[0].fw.size(), ebytes = rns_entry_bytes(word_bits);
  const uint32_t L = (uint32_t)plan.size();
  LIMB_TRY(err, hipSetDevice(d.id));
  LIMB_TRY(err, hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
  LIMB_TRY(err, hipMalloc(tw, 2 * tbytes * L));
  LIMB_TRY(err, hipMalloc((void **)&d.q, sizeof(uint64_t) * L));
  LIMB_TRY(err, hipMalloc((void **)&d.flag, sizeof(int)));
  std::vector<uint64_t> q(L);
  std::vector<uint8_t> host(ebytes * L);
  for (uint32_t l = 0; l < L; l++) {
    char *fw = (char *)*tw + 2 * tbytes * l;
    LIMB_TRY(err, hipMemcpy(fw, plan[l].fw.data(), tbytes, hipMemcpyHostToDevice));
    LIMB_TRY(err, hipMemcpy(fw + tbytes, plan[l].iw.data(), tbytes, hipMemcpyHostToDevice));
    q[l] = plan[l].q;
  }
  LIMB_TRY(err, hipMemcpy(d.q, q.data(), sizeof(uint64_t) * L, hipMemcpyHostToDevice));
  for (int f = 0; f < kRnsFamilies; f++) {
    for (uint32_t l = 0; l < L; l++) {
      const char *fw = (const char *)*tw + 2 * tbytes * l;
      LIMB_TRY(err, fill(limb_tables(plan[l], fw, fw + tbytes), f, host.data() + ebytes * l));
    }
    LIMB_TRY(err, hipMalloc(&tab[f], ebytes * L));
    LIMB_TRY(err, hipMemcpy(tab[f], host.data(), ebytes * L, hipMemcpyHostToDevice));
  }
  return NTTMUL_OK;
}

int op_args(bool have_ctx, int op, const void *c, const void *a, const void *b, size_t batch,
            uint32_t terms) {
  if (!have_ctx || (op == kRnsMac && !terms)) return NTTMUL_EINVAL;
  const bool two = op == kRnsMultiply || op == kRnsMac;
  if (batch && (!c || !a || (two && !b))) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

void op_words(uint32_t limbs, uint32_t n, int op, size_t batch, uint32_t terms, int shared,
              size_t words[3], uint32_t comps) {
  const size_t poly = (size_t)limbs * n;
  words[0] = batch * comps * poly;
  words[1] = op == kRnsMac ? batch * terms * poly : batch * poly;
  words[2] = op == kRnsMac ? (shared ? 1 : batch) * comps * terms * poly
                           : op == kRnsMultiply ? batch * poly : 0;
}

}  // namespace nttmul

namespace {

RnsTables view(const nttmul_rns *r, const RnsDev &d) {
  return tables_for(r->logn, r->limbs, r->word_bits, d.tw, d.tab, d.base.q);
}

// on d (the current device), stream s.  launch: a sibling's kernel in launch_rns's place, with
// comps operands per term (rns.hpp rns_mac_comps)
int run(nttmul_rns *r, RnsDev &d, int op, void *c, const void *a, const void *b, size_t batch,
        uint32_t terms, int shared, hipStream_t s, uint32_t comps = 1,
        RnsMacLaunch launch = nullptr, const void *aux = nullptr) {
  if (!batch) return NTTMUL_OK;
  if (r->flags & NTTMUL_FLAG_VALIDATE) {
    size_t words[3];
    op_words(r->limbs, r->n, op, batch, terms, shared, words, comps);
    if (const int st = check_range(r->err, d.base.flag, d.base.q, r->limbs, r->logn, r->word_bits,
                                   a, words[1], b, words[2],
                                   "input coefficient >= its limb's modulus", s))
      return st;
  }
  if (launch)
    LIMB_TRY(r->err, launch(view(r, d), c, a, b, batch, terms, comps, shared, s, aux));
  else
    LIMB_TRY(r->err, launch_rns(view(r, d), op, c, a, b, batch, terms, shared, s));
  return NTTMUL_OK;
}

int device_op(nttmul_rns *r, int op, void *c, const void *a, const void *b, size_t batch,
              uint32_t terms, int shared, int dev, void *stream, uint32_t comps = 1,
              RnsMacLaunch launch = nullptr, const void *aux = nullptr) {
  if (const int st = op_args(r != nullptr, op, c, a, b, batch, terms)) return st;
  return on_device(r->err, r->dev, r->ndev, dev, [&](RnsDev &d) {
    return run(r, d, op, c, a, b, batch, terms, shared, (hipStream_t)stream, comps, launch,
               aux);
  });
}

// Host buffers: dev[0], device buffers owned by the call, the device path, copy back, synchronise
int host_op(nttmul_rns *r, int op, void *c, const void *a, const void *b, size_t batch,
            uint32_t terms, int shared, uint32_t comps = 1, RnsMacLaunch launch = nullptr,
            const void *aux = nullptr) {
  if (const int st = op_args(r != nullptr, op, c, a, b, batch, terms)) return st;
  if (!batch) return NTTMUL_OK;
  RnsDev &d = r->dev[0];
  size_t words[3];
  op_words(r->limbs, r->n, op, batch, terms, shared, words, comps);
  const size_t wb = (size_t)r->word_bits / 8;
  const Staged ops[3] = {{nullptr, c, words[0] * wb}, {a, nullptr, words[1] * wb},
                         {b, nullptr, words[2] * wb}};
  return staged_op(r->err, d.base, "rns", ops, 3, [&](void *const *buf) {
    return run(r, d, op, buf[0], buf[1], buf[2], batch, terms, shared, d.base.stream, comps,
               launch, aux);
  });
}

}  // namespace

namespace nttmul {

int rns_mac_comps(nttmul_rns *r, RnsMacLaunch launch, void *c, const void *a, const void *b_hat,
                  size_t batch, uint32_t terms, uint32_t comps, int shared, int host, int dev,
                  void *stream, const void *aux) {
  if (host) return host_op(r, kRnsMac, c, a, b_hat, batch, terms, shared, comps, launch, aux);
  return device_op(r, kRnsMac, c, a, b_hat, batch, terms, shared, dev, stream, comps, launch,
                   aux);
}

}  // namespace nttmul

extern "C" {

int nttmul_rns_create(nttmul_rns **out, const nttmul_params *caller, size_t size,
                      const uint64_t *q, uint32_t limbs) {
  if (!out) return NTTMUL_EINVAL;
  *out = nullptr;
  BasisRequest B;
  if (const int st = basis_invalid(caller, size, &q, &limbs, 1, 65536, &B)) return st;
  if (const int st = basis_unsupported(&B, 256, 4096, true)) return st;
  nttmul_rns *r = new (std::nothrow) nttmul_rns();
  if (!r) return NTTMUL_ENOMEM;
  r->n = B.prm.n;
  r->limbs = limbs;
  r->flags = B.prm.flags;
  r->word_bits = B.word_bits;
  r->plan.resize(limbs);
  for (uint32_t l = 0; l < limbs; l++) {
    const int st = make_plan(r->n, q[l], 0, &r->plan[l], false);
    if (st) {
      delete r;
      return st;
    }
  }
  r->logn = r->plan[0].logn;
  DevRange R;
  if (const int st = select_devices(B.prm, &R)) {
    delete r;
    return st;
  }
  DeviceGuard guard;
  for (int i = 0; i < R.ndev; i++) {
    RnsDev &d = r->dev[i];
    d.base.id = R.id(i);
    r->ndev = i + 1;
    const int st =
        upload_limb_tables(r->err, r->plan, r->word_bits, d.base, &d.tw, d.tab, rns_fill_entry);
    if (st) {
      const int ret = create_failed("nttmul_rns", r->err, st);
      nttmul_rns_destroy(r);
      return ret;
    }
  }
  for (Plan &P : r->plan) {  // the devices hold the tables now
    std::vector<uint8_t>().swap(P.fw);
    std::vector<uint8_t>().swap(P.iw);
  }
  *out = r;
  return NTTMUL_OK;
}

void nttmul_rns_destroy(nttmul_rns *r) {
  if (!r) return;
  destroy_devices(r->dev, r->ndev, [](RnsDev &d) {
    free_each({d.tw, d.tab[0], d.tab[1], d.tab[2], d.base.q, d.base.flag});
  });
  delete r;
}

const char *nttmul_rns_last_error(const nttmul_rns *r) { return r ? r->err : ""; }

int nttmul_rns_get_info(const nttmul_rns *r, nttmul_rns_info *info) {
  if (!r || !info) return NTTMUL_EINVAL;
  info->n = r->n;
  info->logn = r->logn;
  info->limbs = r->limbs;
  info->word_bits = (uint32_t)r->word_bits;
  info->ndev = r->ndev;
  return NTTMUL_OK;
}

int nttmul_rns_limb_info(const nttmul_rns *r, uint32_t limb, nttmul_info *info) {
  if (!r || !info || limb >= r->limbs) return NTTMUL_EINVAL;
  fill_info(r->plan[limb], r->ndev, 1, info);
  return NTTMUL_OK;
}

int nttmul_rns_multiply_device(nttmul_rns *r, void *c, const void *a, const void *b, size_t batch,
                               int dev, void *stream) {
  return device_op(r, kRnsMultiply, c, a, b, batch, 1, 0, dev, stream);
}
int nttmul_rns_forward_device(nttmul_rns *r, void *out, const void *in, size_t batch, int dev,
                              void *stream) {
  return device_op(r, kRnsForward, out, in, nullptr, batch, 1, 0, dev, stream);
}
int nttmul_rns_inverse_device(nttmul_rns *r, void *out, const void *in, size_t batch, int dev,
                              void *stream) {
  return device_op(r, kRnsInverseOp, out, in, nullptr, batch, 1, 0, dev, stream);
}
int nttmul_rns_mac_ntt_device(nttmul_rns *r, void *c, const void *a, const void *b_hat,
                              size_t batch, uint32_t terms, int shared, int dev, void *stream) {
  return device_op(r, kRnsMac, c, a, b_hat, batch, terms, shared, dev, stream);
}

int nttmul_rns_multiply(nttmul_rns *r, void *c, const void *a, const void *b, size_t batch) {
  return host_op(r, kRnsMultiply, c, a, b, batch, 1, 0);
}
int nttmul_rns_forward(nttmul_rns *r, void *out, const void *in, size_t batch) {
  return host_op(r, kRnsForward, out, in, nullptr, batch, 1, 0);
}
int nttmul_rns_inverse(nttmul_rns *r, void *out, const void *in, size_t batch) {
  return host_op(r, kRnsInverseOp, out, in, nullptr, batch, 1, 0);
}
int nttmul_rns_mac_ntt(nttmul_rns *r, void *c, const void *a, const void *b_hat, size_t batch,
                       uint32_t terms, int shared) {
  return host_op(r, kRnsMac, c, a, b_hat, batch, terms, shared);
}

int nttmul_rns_kernel_name(const nttmul_rns *r, int op, char *buf, size_t cap) {
  if (!r || op < kRnsMultiply || op > kRnsMac || (cap && !buf)) return NTTMUL_EINVAL;
  std::string name;
  if (describe_rns(view(r, r->dev[0]), op, &name) != hipSuccess) return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

}  // extern "C"
