// rnsmp.cpp — host runtime behind include/nttmul_rnsmp.h (lib/libnttmul_rnsmp.so only): a context
// of several moduli for one degree 4096 < n <= 65536, and the two or three launches per operation
// over [batch][limbs][n] operands (rnsmp.hip).  It plans each limb with the planner of the plain
// contexts (planner.hpp) and keeps, per device, the limbs' twiddle tables in one allocation, one
// table of kernel constants per kernel family (rns.hpp) and one scratch for the intermediates of
// the passes.  No resident server, no issue-priority rule, no CPU fallback.
// The create-time checks are basis.cpp's, the context runtime limb_ctx.cpp's, and the limbs'
// tables, their upload, op_args and op_words rns.cpp's (rns.hpp).  This file keeps its handle and
// what only it has: the scratch (MpScratch, ensure, its event hand-over and its frees) and the
// sub-batch loop of run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "basis.hpp"
#include "limb_ctx.hpp"
#include "nttmul_rnsmp.h"
#include "planner.hpp"
#include "rnsmp.hpp"
#include "subbatch.hpp"

using namespace nttmul;

namespace {

// The intermediates of the passes: buf[0] the column-passed a (the mac: all terms), buf[1] the
// column-passed b of a product, buf[2] the row pass's output.  Each grows on demand to the
// sub-batch of the call.  Every use is ordered after the previous one by `ev`, whatever stream it
// was enqueued on (the plain context's Scratch, nttmul.cpp).
struct MpScratch {
  void *buf[3] = {nullptr, nullptr, nullptr};
  size_t bytes[3] = {0, 0, 0};
  hipEvent_t ev = nullptr;                    // recorded after the last enqueued use
  bool used = false;
  hipStream_t last = nullptr;                 // stream of that use
};

struct MpDev {
  LimbDev base;
  void *tw = nullptr;                         // fw, iw of limb 0, fw, iw of limb 1, ...
  void *tab[kRnsFamilies] = {nullptr, nullptr, nullptr};
  MpScratch scr;
};

}  // namespace

struct nttmul_rnsmp {
  uint32_t n = 0, logn = 0, limbs = 0, flags = 0, scratch_mb = 512;
  int word_bits = 0, ndev = 0;
  std::vector<Plan> plan;                     // per limb (twiddle vectors released after upload)
  MpDev dev[kMaxDev];
  char err[kErrBytes] = {0};
};

namespace {

RnsTables view(const nttmul_rnsmp *r, const MpDev &d) {
  return tables_for(r->logn, r->limbs, r->word_bits, d.tw, d.tab, d.base.q);
}

// One device's tables (rns.hpp upload_limb_tables), n pairs each of fw, iw per limb: the kernels
// form the twiddle pointers from the allocation's base; the entries' own fw / iw hold the same
// addresses.
int setup_device(nttmul_rnsmp *r, MpDev &d) {
  if (r->plan[0].fw.size() != (size_t)r->n * 2 * (r->word_bits / 8)) {
    set_err(r->err, "planner twiddle table is not n pairs");
    return NTTMUL_EUNSUPPORTED;
  }
  return upload_limb_tables(r->err, r->plan, r->word_bits, d.base, &d.tw, d.tab,
                            rnsmp_fill_entry);
}

// Scratch buffer i of at least `need` bytes; its last use must have completed before the old one
// is freed
int ensure(nttmul_rnsmp *r, MpScratch &sc, int i, size_t need) {
  if (sc.bytes[i] >= need) return NTTMUL_OK;
  if (sc.used) LIMB_TRY(r->err, hipEventSynchronize(sc.ev));
  if (sc.buf[i]) (void)hipFree(sc.buf[i]);
  sc.buf[i] = nullptr;
  sc.bytes[i] = 0;
  LIMB_TRY(r->err, hipMalloc(&sc.buf[i], need));
  sc.bytes[i] = need;
  return NTTMUL_OK;
}

// A call's first use of the scratch on stream s: ordered after the last enqueued use, whatever
// stream that was on
int scratch_begin(nttmul_rnsmp *r, MpScratch &sc, hipStream_t s) {
  if (!sc.ev) LIMB_TRY(r->err, hipEventCreateWithFlags(&sc.ev, hipEventDisableTiming));
  if (sc.used && sc.last != s) LIMB_TRY(r->err, hipStreamWaitEvent(s, sc.ev, 0));
  return NTTMUL_OK;
}

// After a call's launches, also after a failure (what was enqueued still uses the scratch): the
// event the next use waits for.  st: the call's status so far, returned unless it was OK
int scratch_end(nttmul_rnsmp *r, MpScratch &sc, hipStream_t s, int st) {
  const hipError_t e = hipEventRecord(sc.ev, s);
  sc.used = true;
  sc.last = s;
  if (!st && e != hipSuccess) st = fail(r->err, e, "hipEventRecord(scratch)");
  return st;
}

// NTTMUL_FLAG_VALIDATE: a_words of a and b_words of b against their limbs' moduli
int validate(nttmul_rnsmp *r, MpDev &d, const void *a, size_t a_words, const void *b,
             size_t b_words, hipStream_t s) {
  if (!(r->flags & NTTMUL_FLAG_VALIDATE)) return NTTMUL_OK;
  return check_range(r->err, d.base.flag, d.base.q, r->limbs, r->logn, r->word_bits, a, a_words, b,
                     b_words, "input coefficient >= its limb's modulus", s);
}

// on d (the current device), stream s: the range check, then sub-batches of whole polynomials
// through the scratch.  launch: a sibling's launches in launch_rnsmp's place, with comps operands
// per term and as many output polynomials per batch entry (rnsmp.hpp rnsmp_mac_comps)
int run(nttmul_rnsmp *r, MpDev &d, int op, void *c, const void *a, const void *b, size_t batch,
        uint32_t terms, int shared, hipStream_t s, uint32_t comps = 1,
        MpMacLaunch launch = nullptr) {
  if (!batch) return NTTMUL_OK;
  const RnsTables T = view(r, d);
  size_t words[3];
  op_words(r->limbs, r->n, op, batch, terms, shared, words, comps);
  if (const int st = validate(r, d, a, words[1], b, words[2], s)) return st;
  // bytes of one polynomial (all limbs) in a scratch buffer, of one polynomial's a (for the mac
  // all its terms) and of its output (all components), so that no scratch buffer of a sub-batch
  // exceeds scratch_mb
  const size_t poly = (size_t)r->limbs * r->n * (r->word_bits / 8);
  const size_t apoly = op == kRnsMac ? poly * terms : poly, cpoly = poly * comps;
  const size_t chunk = mp_chunk((size_t)r->scratch_mb << 20, apoly, cpoly, batch);
  MpScratch &sc = d.scr;
  if (const int st = scratch_begin(r, sc, s)) return st;
  const bool two = op == kRnsMultiply, three = op == kRnsMultiply || op == kRnsMac;
  int st = ensure(r, sc, 0, chunk * apoly);
  if (!st && two) st = ensure(r, sc, 1, chunk * poly);
  if (!st && three) st = ensure(r, sc, 2, chunk * cpoly);
  if (st) return st;
  const size_t bstep = op == kRnsMac ? (shared ? 0 : apoly * comps) : poly;
  for (size_t k = 0; k < mp_subs(batch, chunk) && !st; k++) {
    const MpSub u = mp_sub(batch, chunk, k);
    void *cu = (char *)c + u.p * cpoly;
    const void *au = (const char *)a + u.p * apoly;
    const void *bu = b ? (const char *)b + u.p * bstep : nullptr;
    const hipError_t e =
        launch ? launch(T, cu, au, bu, u.cnt, terms, comps, shared, sc.buf, s)
               : launch_rnsmp(T, op, cu, au, bu, u.cnt, terms, shared, sc.buf, s);
    if (e != hipSuccess) st = fail(r->err, e, "sub-batch launch");
  }
  return scratch_end(r, sc, s, st);
}

int device_op(nttmul_rnsmp *r, int op, void *c, const void *a, const void *b, size_t batch,
              uint32_t terms, int shared, int dev, void *stream, uint32_t comps = 1,
              MpMacLaunch launch = nullptr) {
  if (const int st = op_args(r != nullptr, op, c, a, b, batch, terms)) return st;
  return on_device(r->err, r->dev, r->ndev, dev, [&](MpDev &d) {
    return run(r, d, op, c, a, b, batch, terms, shared, (hipStream_t)stream, comps, launch);
  });
}

// Host buffers: dev[0], device buffers owned by the call, the device path, copy back, synchronise
int host_op(nttmul_rnsmp *r, int op, void *c, const void *a, const void *b, size_t batch,
            uint32_t terms, int shared, uint32_t comps = 1, MpMacLaunch launch = nullptr) {
  if (const int st = op_args(r != nullptr, op, c, a, b, batch, terms)) return st;
  if (!batch) return NTTMUL_OK;
  MpDev &d = r->dev[0];
  size_t words[3];
  op_words(r->limbs, r->n, op, batch, terms, shared, words, comps);
  const size_t wb = (size_t)r->word_bits / 8;
  const Staged ops[3] = {{nullptr, c, words[0] * wb}, {a, nullptr, words[1] * wb},
                         {b, nullptr, words[2] * wb}};
  return staged_op(r->err, d.base, "rnsmp", ops, 3, [&](void *const *buf) {
    return run(r, d, op, buf[0], buf[1], buf[2], batch, terms, shared, d.base.stream, comps,
               launch);
  });
}

}  // namespace

namespace nttmul {

int rnsmp_mac_comps(nttmul_rnsmp *r, MpMacLaunch launch, void *c, const void *a, const void *b_hat,
                    size_t batch, uint32_t terms, uint32_t comps, int shared, int host, int dev,
                    void *stream) {
  if (host) return host_op(r, kRnsMac, c, a, b_hat, batch, terms, shared, comps, launch);
  return device_op(r, kRnsMac, c, a, b_hat, batch, terms, shared, dev, stream, comps, launch);
}

}  // namespace nttmul

namespace {

// rnsmp_units_op on d (the current device), stream s: the range check, then sub-batches of whole
// output units through scr[2]
int run_units(nttmul_rnsmp *r, MpDev &d, MpUnitsLaunch launch, const void *aux, void *c,
              const void *a, const void *b, size_t batch, uint32_t terms, uint32_t upb,
              uint32_t comps, hipStream_t s) {
  if (!batch) return NTTMUL_OK;
  const RnsTables T = view(r, d);
  size_t words[3];
  mp_unit_words(r->limbs, r->n, batch, terms, upb, comps, words);
  if (const int st = validate(r, d, a, words[1], b, words[2], s)) return st;
  const size_t poly = (size_t)r->limbs * r->n * (r->word_bits / 8);
  const size_t cunit = poly * comps, units = batch * upb;
  const size_t chunk = mp_unit_chunk((size_t)r->scratch_mb << 20, poly, comps, units);
  MpScratch &sc = d.scr;
  if (const int st = scratch_begin(r, sc, s)) return st;
  int st = ensure(r, sc, 2, chunk * cunit);
  if (st) return st;
  for (size_t k = 0; k < mp_subs(units, chunk) && !st; k++) {
    const MpSub u = mp_sub(units, chunk, k);
    const hipError_t e =
        launch(T, (char *)c + u.p * cunit, a, b, u.p, u.cnt, terms, aux, sc.buf, s);
    if (e != hipSuccess) st = fail(r->err, e, "sub-batch launch");
  }
  return scratch_end(r, sc, s, st);
}

}  // namespace

namespace nttmul {

int rnsmp_units_op(nttmul_rnsmp *r, MpUnitsLaunch launch, const void *aux, void *c, const void *a,
                   const void *b, size_t batch, uint32_t terms, uint32_t upb, uint32_t comps,
                   int host, int dev, void *stream) {
  if (!host)
    return on_device(r->err, r->dev, r->ndev, dev, [&](MpDev &d) {
      return run_units(r, d, launch, aux, c, a, b, batch, terms, upb, comps,
                       (hipStream_t)stream);
    });
  if (!batch) return NTTMUL_OK;
  MpDev &d = r->dev[0];
  size_t words[3];
  mp_unit_words(r->limbs, r->n, batch, terms, upb, comps, words);
  const size_t wb = (size_t)r->word_bits / 8;
  const Staged ops[3] = {{nullptr, c, words[0] * wb}, {a, nullptr, words[1] * wb},
                         {b, nullptr, words[2] * wb}};
  return staged_op(r->err, d.base, "rnsmp", ops, 3, [&](void *const *buf) {
    return run_units(r, d, launch, aux, buf[0], buf[1], buf[2], batch, terms, upb, comps,
                     d.base.stream);
  });
}

}  // namespace nttmul

extern "C" {

int nttmul_rnsmp_create(nttmul_rnsmp **out, const nttmul_params *caller, size_t size,
                        const uint64_t *q, uint32_t limbs) {
  if (!out) return NTTMUL_EINVAL;
  *out = nullptr;
  // a degree above 65536 is valid and unsupported; n <= 4096 is nttmul_rns_*'s
  // (include/nttmul_rns.h, lib/libnttmul_rns.so).  No Arith32P3 above n = 4096
  BasisRequest B;
  if (const int st = basis_invalid(caller, size, &q, &limbs, 1, 1u << 30, &B)) return st;
  if (const int st = basis_unsupported(&B, 8192, 65536, false)) return st;
  nttmul_rnsmp *r = new (std::nothrow) nttmul_rnsmp();
  if (!r) return NTTMUL_ENOMEM;
  r->n = B.prm.n;
  r->limbs = limbs;
  r->flags = B.prm.flags;
  r->scratch_mb = B.prm.scratch_mb ? B.prm.scratch_mb : 512;
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
    MpDev &d = r->dev[i];
    d.base.id = R.id(i);
    r->ndev = i + 1;
    const int st = setup_device(r, d);
    if (st) {
      const int ret = create_failed("nttmul_rnsmp", r->err, st);
      nttmul_rnsmp_destroy(r);
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

void nttmul_rnsmp_destroy(nttmul_rnsmp *r) {
  if (!r) return;
  destroy_devices(r->dev, r->ndev, [](MpDev &d) {
    // the last enqueued use of the scratch, not the caller's streams
    if (d.scr.used) (void)hipEventSynchronize(d.scr.ev);
    free_each({d.scr.buf[0], d.scr.buf[1], d.scr.buf[2], d.tw, d.tab[0], d.tab[1], d.tab[2],
               d.base.q, d.base.flag});
    if (d.scr.ev) (void)hipEventDestroy(d.scr.ev);
  });
  delete r;
}

const char *nttmul_rnsmp_last_error(const nttmul_rnsmp *r) { return r ? r->err : ""; }

int nttmul_rnsmp_get_info(const nttmul_rnsmp *r, nttmul_rnsmp_info *info) {
  if (!r || !info) return NTTMUL_EINVAL;
  info->n = r->n;
  info->logn = r->logn;
  info->limbs = r->limbs;
  info->word_bits = (uint32_t)r->word_bits;
  info->ndev = r->ndev;
  info->scratch_mb = r->scratch_mb;
  return NTTMUL_OK;
}

int nttmul_rnsmp_limb_info(const nttmul_rnsmp *r, uint32_t limb, nttmul_info *info) {
  if (!r || !info || limb >= r->limbs) return NTTMUL_EINVAL;
  fill_info(r->plan[limb], r->ndev, 1, info);
  return NTTMUL_OK;
}

int nttmul_rnsmp_multiply_device(nttmul_rnsmp *r, void *c, const void *a, const void *b,
                                 size_t batch, int dev, void *stream) {
  return device_op(r, kRnsMultiply, c, a, b, batch, 1, 0, dev, stream);
}
int nttmul_rnsmp_forward_device(nttmul_rnsmp *r, void *out, const void *in, size_t batch, int dev,
                                void *stream) {
  return device_op(r, kRnsForward, out, in, nullptr, batch, 1, 0, dev, stream);
}
int nttmul_rnsmp_inverse_device(nttmul_rnsmp *r, void *out, const void *in, size_t batch, int dev,
                                void *stream) {
  return device_op(r, kRnsInverseOp, out, in, nullptr, batch, 1, 0, dev, stream);
}
int nttmul_rnsmp_mac_ntt_device(nttmul_rnsmp *r, void *c, const void *a, const void *b_hat,
                                size_t batch, uint32_t terms, int shared, int dev, void *stream) {
  return device_op(r, kRnsMac, c, a, b_hat, batch, terms, shared, dev, stream);
}

int nttmul_rnsmp_multiply(nttmul_rnsmp *r, void *c, const void *a, const void *b, size_t batch) {
  return host_op(r, kRnsMultiply, c, a, b, batch, 1, 0);
}
int nttmul_rnsmp_forward(nttmul_rnsmp *r, void *out, const void *in, size_t batch) {
  return host_op(r, kRnsForward, out, in, nullptr, batch, 1, 0);
}
int nttmul_rnsmp_inverse(nttmul_rnsmp *r, void *out, const void *in, size_t batch) {
  return host_op(r, kRnsInverseOp, out, in, nullptr, batch, 1, 0);
}
int nttmul_rnsmp_mac_ntt(nttmul_rnsmp *r, void *c, const void *a, const void *b_hat, size_t batch,
                         uint32_t terms, int shared) {
  return host_op(r, kRnsMac, c, a, b_hat, batch, terms, shared);
}

int nttmul_rnsmp_kernel_name(const nttmul_rnsmp *r, int op, char *buf, size_t cap) {
  if (!r || op < kRnsMultiply || op > kRnsMac || (cap && !buf)) return NTTMUL_EINVAL;
  std::string name;
  if (describe_rnsmp(view(r, r->dev[0]), op, &name) != hipSuccess) return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

}  // extern "C"
