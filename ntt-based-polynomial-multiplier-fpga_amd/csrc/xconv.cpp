// xconv.cpp — host runtime behind include/nttmul_xconv.h (lib/libnttmul_xconv.so only): a context
// of the bases Q and P and a scale t for one degree 256 <= n <= 65536, and the two or four
// launches per sub-batch of xconv.hip.  The create-time checks and the plain constants are
// xconv_plan.hpp's (basis.cpp's checks through mdntt_plan.hpp), the context runtime limb_ctx.cpp's,
// the limbs' plans and their upload planner.cpp's and rns.cpp's (upload_limb_tables over the
// extended basis Q u P), the conversion tables' device form bconv.hpp's build_tables.  This file
// keeps its handle and what only it has: the inverse's table with t Ph_j^-1 folded into its scale,
// the two weight tables with the correction's row, the table of 1 / p_j, the scratch (as
// mdntt.cpp's: grown on demand, handed between streams by an event) and the sub-batch loop of
// run.  No CPU fallback.
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "limb_ctx.hpp"
#include "nttmul_xconv.h"
#include "planner.hpp"
#include "xconv.hpp"
#include "xconv_plan.hpp"

using namespace nttmul;

namespace {

struct XcScr {
  void *buf[kMdScratch] = {nullptr, nullptr, nullptr};
  size_t bytes[kMdScratch] = {0, 0, 0};
  hipEvent_t ev = nullptr;     // recorded after the last enqueued use
  bool used = false;
  hipStream_t last = nullptr;  // stream of that use
};

struct XcDev {
  LimbDev base;                // q: q_0 .. q_{L-1}, p_0 .. p_{K-1}
  void *tw = nullptr;          // fw, iw of limb 0, fw, iw of limb 1, ... over Q u P
  void *tab[kRnsFamilies] = {nullptr, nullptr, nullptr};  // over Q u P (upload_limb_tables)
  void *tab_inv = nullptr;     // P's limbs, the scale n^-1 Ph_j^-1 t
  void *to = nullptr;          // build_tables(to = Q) with t P^-1 as the entries' factor
  void *w[2] = {nullptr, nullptr};  // per XcOp: K + 1 rows
  void *ip = nullptr;          // double [K]: 1 / p_j
  XcScr scr;
};

}  // namespace

struct nttmul_xconv {
  XcPlan xc;
  uint32_t scratch_mb = 512;
  int ndev = 0;
  std::vector<Plan> plan;      // per limb of Q u P (twiddle vectors released after upload)
  XcDev dev[kMaxDev];
  char err[kErrBytes] = {0};
};

namespace {

XcTables view(const nttmul_xconv *h, const XcDev &d) {
  XcTables T;
  T.logn = h->xc.logn;
  T.L = h->xc.L;
  T.K = h->xc.K;
  T.word_bits = h->xc.word_bits;
  T.tab_fwd = d.tab[kRnsTransform];
  T.tab_inv = d.tab_inv;
  T.tw = d.tw;
  T.to = d.to;
  T.w[kXcExtend] = d.w[kXcExtend];
  T.w[kXcModdown] = d.w[kXcModdown];
  T.ip = (const double *)d.ip;
  return T;
}

hipError_t fill_entry(const LaunchTables &T, int fam, void *dst) {
  return T.logn <= 12 ? rns_fill_entry(T, fam, dst) : rnsmp_fill_entry(T, fam, dst);
}

// The inverse's table for the K limbs of P: mdntt.cpp upload_inv_table's with t Ph_j^-1 where it
// folds Ph_j^-1
int upload_inv_table(nttmul_xconv *h, XcDev &d) {
  const XcPlan &P = h->xc;
  const size_t ebytes = rns_entry_bytes(P.word_bits), tbytes = h->plan[0].fw.size();
  std::vector<uint8_t> host(ebytes * P.K);
  for (uint32_t j = 0; j < P.K; j++) {
    const Plan &pl = h->plan[P.L + j];
    const char *fw = (const char *)d.tw + 2 * tbytes * (P.L + j);
    LaunchTables T = limb_tables(pl, fw, fw + tbytes);
    const uint64_t f = mulmod(pl.inv_n, P.yscale[j], pl.q);
    const uint64_t iw1 = powmod(pl.inv_psi, pl.n / 2, pl.q);
    tw_pair(f, pl.q, pl.word_bits, &T.fi, &T.fis);
    tw_pair(mulmod(iw1, f, pl.q), pl.q, pl.word_bits, &T.wfi, &T.wfis, true);
    LIMB_TRY(h->err, fill_entry(T, kRnsInverse, host.data() + ebytes * j));
  }
  return upload(h->err, &d.tab_inv, host.data(), host.size());
}

int setup_device(nttmul_xconv *h, XcDev &d) {
  const XcPlan &P = h->xc;
  if (h->plan[0].fw.size() != (size_t)P.n * 2 * (P.word_bits / 8)) {
    set_err(h->err, "planner twiddle table is not n pairs");
    return NTTMUL_EUNSUPPORTED;
  }
  if (const int st = upload_limb_tables(h->err, h->plan, P.word_bits, d.base, &d.tw, d.tab,
                                        fill_entry))
    return st;
  if (const int st = upload_inv_table(h, d)) return st;
  // K + 1 `from` rows: the limbs of P and the correction's.  The `from` entries themselves are not
  // needed (t Ph_j^-1 is in tab_inv's scale); the last one only has to be well formed
  std::vector<uint64_t> b(P.p), binv(P.yscale);
  b.push_back(P.p[0]);
  binv.push_back(1);
  std::vector<uint8_t> from, to, w;
  build_tables(P.word_bits, b, binv, P.q, P.v, P.w_md, &from, &to, &w);
  if (const int st = upload(h->err, &d.to, to.data(), to.size())) return st;
  if (const int st = upload(h->err, &d.w[kXcModdown], w.data(), w.size())) return st;
  build_tables(P.word_bits, b, binv, P.q, P.v, P.w_ext, &from, &to, &w);
  if (const int st = upload(h->err, &d.w[kXcExtend], w.data(), w.size())) return st;
  std::vector<double> ip(P.K);
  for (uint32_t j = 0; j < P.K; j++) ip[j] = 1.0 / (double)P.p[j];
  return upload(h->err, &d.ip, ip.data(), ip.size() * sizeof(double));
}

// Scratch buffer i of at least `need` bytes; its last use must have completed before the old one
// is freed (mdntt.cpp ensure)
int ensure(nttmul_xconv *h, XcScr &sc, int i, size_t need) {
  if (sc.bytes[i] >= need) return NTTMUL_OK;
  if (sc.used) LIMB_TRY(h->err, hipEventSynchronize(sc.ev));
  if (sc.buf[i]) (void)hipFree(sc.buf[i]);
  sc.buf[i] = nullptr;
  sc.bytes[i] = 0;
  LIMB_TRY(h->err, hipMalloc(&sc.buf[i], need));
  sc.bytes[i] = need;
  return NTTMUL_OK;
}

// on d (the current device), stream s: the range check, then sub-batches of whole polynomials
// through the scratch
int run(nttmul_xconv *h, XcDev &d, int op, void *out, const void *in, size_t batch,
        hipStream_t s) {
  if (!batch) return NTTMUL_OK;
  const XcPlan &P = h->xc;
  const MdShape S =
      xconv_shape((size_t)h->scratch_mb << 20, P.n, P.L, P.K, P.word_bits, batch, op);
  if (P.flags & NTTMUL_FLAG_VALIDATE) {
    // extend's operand holds the limbs of P alone: the moduli from the L-th on
    const uint64_t *mod = op == kXcExtend ? d.base.q + P.L : d.base.q;
    const uint32_t limbs = op == kXcExtend ? P.K : P.L + P.K;
    if (const int st = check_range(h->err, d.base.flag, mod, limbs, P.logn, P.word_bits, in,
                                   batch * S.in_words, nullptr, 0,
                                   "input word >= its limb's modulus", s))
      return st;
  }
  XcScr &sc = d.scr;
  // a call's first use of the scratch on s: ordered after the last enqueued use, whatever stream
  // that was on
  if (!sc.ev) LIMB_TRY(h->err, hipEventCreateWithFlags(&sc.ev, hipEventDisableTiming));
  if (sc.used && sc.last != s) LIMB_TRY(h->err, hipStreamWaitEvent(s, sc.ev, 0));
  int st = ensure(h, sc, kMdY, S.chunk * S.y_bytes);
  if (!st && S.t_bytes) st = ensure(h, sc, kMdYLazy, S.chunk * S.y_bytes);
  if (!st && S.t_bytes) st = ensure(h, sc, kMdT, S.chunk * S.t_bytes);
  if (st) return st;
  const XcTables T = view(h, d);
  const size_t wb = (size_t)P.word_bits / 8;
  for (size_t k = 0; k < S.subs && !st; k++) {
    const MpSub u = mp_sub(batch, S.chunk, k);
    const hipError_t e = launch_xconv(T, op, (char *)out + u.p * S.out_words * wb,
                                      (const char *)in + u.p * S.in_words * wb, u.cnt, sc.buf, s);
    if (e != hipSuccess) st = fail(h->err, e, "sub-batch launch");
  }
  // also after a failure: what was enqueued still uses the scratch
  const hipError_t e = hipEventRecord(sc.ev, s);
  sc.used = true;
  sc.last = s;
  if (!st && e != hipSuccess) st = fail(h->err, e, "hipEventRecord(scratch)");
  return st;
}

int run_device(nttmul_xconv *h, int op, void *out, const void *in, size_t batch, int dev,
               void *stream) {
  if (const int st = xconv_call_status(h != nullptr, out, in, batch)) return st;
  return on_device(h->err, h->dev, h->ndev, dev, [&](XcDev &d) {
    return run(h, d, op, out, in, batch, (hipStream_t)stream);
  });
}

int run_host(nttmul_xconv *h, int op, void *out, const void *in, size_t batch) {
  if (const int st = xconv_call_status(h != nullptr, out, in, batch)) return st;
  if (!batch) return NTTMUL_OK;
  XcDev &d = h->dev[0];
  const size_t poly = ((size_t)batch << h->xc.logn) * (h->xc.word_bits / 8);
  const uint32_t in_limbs = op == kXcExtend ? h->xc.K : h->xc.L + h->xc.K;
  const Staged ops[2] = {{nullptr, out, poly * h->xc.L}, {in, nullptr, poly * in_limbs}};
  return staged_op(h->err, d.base, "xconv", ops, 2, [&](void *const *buf) {
    return run(h, d, op, buf[0], buf[1], batch, d.base.stream);
  });
}

}  // namespace

extern "C" {

int nttmul_xconv_create(nttmul_xconv **out, const nttmul_params *params, size_t size,
                        const uint64_t *q, uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs,
                        uint64_t scale) {
  if (!out) return NTTMUL_EINVAL;
  *out = nullptr;
  nttmul_xconv *h = new (std::nothrow) nttmul_xconv();
  if (!h) return NTTMUL_ENOMEM;
  if (const int st = xconv_validate(params, size, q, q_limbs, p, p_limbs, scale, &h->xc)) {
    delete h;
    return st;
  }
  xconv_constants(&h->xc);
  h->scratch_mb = h->xc.prm.scratch_mb ? h->xc.prm.scratch_mb : 512;
  const uint32_t M = q_limbs + p_limbs;
  h->plan.resize(M);
  for (uint32_t l = 0; l < M; l++) {
    const int st = make_plan(h->xc.n, h->xc.modulus(l), 0, &h->plan[l], false);
    if (st) {
      delete h;
      return st;
    }
  }
  DevRange R;
  if (const int st = select_devices(h->xc.prm, &R)) {
    delete h;
    return st;
  }
  DeviceGuard guard;
  for (int i = 0; i < R.ndev; i++) {
    XcDev &d = h->dev[i];
    d.base.id = R.id(i);
    h->ndev = i + 1;
    const int st = setup_device(h, d);
    if (st) {
      const int ret = create_failed("nttmul_xconv", h->err, st);
      nttmul_xconv_destroy(h);
      return ret;
    }
  }
  for (Plan &P : h->plan) {  // the devices hold the tables now
    std::vector<uint8_t>().swap(P.fw);
    std::vector<uint8_t>().swap(P.iw);
  }
  *out = h;
  return NTTMUL_OK;
}

void nttmul_xconv_destroy(nttmul_xconv *h) {
  if (!h) return;
  destroy_devices(h->dev, h->ndev, [](XcDev &d) {
    // the last enqueued use of the scratch, not the caller's streams
    if (d.scr.used) (void)hipEventSynchronize(d.scr.ev);
    free_each({d.scr.buf[0], d.scr.buf[1], d.scr.buf[2], d.tw, d.tab[0], d.tab[1], d.tab[2],
               d.tab_inv, d.to, d.w[0], d.w[1], d.ip, d.base.q, d.base.flag});
    if (d.scr.ev) (void)hipEventDestroy(d.scr.ev);
  });
  delete h;
}

const char *nttmul_xconv_last_error(const nttmul_xconv *h) { return h ? h->err : ""; }

int nttmul_xconv_get_info(const nttmul_xconv *h, nttmul_xconv_info *info) {
  if (!h || !info) return NTTMUL_EINVAL;
  info->n = h->xc.n;
  info->logn = h->xc.logn;
  info->q_limbs = h->xc.L;
  info->p_limbs = h->xc.K;
  info->word_bits = (uint32_t)h->xc.word_bits;
  info->ndev = h->ndev;
  info->scratch_mb = h->scratch_mb;
  info->band_log2 = kXcBandLog2;
  info->scale = h->xc.scale;
  return NTTMUL_OK;
}

int nttmul_xconv_extend_device(nttmul_xconv *h, void *out, const void *p_hat, size_t batch,
                               int dev, void *stream) {
  return run_device(h, kXcExtend, out, p_hat, batch, dev, stream);
}

int nttmul_xconv_moddown_device(nttmul_xconv *h, void *out, const void *x_hat, size_t batch,
                                int dev, void *stream) {
  return run_device(h, kXcModdown, out, x_hat, batch, dev, stream);
}

int nttmul_xconv_extend(nttmul_xconv *h, void *out, const void *p_hat, size_t batch) {
  return run_host(h, kXcExtend, out, p_hat, batch);
}

int nttmul_xconv_moddown(nttmul_xconv *h, void *out, const void *x_hat, size_t batch) {
  return run_host(h, kXcModdown, out, x_hat, batch);
}

int nttmul_xconv_plan(const nttmul_params *params, size_t size, const uint64_t *q,
                      uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs, uint64_t scale,
                      uint64_t *yscale, uint64_t *w_ext, uint64_t *w_md, uint64_t *v) {
  XcPlan P;
  if (const int st = xconv_validate(params, size, q, q_limbs, p, p_limbs, scale, &P)) return st;
  xconv_constants(&P);
  const auto copy = [](uint64_t *dst, const std::vector<uint64_t> &src) {
    if (dst) memcpy(dst, src.data(), sizeof(uint64_t) * src.size());
  };
  copy(yscale, P.yscale);
  copy(w_ext, P.w_ext);
  copy(w_md, P.w_md);
  copy(v, P.v);
  return NTTMUL_OK;
}

int nttmul_xconv_kernel_name(const nttmul_xconv *h, int op, char *buf, size_t cap) {
  if (!h || op < NTTMUL_XCONV_EXTEND || op > NTTMUL_XCONV_MODDOWN || (cap && !buf))
    return NTTMUL_EINVAL;
  std::string name;
  if (describe_xconv(view(h, h->dev[0]), op, &name) != hipSuccess) return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

}  // extern "C"
