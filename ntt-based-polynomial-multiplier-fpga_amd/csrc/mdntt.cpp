// mdntt.cpp — host runtime behind include/nttmul_mdntt.h (lib/libnttmul_mdntt.so only): a context
// of the bases Q and P for one degree 256 <= n <= 65536, and the two or four launches per
// sub-batch of mdntt.hip.  The create-time checks are basis.cpp's (through mdntt_plan.hpp), the
// context runtime limb_ctx.cpp's, the limbs' plans and their upload planner.cpp's and rns.cpp's
// (upload_limb_tables over the extended basis Q u P), the conversion constants ks_plan.cpp's and
// their device form bconv.hpp's build_tables.  This file keeps its handle and what only it has:
// the inverse's table with Ph_j^-1 folded into its scale, the scratch (as rnsmp.cpp's: grown on
// demand, handed between streams by an event) and the sub-batch loop of run.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "ks_plan.hpp"
#include "limb_ctx.hpp"
#include "mdntt.hpp"
#include "mdntt_plan.hpp"
#include "nttmul_mdntt.h"
#include "planner.hpp"

using namespace nttmul;

namespace {

struct MdScr {
  void *buf[kMdScratch] = {nullptr, nullptr, nullptr};
  size_t bytes[kMdScratch] = {0, 0, 0};
  hipEvent_t ev = nullptr;     // recorded after the last enqueued use
  bool used = false;
  hipStream_t last = nullptr;  // stream of that use
};

struct MdDev {
  LimbDev base;                // q: q_0 .. q_{L-1}, p_0 .. p_{K-1}
  void *tw = nullptr;          // fw, iw of limb 0, fw, iw of limb 1, ... over Q u P
  void *tab[kRnsFamilies] = {nullptr, nullptr, nullptr};  // over Q u P (upload_limb_tables)
  void *tab_inv = nullptr;     // P's limbs, the scale n^-1 Ph_j^-1
  void *to = nullptr, *w = nullptr;  // build_tables(from = P, to = Q); its `from` entries are
                                     // not needed: Ph_j^-1 is in tab_inv's scale
  MdScr scr;
};

}  // namespace

struct nttmul_mdntt {
  KsPlan ks;                   // the bases and pinv, pw, Pinv (one digit of all of Q: unused)
  uint32_t scratch_mb = 512;
  int ndev = 0;
  std::vector<Plan> plan;      // per limb of Q u P (twiddle vectors released after upload)
  MdDev dev[kMaxDev];
  char err[kErrBytes] = {0};
};

namespace {

MdTables view(const nttmul_mdntt *h, const MdDev &d) {
  MdTables T;
  T.logn = h->ks.logn;
  T.L = h->ks.L;
  T.K = h->ks.K;
  T.word_bits = h->ks.word_bits;
  T.tab_fwd = d.tab[kRnsTransform];
  T.tab_inv = d.tab_inv;
  T.tw = d.tw;
  T.to = d.to;
  T.w = d.w;
  return T;
}

hipError_t fill_entry(const LaunchTables &T, int fam, void *dst) {
  return T.logn <= 12 ? rns_fill_entry(T, fam, dst) : rnsmp_fill_entry(T, fam, dst);
}

// The inverse's table for the K limbs of P: the standalone inverse's entry (kRnsInverse) with
// n^-1 Ph_j^-1 and iw[1] n^-1 Ph_j^-1 where it holds n^-1 and iw[1] n^-1, built with the
// planner's pair function in the forms make_plan gives fi and wfi.  iw[1] = psi^(-n / 2).
int upload_inv_table(nttmul_mdntt *h, MdDev &d) {
  const KsPlan &P = h->ks;
  const size_t ebytes = rns_entry_bytes(P.word_bits), tbytes = h->plan[0].fw.size();
  std::vector<uint8_t> host(ebytes * P.K);
  for (uint32_t j = 0; j < P.K; j++) {
    const Plan &pl = h->plan[P.L + j];
    const char *fw = (const char *)d.tw + 2 * tbytes * (P.L + j);
    LaunchTables T = limb_tables(pl, fw, fw + tbytes);
    const uint64_t f = mulmod(pl.inv_n, P.pinv[j], pl.q);
    const uint64_t iw1 = powmod(pl.inv_psi, pl.n / 2, pl.q);
    tw_pair(f, pl.q, pl.word_bits, &T.fi, &T.fis);
    tw_pair(mulmod(iw1, f, pl.q), pl.q, pl.word_bits, &T.wfi, &T.wfis, true);
    LIMB_TRY(h->err, fill_entry(T, kRnsInverse, host.data() + ebytes * j));
  }
  return upload(h->err, &d.tab_inv, host.data(), host.size());
}

int setup_device(nttmul_mdntt *h, MdDev &d) {
  const KsPlan &P = h->ks;
  if (h->plan[0].fw.size() != (size_t)P.n * 2 * (P.word_bits / 8)) {
    set_err(h->err, "planner twiddle table is not n pairs");
    return NTTMUL_EUNSUPPORTED;
  }
  if (const int st = upload_limb_tables(h->err, h->plan, P.word_bits, d.base, &d.tw, d.tab,
                                        fill_entry))
    return st;
  if (const int st = upload_inv_table(h, d)) return st;
  std::vector<uint8_t> from, to, w;
  build_tables(P.word_bits, P.p, P.pinv, P.q, P.Pinv, P.pw, &from, &to, &w);
  if (const int st = upload(h->err, &d.to, to.data(), to.size())) return st;
  return upload(h->err, &d.w, w.data(), w.size());
}

// Scratch buffer i of at least `need` bytes; its last use must have completed before the old one
// is freed (rnsmp.cpp ensure)
int ensure(nttmul_mdntt *h, MdScr &sc, int i, size_t need) {
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
int run(nttmul_mdntt *h, MdDev &d, void *out, const void *x_hat, size_t batch, hipStream_t s) {
  if (!batch) return NTTMUL_OK;
  const KsPlan &P = h->ks;
  const MdShape S =
      mdntt_shape((size_t)h->scratch_mb << 20, P.n, P.L, P.K, P.word_bits, batch);
  if (P.flags & NTTMUL_FLAG_VALIDATE) {
    if (const int st = check_range(h->err, d.base.flag, d.base.q, P.L + P.K, P.logn, P.word_bits,
                                   x_hat, batch * S.in_words, nullptr, 0,
                                   "input word >= its limb's modulus", s))
      return st;
  }
  MdScr &sc = d.scr;
  // a call's first use of the scratch on s: ordered after the last enqueued use, whatever stream
  // that was on
  if (!sc.ev) LIMB_TRY(h->err, hipEventCreateWithFlags(&sc.ev, hipEventDisableTiming));
  if (sc.used && sc.last != s) LIMB_TRY(h->err, hipStreamWaitEvent(s, sc.ev, 0));
  int st = ensure(h, sc, kMdY, S.chunk * S.y_bytes);
  if (!st && S.t_bytes) st = ensure(h, sc, kMdYLazy, S.chunk * S.y_bytes);
  if (!st && S.t_bytes) st = ensure(h, sc, kMdT, S.chunk * S.t_bytes);
  if (st) return st;
  const MdTables T = view(h, d);
  const size_t wb = (size_t)P.word_bits / 8;
  for (size_t k = 0; k < S.subs && !st; k++) {
    const MpSub u = mp_sub(batch, S.chunk, k);
    const hipError_t e = launch_mdntt(T, (char *)out + u.p * S.out_words * wb,
                                      (const char *)x_hat + u.p * S.in_words * wb, u.cnt, sc.buf, s);
    if (e != hipSuccess) st = fail(h->err, e, "sub-batch launch");
  }
  // also after a failure: what was enqueued still uses the scratch
  const hipError_t e = hipEventRecord(sc.ev, s);
  sc.used = true;
  sc.last = s;
  if (!st && e != hipSuccess) st = fail(h->err, e, "hipEventRecord(scratch)");
  return st;
}

}  // namespace

extern "C" {

int nttmul_mdntt_create(nttmul_mdntt **out, const nttmul_params *params, size_t size,
                        const uint64_t *q, uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs) {
  if (!out) return NTTMUL_EINVAL;
  *out = nullptr;
  BasisRequest B;
  if (const int st = mdntt_validate(params, size, q, q_limbs, p, p_limbs, &B)) return st;
  nttmul_mdntt *h = new (std::nothrow) nttmul_mdntt();
  if (!h) return NTTMUL_ENOMEM;
  // the same checks again with one digit of all of Q, for the plain constants pinv, pw, Pinv
  if (const int st = ks_validate(params, size, q, q_limbs, p, p_limbs, q_limbs, &h->ks)) {
    delete h;
    return st;
  }
  ks_constants(&h->ks);
  h->scratch_mb = B.prm.scratch_mb ? B.prm.scratch_mb : 512;
  const uint32_t M = q_limbs + p_limbs;
  h->plan.resize(M);
  for (uint32_t l = 0; l < M; l++) {
    const int st = make_plan(h->ks.n, h->ks.modulus(l), 0, &h->plan[l], false);
    if (st) {
      delete h;
      return st;
    }
  }
  DevRange R;
  if (const int st = select_devices(h->ks.prm, &R)) {
    delete h;
    return st;
  }
  DeviceGuard guard;
  for (int i = 0; i < R.ndev; i++) {
    MdDev &d = h->dev[i];
    d.base.id = R.id(i);
    h->ndev = i + 1;
    const int st = setup_device(h, d);
    if (st) {
      const int ret = create_failed("nttmul_mdntt", h->err, st);
      nttmul_mdntt_destroy(h);
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

void nttmul_mdntt_destroy(nttmul_mdntt *h) {
  if (!h) return;
  destroy_devices(h->dev, h->ndev, [](MdDev &d) {
    // the last enqueued use of the scratch, not the caller's streams
    if (d.scr.used) (void)hipEventSynchronize(d.scr.ev);
    free_each({d.scr.buf[0], d.scr.buf[1], d.scr.buf[2], d.tw, d.tab[0], d.tab[1], d.tab[2],
               d.tab_inv, d.to, d.w, d.base.q, d.base.flag});
    if (d.scr.ev) (void)hipEventDestroy(d.scr.ev);
  });
  delete h;
}

const char *nttmul_mdntt_last_error(const nttmul_mdntt *h) { return h ? h->err : ""; }

int nttmul_mdntt_get_info(const nttmul_mdntt *h, nttmul_mdntt_info *info) {
  if (!h || !info) return NTTMUL_EINVAL;
  info->n = h->ks.n;
  info->logn = h->ks.logn;
  info->q_limbs = h->ks.L;
  info->p_limbs = h->ks.K;
  info->word_bits = (uint32_t)h->ks.word_bits;
  info->ndev = h->ndev;
  info->scratch_mb = h->scratch_mb;
  return NTTMUL_OK;
}

int nttmul_mdntt_moddown_device(nttmul_mdntt *h, void *out, const void *x_hat, size_t batch,
                                int dev, void *stream) {
  if (const int st = mdntt_call_status(h != nullptr, out, x_hat, batch)) return st;
  return on_device(h->err, h->dev, h->ndev, dev, [&](MdDev &d) {
    return run(h, d, out, x_hat, batch, (hipStream_t)stream);
  });
}

int nttmul_mdntt_moddown(nttmul_mdntt *h, void *out, const void *x_hat, size_t batch) {
  if (const int st = mdntt_call_status(h != nullptr, out, x_hat, batch)) return st;
  if (!batch) return NTTMUL_OK;
  MdDev &d = h->dev[0];
  const size_t poly = ((size_t)batch << h->ks.logn) * (h->ks.word_bits / 8);
  const Staged ops[2] = {{nullptr, out, poly * h->ks.L},
                         {x_hat, nullptr, poly * (h->ks.L + h->ks.K)}};
  return staged_op(h->err, d.base, "mdntt", ops, 2, [&](void *const *buf) {
    return run(h, d, buf[0], buf[1], batch, d.base.stream);
  });
}

int nttmul_mdntt_kernel_name(const nttmul_mdntt *h, char *buf, size_t cap) {
  if (!h || (cap && !buf)) return NTTMUL_EINVAL;
  std::string name;
  if (describe_mdntt(view(h, h->dev[0]), &name) != hipSuccess) return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

}  // extern "C"
