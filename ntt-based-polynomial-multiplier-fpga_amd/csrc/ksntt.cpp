// ksntt.cpp — host runtime behind include/nttmul_ksntt.h (lib/libnttmul_ksntt.so only): a context
// of the bases Q and P and a digit width for one degree 256 <= n <= 65536, the two or four
// launches per sub-batch of modup and the one launch of mac (ksntt.hip).  The create-time checks
// and the plain constants are ks_plan.cpp's (through ksntt_plan.hpp), the context runtime
// limb_ctx.cpp's, the limbs' plans and their upload planner.cpp's and rns.cpp's
// (upload_limb_tables over the extended basis Q u P), the conversion tables' device form
// bconv.hpp's build_tables.  This file keeps its handle and what only it has: the inverse's table
// with Dh_i^-1 folded into its scale, the scratch (as mdntt.cpp's: grown on demand, handed between
// streams by an event) and the sub-batch loop of modup.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "ksntt.hpp"
#include "ksntt_plan.hpp"
#include "limb_ctx.hpp"
#include "nttmul_ksntt.h"
#include "planner.hpp"

using namespace nttmul;

namespace {

struct KnScr {
  void *buf[kMdScratch] = {nullptr, nullptr, nullptr};
  size_t bytes[kMdScratch] = {0, 0, 0};
  hipEvent_t ev = nullptr;     // recorded after the last enqueued use
  bool used = false;
  hipStream_t last = nullptr;  // stream of that use
};

struct KnDev {
  LimbDev base;                // q: q_0 .. q_{L-1}, p_0 .. p_{K-1}
  void *tw = nullptr;          // fw, iw of limb 0, fw, iw of limb 1, ... over Q u P
  void *tab[kRnsFamilies] = {nullptr, nullptr, nullptr};  // over Q u P (upload_limb_tables)
  void *tab_inv = nullptr;     // Q's limbs, the scale n^-1 Dh_i^-1
  void *to = nullptr, *w = nullptr;  // build_tables(from = Q, to = Q u P) with R mod m as the
                                     // `to` entries' factor; its `from` entries are not needed:
                                     // Dh_i^-1 is in tab_inv's scale
  KnScr scr;
};

}  // namespace

struct nttmul_ksntt {
  KsPlan ks;
  uint32_t scratch_mb = 512;
  int ndev = 0;
  std::vector<Plan> plan;      // per limb of Q u P (twiddle vectors released after upload)
  KnDev dev[kMaxDev];
  char err[kErrBytes] = {0};
};

namespace {

KsnttTables view(const nttmul_ksntt *h, const KnDev &d) {
  KsnttTables T;
  T.logn = h->ks.logn;
  T.L = h->ks.L;
  T.K = h->ks.K;
  T.alpha = h->ks.alpha;
  T.dnum = h->ks.dnum;
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

// The inverse's table for the L limbs of Q: the standalone inverse's entry (kRnsInverse) with
// n^-1 Dh_i^-1 and iw[1] n^-1 Dh_i^-1 where it holds n^-1 and iw[1] n^-1 (mdntt.cpp
// upload_inv_table, which folds Ph_j^-1 the same way)
int upload_inv_table(nttmul_ksntt *h, KnDev &d) {
  const KsPlan &P = h->ks;
  const size_t ebytes = rns_entry_bytes(P.word_bits), tbytes = h->plan[0].fw.size();
  std::vector<uint8_t> host(ebytes * P.L);
  for (uint32_t i = 0; i < P.L; i++) {
    const Plan &pl = h->plan[i];
    const char *fw = (const char *)d.tw + 2 * tbytes * i;
    LaunchTables T = limb_tables(pl, fw, fw + tbytes);
    const uint64_t f = mulmod(pl.inv_n, P.inv[i], pl.q);
    const uint64_t iw1 = powmod(pl.inv_psi, pl.n / 2, pl.q);
    tw_pair(f, pl.q, pl.word_bits, &T.fi, &T.fis);
    tw_pair(mulmod(iw1, f, pl.q), pl.q, pl.word_bits, &T.wfi, &T.wfis, true);
    LIMB_TRY(h->err, fill_entry(T, kRnsInverse, host.data() + ebytes * i));
  }
  return upload(h->err, &d.tab_inv, host.data(), host.size());
}

int setup_device(nttmul_ksntt *h, KnDev &d) {
  const KsPlan &P = h->ks;
  if (h->plan[0].fw.size() != (size_t)P.n * 2 * (P.word_bits / 8)) {
    set_err(h->err, "planner twiddle table is not n pairs");
    return NTTMUL_EUNSUPPORTED;
  }
  if (const int st = upload_limb_tables(h->err, h->plan, P.word_bits, d.base, &d.tw, d.tab,
                                        fill_entry))
    return st;
  if (const int st = upload_inv_table(h, d)) return st;
  std::vector<uint64_t> ext(P.q);
  ext.insert(ext.end(), P.p.begin(), P.p.end());
  // the `to` entries' factor: R mod m, what mac multiplies its Montgomery-scaled sum by
  std::vector<uint64_t> rmod(ext.size());
  for (size_t m = 0; m < ext.size(); m++)
    rmod[m] = (uint64_t)(((unsigned __int128)1 << P.word_bits) % ext[m]);
  std::vector<uint8_t> from, to, w;
  build_tables(P.word_bits, P.q, P.inv, ext, rmod, P.w, &from, &to, &w);
  if (const int st = upload(h->err, &d.to, to.data(), to.size())) return st;
  return upload(h->err, &d.w, w.data(), w.size());
}

// Scratch buffer i of at least `need` bytes; its last use must have completed before the old one
// is freed (mdntt.cpp ensure)
int ensure(nttmul_ksntt *h, KnScr &sc, int i, size_t need) {
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
int run_modup(nttmul_ksntt *h, KnDev &d, void *up, const void *x_hat, size_t batch,
              hipStream_t s) {
  if (!batch) return NTTMUL_OK;
  const KsPlan &P = h->ks;
  const KsnttShape S = ksntt_shape((size_t)h->scratch_mb << 20, P.n, P.L, P.K, P.alpha,
                                   P.word_bits, batch);
  if (P.flags & NTTMUL_FLAG_VALIDATE) {
    if (const int st = check_range(h->err, d.base.flag, d.base.q, P.L, P.logn, P.word_bits, x_hat,
                                   batch * S.in_words, nullptr, 0,
                                   "input word >= its limb's modulus", s))
      return st;
  }
  KnScr &sc = d.scr;
  // a call's first use of the scratch on s: ordered after the last enqueued use, whatever stream
  // that was on
  if (!sc.ev) LIMB_TRY(h->err, hipEventCreateWithFlags(&sc.ev, hipEventDisableTiming));
  if (sc.used && sc.last != s) LIMB_TRY(h->err, hipStreamWaitEvent(s, sc.ev, 0));
  int st = ensure(h, sc, kMdY, S.chunk * S.y_bytes);
  if (!st && P.n > 4096) st = ensure(h, sc, kMdYLazy, S.chunk * S.y_bytes);
  if (st) return st;
  const KsnttTables T = view(h, d);
  const size_t wb = (size_t)P.word_bits / 8;
  for (size_t k = 0; k < S.subs && !st; k++) {
    const MpSub u = mp_sub(batch, S.chunk, k);
    const hipError_t e =
        launch_ksntt_modup(T, (char *)up + u.p * S.out_words * wb,
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

// on d, stream s: the range check of both operands over the L + K limbs, then the one launch.
// V: b_hat is viewed (ksntt.hpp KsnttViewed), its check and the launch are V's
int run_mac(nttmul_ksntt *h, KnDev &d, void *c, const void *a, const void *b, const HoistArgs &H,
            size_t batch, uint32_t terms, hipStream_t s, const KsnttViewed *V = nullptr) {
  if (!batch) return NTTMUL_OK;
  const KsPlan &P = h->ks;
  if (P.flags & NTTMUL_FLAG_VALIDATE) {
    const char *msg = "operand word >= its limb's modulus";
    size_t words[3];
    ksntt_mac_words(P.L + P.K, P.n, batch, terms, H.rots, H.comps, words);
    if (const int st = check_range(h->err, d.base.flag, d.base.q, P.L + P.K, P.logn, P.word_bits,
                                   a, words[1], b, V ? 0 : words[2], msg, s))
      return st;
    if (V)
      if (const int st = V->check(h->err, d.base.flag, d.base.q, P.word_bits, b, *V->addr,
                                  (size_t)H.rots * H.comps, terms, true, msg, s))
        return st;
  }
  const hipError_t e = V ? V->launch(view(h, d), c, a, b, H, batch, terms, *V->addr, s)
                         : launch_ksntt_mac(view(h, d), c, a, b, H, batch, terms, s);
  return e == hipSuccess ? NTTMUL_OK : fail(h->err, e, "mac launch");
}

int mac_call(nttmul_ksntt *h, void *c, const void *a, const void *b, const uint32_t *k,
             uint32_t rots, size_t batch, uint32_t terms, uint32_t comps, HoistArgs *H) {
  H->rots = rots;
  H->comps = comps;
  return ksntt_mac_status(h != nullptr, h ? h->ks.n : 0, c, a, b, k, rots, batch, terms, comps,
                          H->ks.k);
}

// nttmul_ksntt_mac_device; V: b_hat viewed
int mac_device(nttmul_ksntt *h, void *c_hat, const void *a_hat, const void *b_hat,
               const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms, uint32_t comps,
               int dev, void *stream, const KsnttViewed *V) {
  HoistArgs H;
  if (const int st = mac_call(h, c_hat, a_hat, b_hat, k, rots, batch, terms, comps, &H)) return st;
  return on_device(h->err, h->dev, h->ndev, dev, [&](KnDev &d) {
    return run_mac(h, d, c_hat, a_hat, b_hat, H, batch, terms, (hipStream_t)stream, V);
  });
}

// nttmul_ksntt_mac; V: b_hat viewed, staged whole
int mac_host(nttmul_ksntt *h, void *c_hat, const void *a_hat, const void *b_hat, const uint32_t *k,
             uint32_t rots, size_t batch, uint32_t terms, uint32_t comps, const KsnttViewed *V) {
  HoistArgs H;
  if (const int st = mac_call(h, c_hat, a_hat, b_hat, k, rots, batch, terms, comps, &H)) return st;
  if (!batch) return NTTMUL_OK;
  KnDev &d = h->dev[0];
  size_t words[3];
  ksntt_mac_words(h->ks.L + h->ks.K, h->ks.n, batch, terms, rots, comps, words);
  const size_t wb = (size_t)h->ks.word_bits / 8;
  const Staged ops[3] = {{nullptr, c_hat, words[0] * wb},
                         {a_hat, nullptr, words[1] * wb},
                         {b_hat, nullptr, (V ? V->b_words : words[2]) * wb}};
  return staged_op(h->err, d.base, "ksntt", ops, 3, [&](void *const *buf) {
    return run_mac(h, d, buf[0], buf[1], buf[2], H, batch, terms, d.base.stream, V);
  });
}

}  // namespace

namespace nttmul {

int ksntt_mac_viewed(nttmul_ksntt *h, const KsnttViewed &V, void *c_hat, const void *a_hat,
                     const void *b_hat, const uint32_t *k, uint32_t rots, size_t batch,
                     uint32_t terms, uint32_t comps, int host, int dev, void *stream) {
  if (host) return mac_host(h, c_hat, a_hat, b_hat, k, rots, batch, terms, comps, &V);
  return mac_device(h, c_hat, a_hat, b_hat, k, rots, batch, terms, comps, dev, stream, &V);
}

}  // namespace nttmul

extern "C" {

int nttmul_ksntt_create(nttmul_ksntt **out, const nttmul_params *params, size_t size,
                        const uint64_t *q, uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs,
                        uint32_t digit_limbs) {
  if (!out) return NTTMUL_EINVAL;
  *out = nullptr;
  nttmul_ksntt *h = new (std::nothrow) nttmul_ksntt();
  if (!h) return NTTMUL_ENOMEM;
  if (const int st = ksntt_validate(params, size, q, q_limbs, p, p_limbs, digit_limbs, &h->ks)) {
    delete h;
    return st;
  }
  ks_constants(&h->ks);
  h->scratch_mb = h->ks.prm.scratch_mb ? h->ks.prm.scratch_mb : 512;
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
    KnDev &d = h->dev[i];
    d.base.id = R.id(i);
    h->ndev = i + 1;
    const int st = setup_device(h, d);
    if (st) {
      const int ret = create_failed("nttmul_ksntt", h->err, st);
      nttmul_ksntt_destroy(h);
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

void nttmul_ksntt_destroy(nttmul_ksntt *h) {
  if (!h) return;
  destroy_devices(h->dev, h->ndev, [](KnDev &d) {
    // the last enqueued use of the scratch, not the caller's streams
    if (d.scr.used) (void)hipEventSynchronize(d.scr.ev);
    free_each({d.scr.buf[0], d.scr.buf[1], d.scr.buf[2], d.tw, d.tab[0], d.tab[1], d.tab[2],
               d.tab_inv, d.to, d.w, d.base.q, d.base.flag});
    if (d.scr.ev) (void)hipEventDestroy(d.scr.ev);
  });
  delete h;
}

const char *nttmul_ksntt_last_error(const nttmul_ksntt *h) { return h ? h->err : ""; }

int nttmul_ksntt_get_info(const nttmul_ksntt *h, nttmul_ksntt_info *info) {
  if (!h || !info) return NTTMUL_EINVAL;
  info->n = h->ks.n;
  info->logn = h->ks.logn;
  info->q_limbs = h->ks.L;
  info->p_limbs = h->ks.K;
  info->digit_limbs = h->ks.alpha;
  info->digits = h->ks.dnum;
  info->word_bits = (uint32_t)h->ks.word_bits;
  info->ndev = h->ndev;
  info->scratch_mb = h->scratch_mb;
  return NTTMUL_OK;
}

int nttmul_ksntt_modup_device(nttmul_ksntt *h, void *up_hat, const void *x_hat, size_t batch,
                              int dev, void *stream) {
  if (const int st = ksntt_modup_status(h != nullptr, up_hat, x_hat, batch)) return st;
  return on_device(h->err, h->dev, h->ndev, dev, [&](KnDev &d) {
    return run_modup(h, d, up_hat, x_hat, batch, (hipStream_t)stream);
  });
}

int nttmul_ksntt_modup(nttmul_ksntt *h, void *up_hat, const void *x_hat, size_t batch) {
  if (const int st = ksntt_modup_status(h != nullptr, up_hat, x_hat, batch)) return st;
  if (!batch) return NTTMUL_OK;
  KnDev &d = h->dev[0];
  const size_t poly = ((size_t)batch << h->ks.logn) * (h->ks.word_bits / 8);
  const Staged ops[2] = {{nullptr, up_hat, poly * h->ks.dnum * (h->ks.L + h->ks.K)},
                         {x_hat, nullptr, poly * h->ks.L}};
  return staged_op(h->err, d.base, "ksntt", ops, 2, [&](void *const *buf) {
    return run_modup(h, d, buf[0], buf[1], batch, d.base.stream);
  });
}

int nttmul_ksntt_mac_device(nttmul_ksntt *h, void *c_hat, const void *a_hat, const void *b_hat,
                            const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                            uint32_t comps, int dev, void *stream) {
  return mac_device(h, c_hat, a_hat, b_hat, k, rots, batch, terms, comps, dev, stream, nullptr);
}

int nttmul_ksntt_mac(nttmul_ksntt *h, void *c_hat, const void *a_hat, const void *b_hat,
                     const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                     uint32_t comps) {
  return mac_host(h, c_hat, a_hat, b_hat, k, rots, batch, terms, comps, nullptr);
}

int nttmul_ksntt_kernel_name(const nttmul_ksntt *h, int op, uint32_t comps, char *buf,
                             size_t cap) {
  if (!h || op < NTTMUL_KSNTT_MODUP || op > NTTMUL_KSNTT_MAC || (cap && !buf))
    return NTTMUL_EINVAL;
  if (op == NTTMUL_KSNTT_MAC && (!comps || comps > NTTMUL_MACN_MAX_COMPS)) return NTTMUL_EINVAL;
  std::string name;
  if (describe_ksntt(view(h, h->dev[0]), op, comps, &name) != hipSuccess)
    return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

}  // extern "C"
