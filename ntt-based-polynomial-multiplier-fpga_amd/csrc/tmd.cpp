// tmd.cpp — host runtime behind include/nttmul_tmd.h (lib/libnttmul_tmd.so only): a context of
// the bases Q and P and a plaintext modulus t for one degree 256 <= n <= 65536, and the two or
// four launches per sub-batch of tmd.hip.  The create-time checks and the plain constants are
// tmd_plan.hpp's (basis.cpp's checks through mdntt_plan.hpp), the context runtime limb_ctx.cpp's,
// the limbs' plans and their upload planner.cpp's and rns.cpp's (upload_limb_tables over the
// extended basis Q u P), the conversion tables' device form bconv.hpp's build_tables.  This file
// keeps its handle and what only it has: the inverse's table with Ph_j^-1 folded into its scale,
// the weight table with the correction's two rows, the plaintext modulus' entry and g, the
// scratch (as mdntt.cpp's: grown on demand, handed between streams by an event) and the sub-batch
// loop of run.  No CPU fallback.
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "limb_ctx.hpp"
#include "nttmul_tmd.h"
#include "planner.hpp"
#include "tmd.hpp"
#include "tmd_plan.hpp"

using namespace nttmul;

namespace {

struct TmScr {
  void *buf[kMdScratch] = {nullptr, nullptr, nullptr};
  size_t bytes[kMdScratch] = {0, 0, 0};
  hipEvent_t ev = nullptr;     // recorded after the last enqueued use
  bool used = false;
  hipStream_t last = nullptr;  // stream of that use
};

struct TmDev {
  LimbDev base;                // q: q_0 .. q_{L-1}, p_0 .. p_{K-1}
  void *tw = nullptr;          // fw, iw of limb 0, fw, iw of limb 1, ... over Q u P
  void *tab[kRnsFamilies] = {nullptr, nullptr, nullptr};  // over Q u P (upload_limb_tables)
  void *tab_inv = nullptr;     // P's limbs, the scale n^-1 Ph_j^-1
  void *to = nullptr;          // build_tables(to = Q) with P^-1 as the entries' factor
  void *w = nullptr;           // K + 2 rows
  void *tt = nullptr, *g = nullptr;  // build_tables(to = {t}): t's entry and g_j R mod t
  TmScr scr;
};

}  // namespace

struct nttmul_tmd {
  TmPlan tm;
  uint32_t scratch_mb = 512;
  int ndev = 0;
  std::vector<Plan> plan;      // per limb of Q u P (twiddle vectors released after upload)
  TmDev dev[kMaxDev];
  char err[kErrBytes] = {0};
};

namespace {

TmTables view(const nttmul_tmd *h, const TmDev &d) {
  TmTables T;
  T.logn = h->tm.logn;
  T.L = h->tm.L;
  T.K = h->tm.K;
  T.word_bits = h->tm.word_bits;
  T.tab_fwd = d.tab[kRnsTransform];
  T.tab_inv = d.tab_inv;
  T.tw = d.tw;
  T.to = d.to;
  T.w = d.w;
  T.tt = d.tt;
  T.g = d.g;
  return T;
}

hipError_t fill_entry(const LaunchTables &T, int fam, void *dst) {
  return T.logn <= 12 ? rns_fill_entry(T, fam, dst) : rnsmp_fill_entry(T, fam, dst);
}

// The inverse's table for the K limbs of P: mdntt.cpp upload_inv_table's
int upload_inv_table(nttmul_tmd *h, TmDev &d) {
  const TmPlan &P = h->tm;
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

int setup_device(nttmul_tmd *h, TmDev &d) {
  const TmPlan &P = h->tm;
  if (h->plan[0].fw.size() != (size_t)P.n * 2 * (P.word_bits / 8)) {
    set_err(h->err, "planner twiddle table is not n pairs");
    return NTTMUL_EUNSUPPORTED;
  }
  if (const int st = upload_limb_tables(h->err, h->plan, P.word_bits, d.base, &d.tw, d.tab,
                                        fill_entry))
    return st;
  if (const int st = upload_inv_table(h, d)) return st;
  // K + 2 `from` rows: the limbs of P and the correction's two.  The `from` entries themselves
  // are not needed (Ph_j^-1 is in tab_inv's scale); the last two only have to be well formed
  std::vector<uint64_t> b(P.p), binv(P.yscale);
  b.insert(b.end(), 2, P.p[0]);
  binv.insert(binv.end(), 2, 1);
  std::vector<uint8_t> from, to, w;
  build_tables(P.word_bits, b, binv, P.q, P.v, P.w, &from, &to, &w);
  if (const int st = upload(h->err, &d.to, to.data(), to.size())) return st;
  if (const int st = upload(h->err, &d.w, w.data(), w.size())) return st;
  // the plaintext modulus as a one-limb target basis: its entry's factor is not read
  build_tables(P.word_bits, P.p, P.yscale, {P.t}, {1}, P.g, &from, &to, &w);
  if (const int st = upload(h->err, &d.tt, to.data(), to.size())) return st;
  return upload(h->err, &d.g, w.data(), w.size());
}

// Scratch buffer i of at least `need` bytes; its last use must have completed before the old one
// is freed (mdntt.cpp ensure)
int ensure(nttmul_tmd *h, TmScr &sc, int i, size_t need) {
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
int run(nttmul_tmd *h, TmDev &d, void *out, const void *x_hat, size_t batch, hipStream_t s) {
  if (!batch) return NTTMUL_OK;
  const TmPlan &P = h->tm;
  const MdShape S = tmd_shape((size_t)h->scratch_mb << 20, P.n, P.L, P.K, P.word_bits, batch);
  if (P.flags & NTTMUL_FLAG_VALIDATE) {
    if (const int st = check_range(h->err, d.base.flag, d.base.q, P.L + P.K, P.logn, P.word_bits,
                                   x_hat, batch * S.in_words, nullptr, 0,
                                   "input word >= its limb's modulus", s))
      return st;
  }
  TmScr &sc = d.scr;
  // a call's first use of the scratch on s: ordered after the last enqueued use, whatever stream
  // that was on
  if (!sc.ev) LIMB_TRY(h->err, hipEventCreateWithFlags(&sc.ev, hipEventDisableTiming));
  if (sc.used && sc.last != s) LIMB_TRY(h->err, hipStreamWaitEvent(s, sc.ev, 0));
  int st = ensure(h, sc, kMdY, S.chunk * S.y_bytes);
  if (!st && S.t_bytes) st = ensure(h, sc, kMdYLazy, S.chunk * S.y_bytes);
  if (!st && S.t_bytes) st = ensure(h, sc, kMdT, S.chunk * S.t_bytes);
  if (st) return st;
  const TmTables T = view(h, d);
  const size_t wb = (size_t)P.word_bits / 8;
  for (size_t k = 0; k < S.subs && !st; k++) {
    const MpSub u = mp_sub(batch, S.chunk, k);
    const hipError_t e = launch_tmd(T, (char *)out + u.p * S.out_words * wb,
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

int nttmul_tmd_create(nttmul_tmd **out, const nttmul_params *params, size_t size,
                      const uint64_t *q, uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs,
                      uint64_t t) {
  if (!out) return NTTMUL_EINVAL;
  *out = nullptr;
  nttmul_tmd *h = new (std::nothrow) nttmul_tmd();
  if (!h) return NTTMUL_ENOMEM;
  if (const int st = tmd_validate(params, size, q, q_limbs, p, p_limbs, t, &h->tm)) {
    delete h;
    return st;
  }
  tmd_constants(&h->tm);
  h->scratch_mb = h->tm.prm.scratch_mb ? h->tm.prm.scratch_mb : 512;
  const uint32_t M = q_limbs + p_limbs;
  h->plan.resize(M);
  for (uint32_t l = 0; l < M; l++) {
    const int st = make_plan(h->tm.n, h->tm.modulus(l), 0, &h->plan[l], false);
    if (st) {
      delete h;
      return st;
    }
  }
  DevRange R;
  if (const int st = select_devices(h->tm.prm, &R)) {
    delete h;
    return st;
  }
  DeviceGuard guard;
  for (int i = 0; i < R.ndev; i++) {
    TmDev &d = h->dev[i];
    d.base.id = R.id(i);
    h->ndev = i + 1;
    const int st = setup_device(h, d);
    if (st) {
      const int ret = create_failed("nttmul_tmd", h->err, st);
      nttmul_tmd_destroy(h);
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

void nttmul_tmd_destroy(nttmul_tmd *h) {
  if (!h) return;
  destroy_devices(h->dev, h->ndev, [](TmDev &d) {
    // the last enqueued use of the scratch, not the caller's streams
    if (d.scr.used) (void)hipEventSynchronize(d.scr.ev);
    free_each({d.scr.buf[0], d.scr.buf[1], d.scr.buf[2], d.tw, d.tab[0], d.tab[1], d.tab[2],
               d.tab_inv, d.to, d.w, d.tt, d.g, d.base.q, d.base.flag});
    if (d.scr.ev) (void)hipEventDestroy(d.scr.ev);
  });
  delete h;
}

const char *nttmul_tmd_last_error(const nttmul_tmd *h) { return h ? h->err : ""; }

int nttmul_tmd_get_info(const nttmul_tmd *h, nttmul_tmd_info *info) {
  if (!h || !info) return NTTMUL_EINVAL;
  info->n = h->tm.n;
  info->logn = h->tm.logn;
  info->q_limbs = h->tm.L;
  info->p_limbs = h->tm.K;
  info->word_bits = (uint32_t)h->tm.word_bits;
  info->ndev = h->ndev;
  info->scratch_mb = h->scratch_mb;
  info->t = h->tm.t;
  info->msg_factor = h->tm.msg_factor;
  return NTTMUL_OK;
}

int nttmul_tmd_moddown_device(nttmul_tmd *h, void *out, const void *x_hat, size_t batch, int dev,
                              void *stream) {
  if (const int st = tmd_call_status(h != nullptr, out, x_hat, batch)) return st;
  return on_device(h->err, h->dev, h->ndev, dev, [&](TmDev &d) {
    return run(h, d, out, x_hat, batch, (hipStream_t)stream);
  });
}

int nttmul_tmd_moddown(nttmul_tmd *h, void *out, const void *x_hat, size_t batch) {
  if (const int st = tmd_call_status(h != nullptr, out, x_hat, batch)) return st;
  if (!batch) return NTTMUL_OK;
  TmDev &d = h->dev[0];
  const size_t poly = ((size_t)batch << h->tm.logn) * (h->tm.word_bits / 8);
  const Staged ops[2] = {{nullptr, out, poly * h->tm.L},
                         {x_hat, nullptr, poly * (h->tm.L + h->tm.K)}};
  return staged_op(h->err, d.base, "tmd", ops, 2, [&](void *const *buf) {
    return run(h, d, buf[0], buf[1], batch, d.base.stream);
  });
}

int nttmul_tmd_plan(const nttmul_params *params, size_t size, const uint64_t *q, uint32_t q_limbs,
                    const uint64_t *p, uint32_t p_limbs, uint64_t t, uint64_t *yscale,
                    uint64_t *g, uint64_t *w, uint64_t *v, uint64_t *msg_factor) {
  TmPlan P;
  if (const int st = tmd_validate(params, size, q, q_limbs, p, p_limbs, t, &P)) return st;
  tmd_constants(&P);
  const auto copy = [](uint64_t *dst, const std::vector<uint64_t> &src) {
    if (dst) memcpy(dst, src.data(), sizeof(uint64_t) * src.size());
  };
  copy(yscale, P.yscale);
  copy(g, P.g);
  copy(w, P.w);
  copy(v, P.v);
  if (msg_factor) *msg_factor = P.msg_factor;
  return NTTMUL_OK;
}

int nttmul_tmd_kernel_name(const nttmul_tmd *h, char *buf, size_t cap) {
  if (!h || (cap && !buf)) return NTTMUL_EINVAL;
  std::string name;
  if (describe_tmd(view(h, h->dev[0]), &name) != hipSuccess) return NTTMUL_EUNSUPPORTED;
  return copy_name(name, buf, cap);
}

}  // extern "C"
