// ks.cpp — host runtime behind include/nttmul_ks.h (lib/libnttmul_ks.so only): a context of the
// bases Q and P and a digit width for one degree 256 <= n <= 65536, and the one launch per call:
// k_ks_modup (ks.hip) for ModUp, and for ModDown the k_bconv<W,1> of bconv.hip through
// launch_bconv with tables built for from = P, to = Q.  The validation and the plain constants
// are in ks_plan.cpp (host only); the device tables are derived here from the same values, in
// bconv.hpp's formats.  A context keeps the tables, the moduli and the range check's flag per
// device: no scratch, no state between calls, no CPU fallback.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "ks.hpp"
#include "ks_plan.hpp"
#include "nttmul_ks.h"
#include "planner.hpp"
#include "rns.hpp"

using namespace nttmul;

namespace {

constexpr int kMaxDev = 16;
using u128 = unsigned __int128;

struct KsDev {
  int id = -1;
  hipStream_t stream = nullptr;  // the host forms' stream
  void *up_from = nullptr, *up_to = nullptr, *up_w = nullptr;  // ModUp: digits of Q -> Q u P
  void *dn_from = nullptr, *dn_to = nullptr, *dn_w = nullptr;  // ModDown: P -> Q
  uint64_t *q = nullptr;         // q_0 .. q_{L-1}, p_0 .. p_{K-1}
  int *flag = nullptr;           // range-check result
};

}  // namespace

struct nttmul_ks {
  KsPlan plan;
  int ndev = 0;
  KsDev dev[kMaxDev];
  char err[256] = {0};
};

namespace {

struct DeviceGuard {  // restores the caller's current device on scope exit
  int prev = -1;
  DeviceGuard() { (void)hipGetDevice(&prev); }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

std::mutex g_err_mu;

int fail(nttmul_ks *h, hipError_t e, const char *what) {
  std::lock_guard<std::mutex> l(g_err_mu);
  snprintf(h->err, sizeof(h->err), "%s: %s", what, hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? NTTMUL_ENOMEM : NTTMUL_EHIP;
}

void set_err(nttmul_ks *h, const char *msg) {
  std::lock_guard<std::mutex> l(g_err_mu);
  snprintf(h->err, sizeof(h->err), "%s", msg);
}

#define KS_TRY(h, expr)                              \
  do {                                               \
    hipError_t _e = (expr);                          \
    if (_e != hipSuccess) return fail(h, _e, #expr); \
  } while (0)

// (value, companion) pair the device multiplies by k with (bconv_dev.hpp mulc): the Plantard pair
// of Arith32P::pmul, BR = B q^-1 mod 2^64 with B = -k 2^64 mod q as (low, high) word, or Shoup
template <class W>
void mul_pair(uint64_t k, uint64_t q, W *v, W *vs) {
  if (sizeof(W) == 4) {
    uint64_t inv = q;  // q^-1 mod 2^64 (Newton on the 2-adic inverse)
    for (int i = 0; i < 6; i++) inv *= 2 - q * inv;
    const uint64_t r64 = (uint64_t)(((u128)1 << 64) % q);
    const uint64_t br = ((q - mulmod(k % q, r64, q)) % q) * inv;
    *v = (W)(br & 0xFFFFFFFFull);
    *vs = (W)(br >> 32);
  } else {
    *v = (W)k;
    *vs = (W)(((u128)k << 64) / q);
  }
}

// -q^-1 mod 2^64 (the low word serves 32-bit words)
uint64_t neg_inv(uint64_t q) {
  uint64_t inv = q;
  for (int i = 0; i < 6; i++) inv *= 2 - q * inv;
  return 0 - inv;
}

// The three device tables of a conversion (bconv.hpp), in host memory: `from` limbs b with the
// factors inv [|b|], `to` limbs c with the epilogue factors binv [|c|] and the weights w [|b|][|c|]
template <class W>
void build_tables(const std::vector<uint64_t> &b, const std::vector<uint64_t> &inv,
                  const std::vector<uint64_t> &c, const std::vector<uint64_t> &binv,
                  const std::vector<uint64_t> &w, std::vector<uint8_t> *from,
                  std::vector<uint8_t> *to, std::vector<uint8_t> *wt) {
  constexpr int bits = sizeof(W) * 8;
  const uint32_t L = (uint32_t)b.size(), K = (uint32_t)c.size(), kpad = bconv_pad(K);
  from->assign(sizeof(BconvFrom<W>) * L, 0);
  to->assign(sizeof(BconvTo<W>) * kpad, 0);
  wt->assign(sizeof(W) * L * kpad, 0);
  BconvFrom<W> *F = (BconvFrom<W> *)from->data();
  BconvTo<W> *C = (BconvTo<W> *)to->data();
  W *t = (W *)wt->data();
  for (uint32_t i = 0; i < L; i++) {
    F[i].b = (W)b[i];
    mul_pair<W>(inv[i], b[i], &F[i].v, &F[i].vs);
  }
  for (uint32_t j = 0; j < kpad; j++) {
    const uint32_t jj = j < K ? j : K - 1;  // the padding repeats the last limb (never stored)
    C[j].c = (W)c[jj];
    C[j].qinv_neg = (W)neg_inv(c[jj]);
    C[j].cr = (W)(((u128)1 << bits) % c[jj]);
    mul_pair<W>(binv[jj], c[jj], &C[j].v, &C[j].vs);
  }
  for (uint32_t i = 0; i < L; i++)
    for (uint32_t j = 0; j < K; j++)  // w R mod c_j; the padding stays 0
      t[(size_t)i * kpad + j] = (W)(((u128)w[(size_t)i * K + j] << bits) % c[j]);
}

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
  T.q = d.q;
  return T;
}

KsDev *find_dev(nttmul_ks *h, int dev) {
  for (int i = 0; i < h->ndev; i++)
    if (h->dev[i].id == dev) return &h->dev[i];
  return nullptr;
}

int upload(nttmul_ks *h, void **dst, const void *src, size_t bytes) {
  KS_TRY(h, hipMalloc(dst, bytes));
  KS_TRY(h, hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return NTTMUL_OK;
}

int setup_device(nttmul_ks *h, KsDev &d) {
  const KsPlan &P = h->plan;
  KS_TRY(h, hipSetDevice(d.id));
  KS_TRY(h, hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
  KS_TRY(h, hipMalloc((void **)&d.flag, sizeof(int)));
  std::vector<uint64_t> ext(P.q);
  ext.insert(ext.end(), P.p.begin(), P.p.end());
  // ModUp's `to` entries carry no epilogue factor: the pair of 1
  const std::vector<uint64_t> one(ext.size(), 1);
  std::vector<uint8_t> from, to, w;
  const auto build = [&](const std::vector<uint64_t> &b, const std::vector<uint64_t> &inv,
                         const std::vector<uint64_t> &c, const std::vector<uint64_t> &binv,
                         const std::vector<uint64_t> &wv) {
    if (P.word_bits == 32)
      build_tables<uint32_t>(b, inv, c, binv, wv, &from, &to, &w);
    else
      build_tables<uint64_t>(b, inv, c, binv, wv, &from, &to, &w);
  };
  build(P.q, P.inv, ext, one, P.w);
  if (const int st = upload(h, &d.up_from, from.data(), from.size())) return st;
  if (const int st = upload(h, &d.up_to, to.data(), to.size())) return st;
  if (const int st = upload(h, &d.up_w, w.data(), w.size())) return st;
  build(P.p, P.pinv, P.q, P.Pinv, P.pw);
  if (const int st = upload(h, &d.dn_from, from.data(), from.size())) return st;
  if (const int st = upload(h, &d.dn_to, to.data(), to.size())) return st;
  if (const int st = upload(h, &d.dn_w, w.data(), w.size())) return st;
  return upload(h, (void **)&d.q, ext.data(), sizeof(uint64_t) * ext.size());
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
    RnsTables R;
    R.logn = h->plan.logn;
    R.limbs = in_limbs(h, op);
    R.word_bits = h->plan.word_bits;
    R.q = d.q;
    KS_TRY(h, hipMemsetAsync(d.flag, 0, sizeof(int), s));
    KS_TRY(h, launch_rns_check(R, in, (batch * R.limbs) << h->plan.logn, d.flag, s));
    int bad = 0;
    KS_TRY(h, hipMemcpyAsync(&bad, d.flag, sizeof(int), hipMemcpyDeviceToHost, s));
    KS_TRY(h, hipStreamSynchronize(s));
    if (bad) {
      set_err(h, "input word >= its limb's modulus");
      return NTTMUL_ERANGE;
    }
  }
  if (op == kKsModdown)
    KS_TRY(h, launch_bconv(down_tables(h, d), kBconvModdown, out, in, batch, s));
  else
    KS_TRY(h, launch_ks_modup(up_tables(h, d), out, in, batch, s));
  return NTTMUL_OK;
}

int device_op(nttmul_ks *h, int op, void *out, const void *in, size_t batch, int dev,
              void *stream) {
  if (const int st = op_args(h, out, in, batch)) return st;
  KsDev *d = find_dev(h, dev);
  if (!d) return NTTMUL_ENODEV;
  DeviceGuard guard;
  KS_TRY(h, hipSetDevice(d->id));
  return run(h, *d, op, out, in, batch, (hipStream_t)stream);
}

// Host buffers: dev[0], device buffers owned by the call, the device path, copy back, synchronise
int host_op(nttmul_ks *h, int op, void *out, const void *in, size_t batch) {
  if (const int st = op_args(h, out, in, batch)) return st;
  if (!batch) return NTTMUL_OK;
  KsDev &d = h->dev[0];
  DeviceGuard guard;
  KS_TRY(h, hipSetDevice(d.id));
  const size_t wb = (size_t)h->plan.word_bits / 8, poly = (batch << h->plan.logn) * wb;
  const size_t bytes[2] = {poly * out_limbs(h, op), poly * in_limbs(h, op)};  // out, in
  void *buf[2] = {nullptr, nullptr};
  int st = NTTMUL_OK;
  const auto step = [&](hipError_t e, const char *what) {
    if (!st && e != hipSuccess) st = fail(h, e, what);
    return !st;
  };
  for (int i = 0; i < 2 && !st; i++) step(hipMalloc(&buf[i], bytes[i]), "ks host buffers");
  if (!st) step(hipMemcpyAsync(buf[1], in, bytes[1], hipMemcpyHostToDevice, d.stream), "ks copy in");
  if (!st) st = run(h, d, op, buf[0], buf[1], batch, d.stream);
  if (!st) step(hipMemcpyAsync(out, buf[0], bytes[0], hipMemcpyDeviceToHost, d.stream), "ks copy out");
  // (also after a failure: nothing of this call may still run when its buffers go)
  step(hipStreamSynchronize(d.stream), "ks synchronise");
  for (void *p : buf)
    if (p) (void)hipFree(p);
  return st;
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
  nttmul_params prm;
  memset(&prm, 0, sizeof(prm));
  memcpy(&prm, params, size);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    delete h;
    return NTTMUL_ENODEV;
  }
  const int first = prm.first_dev < 0 ? 0 : prm.first_dev;
  const int ndev = prm.ndev <= 0 ? count - first : prm.ndev;
  const bool share = (prm.flags & NTTMUL_FLAG_SHARE_DEVICES) != 0;
  if (first >= count || ndev <= 0 || (!share && first + ndev > count) || ndev > kMaxDev) {
    delete h;
    return NTTMUL_ENODEV;
  }
  DeviceGuard guard;
  for (int i = 0; i < ndev; i++) {
    KsDev &d = h->dev[i];
    d.id = first + i % (count - first);
    h->ndev = i + 1;
    const int st = setup_device(h, d);
    if (st) {
      fprintf(stderr, "nttmul_ks: %s\n", h->err);
      nttmul_ks_destroy(h);
      return st == NTTMUL_EHIP ? NTTMUL_ENODEV : st;
    }
  }
  *out = h;
  return NTTMUL_OK;
}

void nttmul_ks_destroy(nttmul_ks *h) {
  if (!h) return;
  DeviceGuard guard;
  for (int i = 0; i < h->ndev; i++) {
    KsDev &d = h->dev[i];
    if (d.id < 0) continue;
    (void)hipSetDevice(d.id);
    if (d.stream) (void)hipStreamSynchronize(d.stream);
    for (void *p : {d.up_from, d.up_to, d.up_w, d.dn_from, d.dn_to, d.dn_w, (void *)d.q,
                    (void *)d.flag})
      if (p) (void)hipFree(p);
    if (d.stream) (void)hipStreamDestroy(d.stream);
  }
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
  if (cap) {
    const size_t k = name.size() < cap - 1 ? name.size() : cap - 1;
    memcpy(buf, name.data(), k);
    buf[k] = 0;
  }
  return (int)name.size();
}

}  // extern "C"
