// bconv.cpp — host runtime behind include/nttmul_bconv.h (lib/libnttmul_bconv.so only): a
// converter between two disjoint RNS bases of one word class for one degree n <= 4096, and one
// launch per conversion over [batch][limbs][n] operands (bconv.hip).  The constants come from the
// planner's modular arithmetic (planner.hpp mulmod / powmod) in 128-bit host integers;
// nttmul_bconv_plan returns them plain, create derives its device tables from the same values.
// No resident server, no CPU fallback.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "bconv.hpp"
#include "nttmul_bconv.h"
#include "planner.hpp"
#include "rns.hpp"

using namespace nttmul;

namespace {

constexpr int kMaxDev = 16;
using u128 = unsigned __int128;

struct BconvDev {
  int id = -1;
  hipStream_t stream = nullptr;               // the host forms' stream
  void *from = nullptr, *to = nullptr, *w = nullptr;
  uint64_t *q = nullptr;                      // c_0 .. c_{K-1}, b_0 .. b_{L-1}
  int *flag = nullptr;                        // range-check result
};

// The plain constants of a converter (nttmul_bconv_plan)
struct BconvPlan {
  uint32_t n = 0, logn = 0, L = 0, K = 0, flags = 0;
  int word_bits = 0;
  std::vector<uint64_t> b, c, inv, w, binv;   // w: [L][K]
};

}  // namespace

struct nttmul_bconv {
  BconvPlan plan;
  int ndev = 0;
  BconvDev dev[kMaxDev];
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

int fail(nttmul_bconv *h, hipError_t e, const char *what) {
  std::lock_guard<std::mutex> l(g_err_mu);
  snprintf(h->err, sizeof(h->err), "%s: %s", what, hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? NTTMUL_ENOMEM : NTTMUL_EHIP;
}

void set_err(nttmul_bconv *h, const char *msg) {
  std::lock_guard<std::mutex> l(g_err_mu);
  snprintf(h->err, sizeof(h->err), "%s", msg);
}

#define BCONV_TRY(h, expr)                           \
  do {                                               \
    hipError_t _e = (expr);                          \
    if (_e != hipSuccess) return fail(h, _e, #expr); \
  } while (0)

// What create and plan decide before any device access, in nttmul_rns_create's order: every
// EINVAL of either basis first, then the unsupported shapes, then the word classes
int validate(const nttmul_params *caller, size_t size, const uint64_t *from_q, uint32_t L,
             const uint64_t *to_q, uint32_t K, BconvPlan *P) {
  if (!caller || size < NTTMUL_PARAMS_BASE_SIZE || size > sizeof(nttmul_params))
    return NTTMUL_EINVAL;
  nttmul_params p;
  memset(&p, 0, sizeof(p));
  memcpy(&p, caller, size);
  if (!from_q || !to_q || L == 0 || L > NTTMUL_RNS_MAX_LIMBS || K == 0 ||
      K > NTTMUL_RNS_MAX_LIMBS || p.q || p.psi)
    return NTTMUL_EINVAL;
  const uint32_t n = p.n;
  if (n < 256 || n > 65536 || (n & (n - 1))) return NTTMUL_EINVAL;
  std::vector<uint64_t> all(from_q, from_q + L);
  all.insert(all.end(), to_q, to_q + K);
  for (size_t l = 0; l < all.size(); l++) {
    const uint64_t q = all[l];
    if (q < 3 || q >= (1ull << 62) || (q - 1) % (2ull * n) || !is_prime(q)) return NTTMUL_EINVAL;
    for (size_t m = 0; m < l; m++)
      if (all[m] == q) return NTTMUL_EINVAL;
  }
  if (n > 4096 || (p.flags & NTTMUL_FLAG_CYCLIC)) return NTTMUL_EUNSUPPORTED;
  const bool small = all[0] < (1ull << 31);
  for (const uint64_t q : all) {
    if (q >= (1ull << 31) && q < (1ull << 32)) return NTTMUL_EUNSUPPORTED;
    if ((q < (1ull << 31)) != small) return NTTMUL_EUNSUPPORTED;
    // (what nttmul_rns_create asks of a 32-bit basis at n = 4096)
    if (small && n == 4096 && !p3_fold_ok(q)) return NTTMUL_EUNSUPPORTED;
  }
  P->n = n;
  P->logn = (uint32_t)__builtin_ctz(n);
  P->L = L;
  P->K = K;
  P->flags = p.flags;
  P->word_bits = small ? 32 : 64;
  P->b.assign(from_q, from_q + L);
  P->c.assign(to_q, to_q + K);
  return NTTMUL_OK;
}

uint64_t invmod(uint64_t a, uint64_t q) { return powmod(a % q, q - 2, q); }  // q prime

// inv[i] = Bh_i^-1 mod b_i, w[i][j] = Bh_i mod c_j, binv[j] = B^-1 mod c_j
void plan_constants(BconvPlan *P) {
  const uint32_t L = P->L, K = P->K;
  P->inv.resize(L);
  P->w.resize((size_t)L * K);
  P->binv.resize(K);
  for (uint32_t i = 0; i < L; i++) {
    uint64_t h = 1;
    for (uint32_t m = 0; m < L; m++)
      if (m != i) h = mulmod(h, P->b[m] % P->b[i], P->b[i]);
    P->inv[i] = invmod(h, P->b[i]);
    for (uint32_t j = 0; j < K; j++) {
      uint64_t v = 1;
      for (uint32_t m = 0; m < L; m++)
        if (m != i) v = mulmod(v, P->b[m] % P->c[j], P->c[j]);
      P->w[(size_t)i * K + j] = v;
    }
  }
  for (uint32_t j = 0; j < K; j++) {
    uint64_t v = 1;
    for (uint32_t m = 0; m < L; m++) v = mulmod(v, P->b[m] % P->c[j], P->c[j]);
    P->binv[j] = invmod(v, P->c[j]);
  }
}

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

// The three device tables of bconv.hpp BconvTables, in host memory
template <class W>
void build_tables(const BconvPlan &P, std::vector<uint8_t> *from, std::vector<uint8_t> *to,
                  std::vector<uint8_t> *w) {
  constexpr int bits = sizeof(W) * 8;
  const uint32_t L = P.L, K = P.K, kpad = bconv_pad(K);
  from->assign(sizeof(BconvFrom<W>) * L, 0);
  to->assign(sizeof(BconvTo<W>) * kpad, 0);
  w->assign(sizeof(W) * L * kpad, 0);
  BconvFrom<W> *F = (BconvFrom<W> *)from->data();
  BconvTo<W> *C = (BconvTo<W> *)to->data();
  W *wt = (W *)w->data();
  for (uint32_t i = 0; i < L; i++) {
    F[i].b = (W)P.b[i];
    mul_pair<W>(P.inv[i], P.b[i], &F[i].v, &F[i].vs);
  }
  for (uint32_t j = 0; j < kpad; j++) {
    const uint32_t jj = j < K ? j : K - 1;  // the padding repeats the last limb (never stored)
    const uint64_t c = P.c[jj];
    C[j].c = (W)c;
    C[j].qinv_neg = (W)neg_inv(c);
    C[j].cr = (W)(((u128)1 << bits) % c);
    mul_pair<W>(P.binv[jj], c, &C[j].v, &C[j].vs);
  }
  for (uint32_t i = 0; i < L; i++)
    for (uint32_t j = 0; j < K; j++)  // Bh_i R mod c_j; the padding stays 0
      wt[(size_t)i * kpad + j] = (W)(((u128)P.w[(size_t)i * K + j] << bits) % P.c[j]);
}

BconvTables tables_for(const nttmul_bconv *h, const BconvDev &d) {
  BconvTables T;
  T.logn = h->plan.logn;
  T.from_limbs = h->plan.L;
  T.to_limbs = h->plan.K;
  T.word_bits = h->plan.word_bits;
  T.from = d.from;
  T.to = d.to;
  T.w = d.w;
  T.q = d.q;
  return T;
}

BconvDev *find_dev(nttmul_bconv *h, int dev) {
  for (int i = 0; i < h->ndev; i++)
    if (h->dev[i].id == dev) return &h->dev[i];
  return nullptr;
}

int upload(nttmul_bconv *h, void **dst, const void *src, size_t bytes) {
  BCONV_TRY(h, hipMalloc(dst, bytes));
  BCONV_TRY(h, hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return NTTMUL_OK;
}

int setup_device(nttmul_bconv *h, BconvDev &d) {
  const BconvPlan &P = h->plan;
  BCONV_TRY(h, hipSetDevice(d.id));
  BCONV_TRY(h, hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
  BCONV_TRY(h, hipMalloc((void **)&d.flag, sizeof(int)));
  std::vector<uint8_t> from, to, w;
  if (P.word_bits == 32)
    build_tables<uint32_t>(P, &from, &to, &w);
  else
    build_tables<uint64_t>(P, &from, &to, &w);
  std::vector<uint64_t> q(P.c);
  q.insert(q.end(), P.b.begin(), P.b.end());
  if (const int st = upload(h, &d.from, from.data(), from.size())) return st;
  if (const int st = upload(h, &d.to, to.data(), to.size())) return st;
  if (const int st = upload(h, &d.w, w.data(), w.size())) return st;
  return upload(h, (void **)&d.q, q.data(), sizeof(uint64_t) * q.size());
}

// what is decided before any device access
int op_args(const nttmul_bconv *h, const void *out, const void *in, size_t batch) {
  if (!h) return NTTMUL_EINVAL;
  if (batch && (!out || !in)) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

uint32_t in_limbs(const nttmul_bconv *h, int op) {
  return op == kBconvModdown ? h->plan.K + h->plan.L : h->plan.L;
}

// on d (the current device), stream s
int run(nttmul_bconv *h, BconvDev &d, int op, void *out, const void *in, size_t batch,
        hipStream_t s) {
  if (!batch) return NTTMUL_OK;
  const BconvTables T = tables_for(h, d);
  if (h->plan.flags & NTTMUL_FLAG_VALIDATE) {
    // k_rns_check_range over the input's own limbs: all K + L of moddown's, the last L of the
    // moduli list for convert's
    RnsTables R;
    R.logn = T.logn;
    R.limbs = in_limbs(h, op);
    R.word_bits = T.word_bits;
    R.q = op == kBconvModdown ? d.q : d.q + h->plan.K;
    BCONV_TRY(h, hipMemsetAsync(d.flag, 0, sizeof(int), s));
    BCONV_TRY(h, launch_rns_check(R, in, batch * R.limbs * h->plan.n, d.flag, s));
    int bad = 0;
    BCONV_TRY(h, hipMemcpyAsync(&bad, d.flag, sizeof(int), hipMemcpyDeviceToHost, s));
    BCONV_TRY(h, hipStreamSynchronize(s));
    if (bad) {
      set_err(h, "input coefficient >= its limb's modulus");
      return NTTMUL_ERANGE;
    }
  }
  BCONV_TRY(h, launch_bconv(T, op, out, in, batch, s));
  return NTTMUL_OK;
}

int device_op(nttmul_bconv *h, int op, void *out, const void *in, size_t batch, int dev,
              void *stream) {
  if (const int st = op_args(h, out, in, batch)) return st;
  BconvDev *d = find_dev(h, dev);
  if (!d) return NTTMUL_ENODEV;
  DeviceGuard guard;
  BCONV_TRY(h, hipSetDevice(d->id));
  return run(h, *d, op, out, in, batch, (hipStream_t)stream);
}

// Host buffers: dev[0], device buffers owned by the call, the device path, copy back, synchronise
int host_op(nttmul_bconv *h, int op, void *out, const void *in, size_t batch) {
  if (const int st = op_args(h, out, in, batch)) return st;
  if (!batch) return NTTMUL_OK;
  BconvDev &d = h->dev[0];
  DeviceGuard guard;
  BCONV_TRY(h, hipSetDevice(d.id));
  const size_t wb = (size_t)h->plan.word_bits / 8, poly = (size_t)h->plan.n * wb * batch;
  const size_t bytes[2] = {poly * h->plan.K, poly * in_limbs(h, op)};  // out, in
  void *buf[2] = {nullptr, nullptr};
  int st = NTTMUL_OK;
  const auto step = [&](hipError_t e, const char *what) {
    if (!st && e != hipSuccess) st = fail(h, e, what);
    return !st;
  };
  for (int i = 0; i < 2 && !st; i++) step(hipMalloc(&buf[i], bytes[i]), "bconv host buffers");
  if (!st) step(hipMemcpyAsync(buf[1], in, bytes[1], hipMemcpyHostToDevice, d.stream), "bconv copy in");
  if (!st) st = run(h, d, op, buf[0], buf[1], batch, d.stream);
  if (!st) step(hipMemcpyAsync(out, buf[0], bytes[0], hipMemcpyDeviceToHost, d.stream), "bconv copy out");
  // (also after a failure: nothing of this call may still run when its buffers go)
  step(hipStreamSynchronize(d.stream), "bconv synchronise");
  for (void *p : buf)
    if (p) (void)hipFree(p);
  return st;
}

}  // namespace

extern "C" {

int nttmul_bconv_plan(const nttmul_params *params, size_t size, const uint64_t *from_q,
                      uint32_t from_limbs, const uint64_t *to_q, uint32_t to_limbs, uint64_t *inv,
                      uint64_t *w, uint64_t *binv) {
  if (!inv || !w || !binv) return NTTMUL_EINVAL;
  BconvPlan P;
  if (const int st = validate(params, size, from_q, from_limbs, to_q, to_limbs, &P)) return st;
  plan_constants(&P);
  memcpy(inv, P.inv.data(), sizeof(uint64_t) * P.inv.size());
  memcpy(w, P.w.data(), sizeof(uint64_t) * P.w.size());
  memcpy(binv, P.binv.data(), sizeof(uint64_t) * P.binv.size());
  return NTTMUL_OK;
}

int nttmul_bconv_create(nttmul_bconv **out, const nttmul_params *params, size_t size,
                        const uint64_t *from_q, uint32_t from_limbs, const uint64_t *to_q,
                        uint32_t to_limbs) {
  if (!out) return NTTMUL_EINVAL;
  *out = nullptr;
  nttmul_bconv *h = new (std::nothrow) nttmul_bconv();
  if (!h) return NTTMUL_ENOMEM;
  if (const int st = validate(params, size, from_q, from_limbs, to_q, to_limbs, &h->plan)) {
    delete h;
    return st;
  }
  plan_constants(&h->plan);
  nttmul_params p;
  memset(&p, 0, sizeof(p));
  memcpy(&p, params, size);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    delete h;
    return NTTMUL_ENODEV;
  }
  const int first = p.first_dev < 0 ? 0 : p.first_dev;
  const int ndev = p.ndev <= 0 ? count - first : p.ndev;
  const bool share = (p.flags & NTTMUL_FLAG_SHARE_DEVICES) != 0;
  if (first >= count || ndev <= 0 || (!share && first + ndev > count) || ndev > kMaxDev) {
    delete h;
    return NTTMUL_ENODEV;
  }
  DeviceGuard guard;
  for (int i = 0; i < ndev; i++) {
    BconvDev &d = h->dev[i];
    d.id = first + i % (count - first);
    h->ndev = i + 1;
    const int st = setup_device(h, d);
    if (st) {
      fprintf(stderr, "nttmul_bconv: %s\n", h->err);
      nttmul_bconv_destroy(h);
      return st == NTTMUL_EHIP ? NTTMUL_ENODEV : st;
    }
  }
  *out = h;
  return NTTMUL_OK;
}

void nttmul_bconv_destroy(nttmul_bconv *h) {
  if (!h) return;
  DeviceGuard guard;
  for (int i = 0; i < h->ndev; i++) {
    BconvDev &d = h->dev[i];
    if (d.id < 0) continue;
    (void)hipSetDevice(d.id);
    if (d.stream) (void)hipStreamSynchronize(d.stream);
    for (void *p : {d.from, d.to, d.w, (void *)d.q, (void *)d.flag})
      if (p) (void)hipFree(p);
    if (d.stream) (void)hipStreamDestroy(d.stream);
  }
  delete h;
}

const char *nttmul_bconv_last_error(const nttmul_bconv *h) { return h ? h->err : ""; }

int nttmul_bconv_get_info(const nttmul_bconv *h, nttmul_bconv_info *info) {
  if (!h || !info) return NTTMUL_EINVAL;
  info->n = h->plan.n;
  info->from_limbs = h->plan.L;
  info->to_limbs = h->plan.K;
  info->word_bits = (uint32_t)h->plan.word_bits;
  info->ndev = h->ndev;
  return NTTMUL_OK;
}

int nttmul_bconv_convert_device(nttmul_bconv *h, void *out, const void *in, size_t batch, int dev,
                                void *stream) {
  return device_op(h, kBconvConvert, out, in, batch, dev, stream);
}
int nttmul_bconv_moddown_device(nttmul_bconv *h, void *out, const void *x, size_t batch, int dev,
                                void *stream) {
  return device_op(h, kBconvModdown, out, x, batch, dev, stream);
}

int nttmul_bconv_convert(nttmul_bconv *h, void *out, const void *in, size_t batch) {
  return host_op(h, kBconvConvert, out, in, batch);
}
int nttmul_bconv_moddown(nttmul_bconv *h, void *out, const void *x, size_t batch) {
  return host_op(h, kBconvModdown, out, x, batch);
}

int nttmul_bconv_kernel_name(const nttmul_bconv *h, int op, char *buf, size_t cap) {
  if (!h || op < kBconvConvert || op > kBconvModdown || (cap && !buf)) return NTTMUL_EINVAL;
  std::string name;
  if (describe_bconv(tables_for(h, h->dev[0]), op, &name) != hipSuccess) return NTTMUL_EUNSUPPORTED;
  if (cap) {
    const size_t k = name.size() < cap - 1 ? name.size() : cap - 1;
    memcpy(buf, name.data(), k);
    buf[k] = 0;
  }
  return (int)name.size();
}

}  // extern "C"
