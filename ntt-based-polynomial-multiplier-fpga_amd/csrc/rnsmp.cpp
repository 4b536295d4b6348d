// rnsmp.cpp — host runtime behind include/nttmul_rnsmp.h (lib/libnttmul_rnsmp.so only): a context
// of several moduli for one degree 4096 < n <= 65536, and the two or three launches per operation
// over [batch][limbs][n] operands (rnsmp.hip).  It plans each limb with the planner of the plain
// contexts (planner.hpp) and keeps, per device, the limbs' twiddle tables in one allocation, one
// table of kernel constants per kernel family (rns.hpp) and one scratch for the intermediates of
// the passes.  No resident server, no issue-priority rule, no CPU fallback.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "nttmul_rnsmp.h"
#include "planner.hpp"
#include "rnsmp.hpp"

using namespace nttmul;

namespace {

constexpr int kMaxDev = 16;

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
  int id = -1;
  hipStream_t stream = nullptr;               // the host forms' stream
  void *tw = nullptr;                         // fw, iw of limb 0, fw, iw of limb 1, ...
  void *tab[kRnsFamilies] = {nullptr, nullptr, nullptr};
  uint64_t *q = nullptr;
  int *flag = nullptr;                        // range-check result
  MpScratch scr;
};

}  // namespace

struct nttmul_rnsmp {
  uint32_t n = 0, logn = 0, limbs = 0, flags = 0, scratch_mb = 512;
  int word_bits = 0, ndev = 0;
  std::vector<Plan> plan;                     // per limb (twiddle vectors released after upload)
  MpDev dev[kMaxDev];
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

int fail(nttmul_rnsmp *r, hipError_t e, const char *what) {
  std::lock_guard<std::mutex> l(g_err_mu);
  snprintf(r->err, sizeof(r->err), "%s: %s", what, hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? NTTMUL_ENOMEM : NTTMUL_EHIP;
}

void set_err(nttmul_rnsmp *r, const char *msg) {
  std::lock_guard<std::mutex> l(g_err_mu);
  snprintf(r->err, sizeof(r->err), "%s", msg);
}

#define MP_TRY(r, expr)                              \
  do {                                               \
    hipError_t _e = (expr);                          \
    if (_e != hipSuccess) return fail(r, _e, #expr); \
  } while (0)

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

RnsTables tables_for(const nttmul_rnsmp *r, const MpDev &d) {
  RnsTables T;
  T.logn = r->logn;
  T.limbs = r->limbs;
  T.word_bits = r->word_bits;
  for (int f = 0; f < kRnsFamilies; f++) T.tab[f] = d.tab[f];
  T.tw = d.tw;
  T.q = d.q;
  return T;
}

MpDev *find_dev(nttmul_rnsmp *r, int dev) {
  for (int i = 0; i < r->ndev; i++)
    if (r->dev[i].id == dev) return &r->dev[i];
  return nullptr;
}

// One device's tables: the limbs' twiddles in one allocation (n pairs each of fw, iw per limb),
// then the three KParams tables.  The kernels form the twiddle pointers from the allocation's
// base; the entries' own fw / iw hold the same addresses.
int setup_device(nttmul_rnsmp *r, MpDev &d) {
  const size_t tbytes = r->plan[0].fw.size(), ebytes = rns_entry_bytes(r->word_bits);
  const uint32_t L = r->limbs;
  if (tbytes != (size_t)r->n * 2 * (r->word_bits / 8)) {
    set_err(r, "planner twiddle table is not n pairs");
    return NTTMUL_EUNSUPPORTED;
  }
  MP_TRY(r, hipSetDevice(d.id));
  MP_TRY(r, hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
  MP_TRY(r, hipMalloc(&d.tw, 2 * tbytes * L));
  MP_TRY(r, hipMalloc((void **)&d.q, sizeof(uint64_t) * L));
  MP_TRY(r, hipMalloc((void **)&d.flag, sizeof(int)));
  std::vector<uint64_t> q(L);
  std::vector<uint8_t> host(ebytes * L);
  for (uint32_t l = 0; l < L; l++) {
    char *fw = (char *)d.tw + 2 * tbytes * l;
    MP_TRY(r, hipMemcpy(fw, r->plan[l].fw.data(), tbytes, hipMemcpyHostToDevice));
    MP_TRY(r, hipMemcpy(fw + tbytes, r->plan[l].iw.data(), tbytes, hipMemcpyHostToDevice));
    q[l] = r->plan[l].q;
  }
  MP_TRY(r, hipMemcpy(d.q, q.data(), sizeof(uint64_t) * L, hipMemcpyHostToDevice));
  for (int f = 0; f < kRnsFamilies; f++) {
    for (uint32_t l = 0; l < L; l++) {
      const char *fw = (const char *)d.tw + 2 * tbytes * l;
      MP_TRY(r, rnsmp_fill_entry(limb_tables(r->plan[l], fw, fw + tbytes), f,
                                 host.data() + ebytes * l));
    }
    MP_TRY(r, hipMalloc(&d.tab[f], ebytes * L));
    MP_TRY(r, hipMemcpy(d.tab[f], host.data(), ebytes * L, hipMemcpyHostToDevice));
  }
  return NTTMUL_OK;
}

// what is decided before any device access
int op_args(const nttmul_rnsmp *r, int op, const void *c, const void *a, const void *b,
            size_t batch, uint32_t terms) {
  if (!r || (op == kRnsMac && !terms)) return NTTMUL_EINVAL;
  const bool two = op == kRnsMultiply || op == kRnsMac;
  if (batch && (!c || !a || (two && !b))) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

// words of the operands of one call: c, a, b (b 0 for the transforms)
void op_words(const nttmul_rnsmp *r, int op, size_t batch, uint32_t terms, int shared,
              size_t words[3]) {
  const size_t poly = (size_t)r->limbs * r->n;
  words[0] = batch * poly;
  words[1] = op == kRnsMac ? batch * terms * poly : batch * poly;
  words[2] = op == kRnsMac ? (shared ? 1 : batch) * terms * poly
                           : op == kRnsMultiply ? batch * poly : 0;
}

// Scratch buffer i of at least `need` bytes; its last use must have completed before the old one
// is freed
int ensure(nttmul_rnsmp *r, MpScratch &sc, int i, size_t need) {
  if (sc.bytes[i] >= need) return NTTMUL_OK;
  if (sc.used) MP_TRY(r, hipEventSynchronize(sc.ev));
  if (sc.buf[i]) (void)hipFree(sc.buf[i]);
  sc.buf[i] = nullptr;
  sc.bytes[i] = 0;
  MP_TRY(r, hipMalloc(&sc.buf[i], need));
  sc.bytes[i] = need;
  return NTTMUL_OK;
}

// on d (the current device), stream s: the range check, then sub-batches of whole polynomials
// through the scratch
int run(nttmul_rnsmp *r, MpDev &d, int op, void *c, const void *a, const void *b, size_t batch,
        uint32_t terms, int shared, hipStream_t s) {
  if (!batch) return NTTMUL_OK;
  const RnsTables T = tables_for(r, d);
  if (r->flags & NTTMUL_FLAG_VALIDATE) {
    size_t words[3];
    op_words(r, op, batch, terms, shared, words);
    MP_TRY(r, hipMemsetAsync(d.flag, 0, sizeof(int), s));
    MP_TRY(r, launch_rns_check(T, a, words[1], d.flag, s));
    if (words[2]) MP_TRY(r, launch_rns_check(T, b, words[2], d.flag, s));
    int bad = 0;
    MP_TRY(r, hipMemcpyAsync(&bad, d.flag, sizeof(int), hipMemcpyDeviceToHost, s));
    MP_TRY(r, hipStreamSynchronize(s));
    if (bad) {
      set_err(r, "input coefficient >= its limb's modulus");
      return NTTMUL_ERANGE;
    }
  }
  // bytes of one polynomial (all limbs) in a scratch buffer, and of one polynomial's a: for the
  // mac all its terms, so that no scratch buffer of a sub-batch exceeds scratch_mb
  const size_t poly = (size_t)r->limbs * r->n * (r->word_bits / 8);
  const size_t apoly = op == kRnsMac ? poly * terms : poly;
  const size_t chunk =
      std::max<size_t>(1, std::min(batch, ((size_t)r->scratch_mb << 20) / apoly));
  MpScratch &sc = d.scr;
  if (!sc.ev) MP_TRY(r, hipEventCreateWithFlags(&sc.ev, hipEventDisableTiming));
  if (sc.used && sc.last != s) MP_TRY(r, hipStreamWaitEvent(s, sc.ev, 0));
  const bool two = op == kRnsMultiply, three = op == kRnsMultiply || op == kRnsMac;
  int st = ensure(r, sc, 0, chunk * apoly);
  if (!st && two) st = ensure(r, sc, 1, chunk * poly);
  if (!st && three) st = ensure(r, sc, 2, chunk * poly);
  if (st) return st;
  const size_t bstep = op == kRnsMac ? (shared ? 0 : apoly) : poly;
  for (size_t p = 0; p < batch && !st; p += chunk) {
    const size_t cnt = std::min(chunk, batch - p);
    const hipError_t e =
        launch_rnsmp(T, op, (char *)c + p * poly, (const char *)a + p * apoly,
                     b ? (const char *)b + p * bstep : nullptr, cnt, terms, shared, sc.buf, s);
    if (e != hipSuccess) st = fail(r, e, "sub-batch launch");
  }
  // (also after a failure: what was enqueued still uses the scratch)
  const hipError_t e = hipEventRecord(sc.ev, s);
  sc.used = true;
  sc.last = s;
  if (!st && e != hipSuccess) st = fail(r, e, "hipEventRecord(scratch)");
  return st;
}

int device_op(nttmul_rnsmp *r, int op, void *c, const void *a, const void *b, size_t batch,
              uint32_t terms, int shared, int dev, void *stream) {
  if (const int st = op_args(r, op, c, a, b, batch, terms)) return st;
  MpDev *d = find_dev(r, dev);
  if (!d) return NTTMUL_ENODEV;
  DeviceGuard guard;
  MP_TRY(r, hipSetDevice(d->id));
  return run(r, *d, op, c, a, b, batch, terms, shared, (hipStream_t)stream);
}

// Host buffers: dev[0], device buffers owned by the call, the device path, copy back, synchronise
int host_op(nttmul_rnsmp *r, int op, void *c, const void *a, const void *b, size_t batch,
            uint32_t terms, int shared) {
  if (const int st = op_args(r, op, c, a, b, batch, terms)) return st;
  if (!batch) return NTTMUL_OK;
  MpDev &d = r->dev[0];
  DeviceGuard guard;
  MP_TRY(r, hipSetDevice(d.id));
  size_t words[3];
  op_words(r, op, batch, terms, shared, words);
  const size_t wb = (size_t)r->word_bits / 8;
  const void *src[3] = {nullptr, a, b};
  void *buf[3] = {nullptr, nullptr, nullptr};  // c, a, b
  int st = NTTMUL_OK;
  const auto step = [&](hipError_t e, const char *what) {
    if (!st && e != hipSuccess) st = fail(r, e, what);
    return !st;
  };
  for (int i = 0; i < 3 && !st; i++)
    if (words[i]) step(hipMalloc(&buf[i], words[i] * wb), "rnsmp host buffers");
  for (int i = 1; i < 3 && !st; i++)
    if (words[i])
      step(hipMemcpyAsync(buf[i], src[i], words[i] * wb, hipMemcpyHostToDevice, d.stream),
           "rnsmp copy in");
  if (!st) st = run(r, d, op, buf[0], buf[1], buf[2], batch, terms, shared, d.stream);
  if (!st)
    step(hipMemcpyAsync(c, buf[0], words[0] * wb, hipMemcpyDeviceToHost, d.stream),
         "rnsmp copy out");
  // (also after a failure: nothing of this call may still run when its buffers go)
  step(hipStreamSynchronize(d.stream), "rnsmp synchronise");
  for (void *p : buf)
    if (p) (void)hipFree(p);
  return st;
}

}  // namespace

extern "C" {

int nttmul_rnsmp_create(nttmul_rnsmp **out, const nttmul_params *caller, size_t size,
                        const uint64_t *q, uint32_t limbs) {
  if (!out) return NTTMUL_EINVAL;
  *out = nullptr;
  if (!caller || size < NTTMUL_PARAMS_BASE_SIZE || size > sizeof(nttmul_params))
    return NTTMUL_EINVAL;
  nttmul_params p;
  memset(&p, 0, sizeof(p));
  memcpy(&p, caller, size);
  if (!q || limbs == 0 || limbs > NTTMUL_RNS_MAX_LIMBS || p.q || p.psi) return NTTMUL_EINVAL;
  // a degree: a power of two from 256 up (above 65536 it is valid and unsupported, below)
  const uint32_t n = p.n;
  if (n < 256 || n > (1u << 30) || (n & (n - 1))) return NTTMUL_EINVAL;
  for (uint32_t l = 0; l < limbs; l++) {
    if (q[l] < 3 || q[l] >= (1ull << 62) || (q[l] - 1) % (2ull * n) || !is_prime(q[l]))
      return NTTMUL_EINVAL;
    for (uint32_t m = 0; m < l; m++)
      if (q[m] == q[l]) return NTTMUL_EINVAL;
  }
  // n <= 4096 is nttmul_rns_*'s (include/nttmul_rns.h, lib/libnttmul_rns.so)
  if (n <= 4096 || n > 65536 || (p.flags & NTTMUL_FLAG_CYCLIC)) return NTTMUL_EUNSUPPORTED;
  // one word class per context: every q_l < 2^31 (32-bit words) or every q_l >= 2^32 (64-bit)
  const bool small = q[0] < (1ull << 31);
  for (uint32_t l = 0; l < limbs; l++) {
    if (q[l] >= (1ull << 31) && q[l] < (1ull << 32)) return NTTMUL_EUNSUPPORTED;
    if ((q[l] < (1ull << 31)) != small) return NTTMUL_EUNSUPPORTED;
  }
  nttmul_rnsmp *r = new (std::nothrow) nttmul_rnsmp();
  if (!r) return NTTMUL_ENOMEM;
  r->n = n;
  r->limbs = limbs;
  r->flags = p.flags;
  r->scratch_mb = p.scratch_mb ? p.scratch_mb : 512;
  r->word_bits = small ? 32 : 64;
  r->plan.resize(limbs);
  for (uint32_t l = 0; l < limbs; l++) {
    const int st = make_plan(n, q[l], 0, &r->plan[l], false);
    if (st) {
      delete r;
      return st;
    }
  }
  r->logn = r->plan[0].logn;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    delete r;
    return NTTMUL_ENODEV;
  }
  const int first = p.first_dev < 0 ? 0 : p.first_dev;
  const int ndev = p.ndev <= 0 ? count - first : p.ndev;
  const bool share = (p.flags & NTTMUL_FLAG_SHARE_DEVICES) != 0;
  if (first >= count || ndev <= 0 || (!share && first + ndev > count) || ndev > kMaxDev) {
    delete r;
    return NTTMUL_ENODEV;
  }
  DeviceGuard guard;
  for (int i = 0; i < ndev; i++) {
    MpDev &d = r->dev[i];
    d.id = first + i % (count - first);
    r->ndev = i + 1;
    const int st = setup_device(r, d);
    if (st) {
      fprintf(stderr, "nttmul_rnsmp: %s\n", r->err);
      nttmul_rnsmp_destroy(r);
      return st == NTTMUL_EHIP ? NTTMUL_ENODEV : st;
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
  DeviceGuard guard;
  for (int i = 0; i < r->ndev; i++) {
    MpDev &d = r->dev[i];
    if (d.id < 0) continue;
    (void)hipSetDevice(d.id);
    if (d.stream) (void)hipStreamSynchronize(d.stream);
    // the last enqueued use of the scratch, not the caller's streams
    if (d.scr.used) (void)hipEventSynchronize(d.scr.ev);
    for (void *p : {d.scr.buf[0], d.scr.buf[1], d.scr.buf[2], d.tw, d.tab[0], d.tab[1], d.tab[2],
                    (void *)d.q, (void *)d.flag})
      if (p) (void)hipFree(p);
    if (d.scr.ev) (void)hipEventDestroy(d.scr.ev);
    if (d.stream) (void)hipStreamDestroy(d.stream);
  }
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
  const Plan &P = r->plan[limb];
  info->n = P.n;
  info->logn = P.logn;
  info->q = P.q;
  info->psi = P.psi;
  info->omega = P.omega;
  info->inv_psi = P.inv_psi;
  info->inv_omega = P.inv_omega;
  info->inv_n = P.inv_n;
  info->word_bits = (uint32_t)P.word_bits;
  info->ndev = r->ndev;
  info->kernel = 1;
  info->cyclic = 0;
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
  if (describe_rnsmp(tables_for(r, r->dev[0]), op, &name) != hipSuccess)
    return NTTMUL_EUNSUPPORTED;
  if (cap) {
    const size_t k = name.size() < cap - 1 ? name.size() : cap - 1;
    memcpy(buf, name.data(), k);
    buf[k] = 0;
  }
  return (int)name.size();
}

}  // extern "C"
