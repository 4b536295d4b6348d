// galois.cpp — host runtime behind include/nttmul_galois.h (lib/libnttmul_galois.so only): a context
// of several moduli for one degree 256 <= n <= 65536, and the one launch per call over
// [batch][limbs][n] operands (galois.hip).  A context keeps, per device, the moduli and the range
// check's flag: the kernels read no twiddles and no index table.  No scratch, no CPU fallback.
// The host-only entry points (nttmul_galois_element, nttmul_galois_plan) and the index arithmetic
// are in galois_plan.cpp.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "galois.hpp"
#include "nttmul_galois.h"
#include "planner.hpp"

using namespace nttmul;

namespace {

constexpr int kMaxDev = 16;

struct GDev {
  int id = -1;
  hipStream_t stream = nullptr;  // the host forms' stream
  uint64_t *q = nullptr;
  int *flag = nullptr;           // range-check result
};

}  // namespace

struct nttmul_galois {
  uint32_t n = 0, logn = 0, limbs = 0, flags = 0;
  int word_bits = 0, ndev = 0;
  std::vector<Plan> plan;  // per limb, for nttmul_galois_limb_info (twiddle vectors released)
  GDev dev[kMaxDev];
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

int fail(nttmul_galois *g, hipError_t e, const char *what) {
  std::lock_guard<std::mutex> l(g_err_mu);
  snprintf(g->err, sizeof(g->err), "%s: %s", what, hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? NTTMUL_ENOMEM : NTTMUL_EHIP;
}

void set_err(nttmul_galois *g, const char *msg) {
  std::lock_guard<std::mutex> l(g_err_mu);
  snprintf(g->err, sizeof(g->err), "%s", msg);
}

#define G_TRY(g, expr)                               \
  do {                                               \
    hipError_t _e = (expr);                          \
    if (_e != hipSuccess) return fail(g, _e, #expr); \
  } while (0)

GaloisTables tables_for(const nttmul_galois *g, const GDev &d) {
  GaloisTables T;
  T.logn = g->logn;
  T.limbs = g->limbs;
  T.word_bits = g->word_bits;
  T.q = d.q;
  return T;
}

GDev *find_dev(nttmul_galois *g, int dev) {
  for (int i = 0; i < g->ndev; i++)
    if (g->dev[i].id == dev) return &g->dev[i];
  return nullptr;
}

int setup_device(nttmul_galois *g, GDev &d) {
  const uint32_t L = g->limbs;
  G_TRY(g, hipSetDevice(d.id));
  G_TRY(g, hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
  G_TRY(g, hipMalloc((void **)&d.q, sizeof(uint64_t) * L));
  G_TRY(g, hipMalloc((void **)&d.flag, sizeof(int)));
  std::vector<uint64_t> q(L);
  for (uint32_t l = 0; l < L; l++) q[l] = g->plan[l].q;
  G_TRY(g, hipMemcpy(d.q, q.data(), sizeof(uint64_t) * L, hipMemcpyHostToDevice));
  return NTTMUL_OK;
}

// What is decided before any device access.  On success kv holds the automorphisms as the kernels
// take them (galois.hpp launch_galois).
int op_args(const nttmul_galois *g, int op, const void *out, const void *in, const uint32_t *k,
            uint32_t count, size_t batch, GaloisKs *kv) {
  if (!g || !k || count == 0 || count > kGaloisMaxCount) return NTTMUL_EINVAL;
  for (uint32_t c = 0; c < count; c++) {
    if (!galois_k_ok(g->n, k[c])) return NTTMUL_EINVAL;
    kv->k[c] = op == kGaloisNtt ? k[c] : galois_inv_mod_2n(g->n, k[c]);
  }
  for (uint32_t c = count; c < kGaloisMaxCount; c++) kv->k[c] = 1;
  if (batch && (!out || !in)) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

// on d (the current device), stream s: the range check, then the launch
int run(nttmul_galois *g, GDev &d, int op, void *out, const void *in, const GaloisKs &kv,
        uint32_t count, size_t batch, hipStream_t s) {
  if (!batch) return NTTMUL_OK;
  const GaloisTables T = tables_for(g, d);
  if (g->flags & NTTMUL_FLAG_VALIDATE) {
    RnsTables R;
    R.logn = T.logn;
    R.limbs = T.limbs;
    R.word_bits = T.word_bits;
    R.q = T.q;
    G_TRY(g, hipMemsetAsync(d.flag, 0, sizeof(int), s));
    G_TRY(g, launch_rns_check(R, in, (batch * g->limbs) << g->logn, d.flag, s));
    int bad = 0;
    G_TRY(g, hipMemcpyAsync(&bad, d.flag, sizeof(int), hipMemcpyDeviceToHost, s));
    G_TRY(g, hipStreamSynchronize(s));
    if (bad) {
      set_err(g, "input word >= its limb's modulus");
      return NTTMUL_ERANGE;
    }
  }
  G_TRY(g, launch_galois(T, op, out, in, kv, count, batch, s));
  return NTTMUL_OK;
}

int device_op(nttmul_galois *g, int op, void *out, const void *in, const uint32_t *k,
              uint32_t count, size_t batch, int dev, void *stream) {
  GaloisKs kv;
  if (const int st = op_args(g, op, out, in, k, count, batch, &kv)) return st;
  GDev *d = find_dev(g, dev);
  if (!d) return NTTMUL_ENODEV;
  DeviceGuard guard;
  G_TRY(g, hipSetDevice(d->id));
  return run(g, *d, op, out, in, kv, count, batch, (hipStream_t)stream);
}

// Host buffers: dev[0], device buffers owned by the call, the device path, copy back, synchronise
int host_op(nttmul_galois *g, int op, void *out, const void *in, uint32_t k, size_t batch) {
  GaloisKs kv;
  if (const int st = op_args(g, op, out, in, &k, 1, batch, &kv)) return st;
  if (!batch) return NTTMUL_OK;
  GDev &d = g->dev[0];
  DeviceGuard guard;
  G_TRY(g, hipSetDevice(d.id));
  const size_t bytes = ((batch * g->limbs) << g->logn) * ((size_t)g->word_bits / 8);
  void *buf[2] = {nullptr, nullptr};  // out, in
  int st = NTTMUL_OK;
  const auto step = [&](hipError_t e, const char *what) {
    if (!st && e != hipSuccess) st = fail(g, e, what);
    return !st;
  };
  for (int i = 0; i < 2 && !st; i++) step(hipMalloc(&buf[i], bytes), "galois host buffers");
  if (!st) step(hipMemcpyAsync(buf[1], in, bytes, hipMemcpyHostToDevice, d.stream), "galois copy in");
  if (!st) st = run(g, d, op, buf[0], buf[1], kv, 1, batch, d.stream);
  if (!st)
    step(hipMemcpyAsync(out, buf[0], bytes, hipMemcpyDeviceToHost, d.stream), "galois copy out");
  // (also after a failure: nothing of this call may still run when its buffers go)
  step(hipStreamSynchronize(d.stream), "galois synchronise");
  for (void *p : buf)
    if (p) (void)hipFree(p);
  return st;
}

}  // namespace

extern "C" {

int nttmul_galois_create(nttmul_galois **out, const nttmul_params *caller, size_t size,
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
  if (n > 65536 || (p.flags & NTTMUL_FLAG_CYCLIC)) return NTTMUL_EUNSUPPORTED;
  // one word class per context: every q_l < 2^31 (32-bit words) or every q_l >= 2^32 (64-bit)
  const bool small = q[0] < (1ull << 31);
  for (uint32_t l = 0; l < limbs; l++) {
    if (q[l] >= (1ull << 31) && q[l] < (1ull << 32)) return NTTMUL_EUNSUPPORTED;
    if ((q[l] < (1ull << 31)) != small) return NTTMUL_EUNSUPPORTED;
  }
  nttmul_galois *g = new (std::nothrow) nttmul_galois();
  if (!g) return NTTMUL_ENOMEM;
  g->n = n;
  g->limbs = limbs;
  g->flags = p.flags;
  g->word_bits = small ? 32 : 64;
  g->plan.resize(limbs);
  for (uint32_t l = 0; l < limbs; l++) {
    const int st = make_plan(n, q[l], 0, &g->plan[l], false);
    if (st) {
      delete g;
      return st;
    }
    // the kernels read no twiddles
    std::vector<uint8_t>().swap(g->plan[l].fw);
    std::vector<uint8_t>().swap(g->plan[l].iw);
  }
  g->logn = g->plan[0].logn;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    delete g;
    return NTTMUL_ENODEV;
  }
  const int first = p.first_dev < 0 ? 0 : p.first_dev;
  const int ndev = p.ndev <= 0 ? count - first : p.ndev;
  const bool share = (p.flags & NTTMUL_FLAG_SHARE_DEVICES) != 0;
  if (first >= count || ndev <= 0 || (!share && first + ndev > count) || ndev > kMaxDev) {
    delete g;
    return NTTMUL_ENODEV;
  }
  DeviceGuard guard;
  for (int i = 0; i < ndev; i++) {
    GDev &d = g->dev[i];
    d.id = first + i % (count - first);
    g->ndev = i + 1;
    const int st = setup_device(g, d);
    if (st) {
      fprintf(stderr, "nttmul_galois: %s\n", g->err);
      nttmul_galois_destroy(g);
      return st == NTTMUL_EHIP ? NTTMUL_ENODEV : st;
    }
  }
  *out = g;
  return NTTMUL_OK;
}

void nttmul_galois_destroy(nttmul_galois *g) {
  if (!g) return;
  DeviceGuard guard;
  for (int i = 0; i < g->ndev; i++) {
    GDev &d = g->dev[i];
    if (d.id < 0) continue;
    (void)hipSetDevice(d.id);
    if (d.stream) (void)hipStreamSynchronize(d.stream);
    for (void *p : {(void *)d.q, (void *)d.flag})
      if (p) (void)hipFree(p);
    if (d.stream) (void)hipStreamDestroy(d.stream);
  }
  delete g;
}

const char *nttmul_galois_last_error(const nttmul_galois *g) { return g ? g->err : ""; }

int nttmul_galois_get_info(const nttmul_galois *g, nttmul_galois_info *info) {
  if (!g || !info) return NTTMUL_EINVAL;
  info->n = g->n;
  info->logn = g->logn;
  info->limbs = g->limbs;
  info->word_bits = (uint32_t)g->word_bits;
  info->ndev = g->ndev;
  return NTTMUL_OK;
}

int nttmul_galois_limb_info(const nttmul_galois *g, uint32_t limb, nttmul_info *info) {
  if (!g || !info || limb >= g->limbs) return NTTMUL_EINVAL;
  const Plan &P = g->plan[limb];
  info->n = P.n;
  info->logn = P.logn;
  info->q = P.q;
  info->psi = P.psi;
  info->omega = P.omega;
  info->inv_psi = P.inv_psi;
  info->inv_omega = P.inv_omega;
  info->inv_n = P.inv_n;
  info->word_bits = (uint32_t)P.word_bits;
  info->ndev = g->ndev;
  info->kernel = P.n > 4096 ? 2 : 1;
  info->cyclic = 0;
  return NTTMUL_OK;
}

int nttmul_galois_coeff_device(nttmul_galois *g, void *out, const void *in, uint32_t k,
                               size_t batch, int dev, void *stream) {
  return device_op(g, kGaloisCoeff, out, in, &k, 1, batch, dev, stream);
}
int nttmul_galois_ntt_device(nttmul_galois *g, void *out, const void *in, uint32_t k, size_t batch,
                             int dev, void *stream) {
  return device_op(g, kGaloisNtt, out, in, &k, 1, batch, dev, stream);
}
int nttmul_galois_ntt_many_device(nttmul_galois *g, void *out, const void *in, const uint32_t *k,
                                  uint32_t count, size_t batch, int dev, void *stream) {
  return device_op(g, kGaloisNttMany, out, in, k, count, batch, dev, stream);
}

int nttmul_galois_coeff(nttmul_galois *g, void *out, const void *in, uint32_t k, size_t batch) {
  return host_op(g, kGaloisCoeff, out, in, k, batch);
}
int nttmul_galois_ntt(nttmul_galois *g, void *out, const void *in, uint32_t k, size_t batch) {
  return host_op(g, kGaloisNtt, out, in, k, batch);
}

int nttmul_galois_kernel_name(const nttmul_galois *g, int op, uint32_t count, char *buf,
                              size_t cap) {
  if (!g || op < kGaloisCoeff || op > kGaloisNttMany || (cap && !buf)) return NTTMUL_EINVAL;
  if (op == kGaloisNttMany && (count == 0 || count > kGaloisMaxCount)) return NTTMUL_EINVAL;
  std::string name;
  if (describe_galois(tables_for(g, g->dev[0]), op, &name) != hipSuccess)
    return NTTMUL_EUNSUPPORTED;
  if (cap) {
    const size_t k = name.size() < cap - 1 ? name.size() : cap - 1;
    memcpy(buf, name.data(), k);
    buf[k] = 0;
  }
  return (int)name.size();
}

}  // extern "C"
