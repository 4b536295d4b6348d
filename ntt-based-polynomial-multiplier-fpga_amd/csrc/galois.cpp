// galois.cpp — host runtime behind include/nttmul_galois.h (lib/libnttmul_galois.so only): a context
// of several moduli for one degree 256 <= n <= 65536, and the one launch per call over
// [batch][limbs][n] operands (galois.hip).  A context keeps, per device, the moduli and the range
// check's flag: the kernels read no twiddles and no index table.  No scratch, no CPU fallback.
// The host-only entry points (nttmul_galois_element, nttmul_galois_plan) and the index arithmetic
// are in galois_plan.cpp.
// The create-time checks are basis.cpp's and the context runtime limb_ctx.cpp's.  This file keeps
// its handle, its run, and the handling of the automorphisms k (op_args).
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "basis.hpp"
#include "galois.hpp"
#include "limb_ctx.hpp"
#include "nttmul_galois.h"
#include "planner.hpp"

using namespace nttmul;

namespace {

struct GDev {
  LimbDev base;
};

}  // namespace

struct nttmul_galois {
  uint32_t n = 0, logn = 0, limbs = 0, flags = 0;
  int word_bits = 0, ndev = 0;
  std::vector<Plan> plan;  // per limb, for nttmul_galois_limb_info (twiddle vectors released)
  GDev dev[kMaxDev];
  char err[kErrBytes] = {0};
};

namespace {

GaloisTables tables_for(const nttmul_galois *g, const GDev &d) {
  GaloisTables T;
  T.logn = g->logn;
  T.limbs = g->limbs;
  T.word_bits = g->word_bits;
  T.q = d.base.q;
  return T;
}

int setup_device(nttmul_galois *g, GDev &d) {
  const uint32_t L = g->limbs;
  LIMB_TRY(g->err, hipSetDevice(d.base.id));
  LIMB_TRY(g->err, hipStreamCreateWithFlags(&d.base.stream, hipStreamNonBlocking));
  LIMB_TRY(g->err, hipMalloc((void **)&d.base.q, sizeof(uint64_t) * L));
  LIMB_TRY(g->err, hipMalloc((void **)&d.base.flag, sizeof(int)));
  std::vector<uint64_t> q(L);
  for (uint32_t l = 0; l < L; l++) q[l] = g->plan[l].q;
  LIMB_TRY(g->err, hipMemcpy(d.base.q, q.data(), sizeof(uint64_t) * L, hipMemcpyHostToDevice));
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
  if (g->flags & NTTMUL_FLAG_VALIDATE)
    if (const int st = check_range(g->err, d.base.flag, d.base.q, g->limbs, g->logn, g->word_bits,
                                   in, (batch * g->limbs) << g->logn, nullptr, 0,
                                   "input word >= its limb's modulus", s))
      return st;
  LIMB_TRY(g->err, launch_galois(tables_for(g, d), op, out, in, kv, count, batch, s));
  return NTTMUL_OK;
}

int device_op(nttmul_galois *g, int op, void *out, const void *in, const uint32_t *k,
              uint32_t count, size_t batch, int dev, void *stream) {
  GaloisKs kv;
  if (const int st = op_args(g, op, out, in, k, count, batch, &kv)) return st;
  return on_device(g->err, g->dev, g->ndev, dev, [&](GDev &d) {
    return run(g, d, op, out, in, kv, count, batch, (hipStream_t)stream);
  });
}

// Host buffers: dev[0], device buffers owned by the call, the device path, copy back, synchronise
int host_op(nttmul_galois *g, int op, void *out, const void *in, uint32_t k, size_t batch) {
  GaloisKs kv;
  if (const int st = op_args(g, op, out, in, &k, 1, batch, &kv)) return st;
  if (!batch) return NTTMUL_OK;
  GDev &d = g->dev[0];
  const size_t bytes = ((batch * g->limbs) << g->logn) * ((size_t)g->word_bits / 8);
  const Staged ops[2] = {{nullptr, out, bytes}, {in, nullptr, bytes}};
  return staged_op(g->err, d.base, "galois", ops, 2, [&](void *const *buf) {
    return run(g, d, op, buf[0], buf[1], kv, 1, batch, d.base.stream);
  });
}

}  // namespace

extern "C" {

int nttmul_galois_create(nttmul_galois **out, const nttmul_params *caller, size_t size,
                         const uint64_t *q, uint32_t limbs) {
  if (!out) return NTTMUL_EINVAL;
  *out = nullptr;
  // a degree above 65536 is valid and unsupported
  BasisRequest B;
  if (const int st = basis_invalid(caller, size, &q, &limbs, 1, 1u << 30, &B)) return st;
  if (const int st = basis_unsupported(&B, 256, 65536, false)) return st;
  nttmul_galois *g = new (std::nothrow) nttmul_galois();
  if (!g) return NTTMUL_ENOMEM;
  g->n = B.prm.n;
  g->limbs = limbs;
  g->flags = B.prm.flags;
  g->word_bits = B.word_bits;
  g->plan.resize(limbs);
  for (uint32_t l = 0; l < limbs; l++) {
    const int st = make_plan(g->n, q[l], 0, &g->plan[l], false);
    if (st) {
      delete g;
      return st;
    }
    // the kernels read no twiddles
    std::vector<uint8_t>().swap(g->plan[l].fw);
    std::vector<uint8_t>().swap(g->plan[l].iw);
  }
  g->logn = g->plan[0].logn;
  DevRange R;
  if (const int st = select_devices(B.prm, &R)) {
    delete g;
    return st;
  }
  DeviceGuard guard;
  for (int i = 0; i < R.ndev; i++) {
    GDev &d = g->dev[i];
    d.base.id = R.id(i);
    g->ndev = i + 1;
    const int st = setup_device(g, d);
    if (st) {
      const int ret = create_failed("nttmul_galois", g->err, st);
      nttmul_galois_destroy(g);
      return ret;
    }
  }
  *out = g;
  return NTTMUL_OK;
}

void nttmul_galois_destroy(nttmul_galois *g) {
  if (!g) return;
  destroy_devices(g->dev, g->ndev, [](GDev &d) { free_each({d.base.q, d.base.flag}); });
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
  fill_info(g->plan[limb], g->ndev, g->n > 4096 ? 2 : 1, info);
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
  return copy_name(name, buf, cap);
}

}  // extern "C"
