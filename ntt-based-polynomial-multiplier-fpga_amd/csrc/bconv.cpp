// bconv.cpp — host runtime behind include/nttmul_bconv.h (lib/libnttmul_bconv.so only): a
// converter between two disjoint RNS bases of one word class for one degree n <= 4096, and one
// launch per conversion over [batch][limbs][n] operands (bconv.hip).  The constants come from the
// planner's modular arithmetic (planner.hpp mulmod / powmod) in 128-bit host integers;
// nttmul_bconv_plan returns them plain, create derives its device tables from the same values.
// No resident server, no CPU fallback.
// The create-time checks are basis.cpp's and the context runtime limb_ctx.cpp's.  This file keeps
// its handle, its plain constants, its run, and the one host side of k_bconv's device table
// format (bconv.hpp mul_pair, neg_inv, build_tables), which ks.cpp builds its tables with too.
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "basis.hpp"
#include "bconv.hpp"
#include "limb_ctx.hpp"
#include "nttmul_bconv.h"
#include "planner.hpp"

using namespace nttmul;

namespace {

using u128 = unsigned __int128;

struct BconvDev {
  LimbDev base;                               // q: c_0 .. c_{K-1}, b_0 .. b_{L-1}
  void *from = nullptr, *to = nullptr, *w = nullptr;
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
  char err[kErrBytes] = {0};
};

namespace nttmul {

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
template void mul_pair<uint32_t>(uint64_t, uint64_t, uint32_t *, uint32_t *);
template void mul_pair<uint64_t>(uint64_t, uint64_t, uint64_t *, uint64_t *);

uint64_t neg_inv(uint64_t q) {
  uint64_t inv = q;
  for (int i = 0; i < 6; i++) inv *= 2 - q * inv;
  return 0 - inv;
}

}  // namespace nttmul

namespace {

template <class W>
void fill_tables(const std::vector<uint64_t> &b, const std::vector<uint64_t> &inv,
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

}  // namespace

namespace nttmul {

void build_tables(int word_bits, const std::vector<uint64_t> &b, const std::vector<uint64_t> &inv,
                  const std::vector<uint64_t> &c, const std::vector<uint64_t> &binv,
                  const std::vector<uint64_t> &w, std::vector<uint8_t> *from,
                  std::vector<uint8_t> *to, std::vector<uint8_t> *wt) {
  if (word_bits == 32)
    fill_tables<uint32_t>(b, inv, c, binv, w, from, to, wt);
  else
    fill_tables<uint64_t>(b, inv, c, binv, w, from, to, wt);
}

}  // namespace nttmul

namespace {

// What create and plan decide before any device access (basis.hpp): every EINVAL of either basis
// first, then the unsupported shapes, then the word classes.  *prm: the zero-extended params
int validate(const nttmul_params *caller, size_t size, const uint64_t *from_q, uint32_t L,
             const uint64_t *to_q, uint32_t K, BconvPlan *P, nttmul_params *prm) {
  const uint64_t *const q[2] = {from_q, to_q};
  const uint32_t limbs[2] = {L, K};
  BasisRequest B;
  if (const int st = basis_invalid(caller, size, q, limbs, 2, 65536, &B)) return st;
  // (p3_fold: what nttmul_rns_create asks of a 32-bit basis at n = 4096)
  if (const int st = basis_unsupported(&B, 256, 4096, true)) return st;
  P->n = B.prm.n;
  P->logn = (uint32_t)__builtin_ctz(P->n);
  P->L = L;
  P->K = K;
  P->flags = B.prm.flags;
  P->word_bits = B.word_bits;
  P->b.assign(from_q, from_q + L);
  P->c.assign(to_q, to_q + K);
  *prm = B.prm;
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

BconvTables tables_for(const nttmul_bconv *h, const BconvDev &d) {
  BconvTables T;
  T.logn = h->plan.logn;
  T.from_limbs = h->plan.L;
  T.to_limbs = h->plan.K;
  T.word_bits = h->plan.word_bits;
  T.from = d.from;
  T.to = d.to;
  T.w = d.w;
  T.q = d.base.q;
  return T;
}

int setup_device(nttmul_bconv *h, BconvDev &d) {
  const BconvPlan &P = h->plan;
  LIMB_TRY(h->err, hipSetDevice(d.base.id));
  LIMB_TRY(h->err, hipStreamCreateWithFlags(&d.base.stream, hipStreamNonBlocking));
  LIMB_TRY(h->err, hipMalloc((void **)&d.base.flag, sizeof(int)));
  std::vector<uint8_t> from, to, w;
  build_tables(P.word_bits, P.b, P.inv, P.c, P.binv, P.w, &from, &to, &w);
  std::vector<uint64_t> q(P.c);
  q.insert(q.end(), P.b.begin(), P.b.end());
  if (const int st = upload(h->err, &d.from, from.data(), from.size())) return st;
  if (const int st = upload(h->err, &d.to, to.data(), to.size())) return st;
  if (const int st = upload(h->err, &d.w, w.data(), w.size())) return st;
  return upload(h->err, (void **)&d.base.q, q.data(), sizeof(uint64_t) * q.size());
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
  if (h->plan.flags & NTTMUL_FLAG_VALIDATE) {
    // k_rns_check_range over the input's own limbs: all K + L of moddown's, the last L of the
    // moduli list for convert's
    const uint32_t limbs = in_limbs(h, op);
    if (const int st = check_range(h->err, d.base.flag,
                                   op == kBconvModdown ? d.base.q : d.base.q + h->plan.K, limbs,
                                   h->plan.logn, h->plan.word_bits, in, batch * limbs * h->plan.n,
                                   nullptr, 0, "input coefficient >= its limb's modulus", s))
      return st;
  }
  LIMB_TRY(h->err, launch_bconv(tables_for(h, d), op, out, in, batch, s));
  return NTTMUL_OK;
}

int device_op(nttmul_bconv *h, int op, void *out, const void *in, size_t batch, int dev,
              void *stream) {
  if (const int st = op_args(h, out, in, batch)) return st;
  return on_device(h->err, h->dev, h->ndev, dev, [&](BconvDev &d) {
    return run(h, d, op, out, in, batch, (hipStream_t)stream);
  });
}

// Host buffers: dev[0], device buffers owned by the call, the device path, copy back, synchronise
int host_op(nttmul_bconv *h, int op, void *out, const void *in, size_t batch) {
  if (const int st = op_args(h, out, in, batch)) return st;
  if (!batch) return NTTMUL_OK;
  BconvDev &d = h->dev[0];
  const size_t wb = (size_t)h->plan.word_bits / 8, poly = (size_t)h->plan.n * wb * batch;
  const Staged ops[2] = {{nullptr, out, poly * h->plan.K}, {in, nullptr, poly * in_limbs(h, op)}};
  return staged_op(h->err, d.base, "bconv", ops, 2, [&](void *const *buf) {
    return run(h, d, op, buf[0], buf[1], batch, d.base.stream);
  });
}

}  // namespace

extern "C" {

int nttmul_bconv_plan(const nttmul_params *params, size_t size, const uint64_t *from_q,
                      uint32_t from_limbs, const uint64_t *to_q, uint32_t to_limbs, uint64_t *inv,
                      uint64_t *w, uint64_t *binv) {
  if (!inv || !w || !binv) return NTTMUL_EINVAL;
  BconvPlan P;
  nttmul_params prm;
  if (const int st = validate(params, size, from_q, from_limbs, to_q, to_limbs, &P, &prm))
    return st;
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
  nttmul_params prm;
  if (const int st = validate(params, size, from_q, from_limbs, to_q, to_limbs, &h->plan, &prm)) {
    delete h;
    return st;
  }
  plan_constants(&h->plan);
  DevRange R;
  if (const int st = select_devices(prm, &R)) {
    delete h;
    return st;
  }
  DeviceGuard guard;
  for (int i = 0; i < R.ndev; i++) {
    BconvDev &d = h->dev[i];
    d.base.id = R.id(i);
    h->ndev = i + 1;
    if (const int st = setup_device(h, d)) {
      const int ret = create_failed("nttmul_bconv", h->err, st);
      nttmul_bconv_destroy(h);
      return ret;
    }
  }
  *out = h;
  return NTTMUL_OK;
}

void nttmul_bconv_destroy(nttmul_bconv *h) {
  if (!h) return;
  destroy_devices(h->dev, h->ndev, [](BconvDev &d) {
    free_each({d.from, d.to, d.w, d.base.q, d.base.flag});
  });
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
  return copy_name(name, buf, cap);
}

}  // extern "C"
