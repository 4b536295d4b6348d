// limb_ctx.cpp — the host runtime the limb-aware libraries share (limb_ctx.hpp).
#include "limb_ctx.hpp"

#include <stdio.h>
#include <string.h>

#include <mutex>

#include "rns.hpp"

namespace nttmul {

namespace {
std::mutex g_err_mu;
}  // namespace

int fail(char *err, hipError_t e, const char *what) {
  std::lock_guard<std::mutex> l(g_err_mu);
  snprintf(err, kErrBytes, "%s: %s", what, hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? NTTMUL_ENOMEM : NTTMUL_EHIP;
}

void set_err(char *err, const char *msg) {
  std::lock_guard<std::mutex> l(g_err_mu);
  snprintf(err, kErrBytes, "%s", msg);
}

int select_devices(const nttmul_params &p, DevRange *R) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    return NTTMUL_ENODEV;
  }
  const int first = p.first_dev < 0 ? 0 : p.first_dev;
  const int ndev = p.ndev <= 0 ? count - first : p.ndev;
  const bool share = (p.flags & NTTMUL_FLAG_SHARE_DEVICES) != 0;
  if (first >= count || ndev <= 0 || (!share && first + ndev > count) || ndev > kMaxDev)
    return NTTMUL_ENODEV;
  R->first = first;
  R->ndev = ndev;
  R->count = count;
  return NTTMUL_OK;
}

int create_failed(const char *lib, const char *err, int st) {
  fprintf(stderr, "%s: %s\n", lib, err);
  return st == NTTMUL_EHIP ? NTTMUL_ENODEV : st;
}

int upload(char *err, void **dst, const void *src, size_t bytes) {
  LIMB_TRY(err, hipMalloc(dst, bytes));
  LIMB_TRY(err, hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return NTTMUL_OK;
}

int check_range(char *err, int *flag, const uint64_t *q, uint32_t limbs, uint32_t logn,
                int word_bits, const void *a, size_t a_words, const void *b, size_t b_words,
                const char *msg, hipStream_t s) {
  RnsTables R;
  R.logn = logn;
  R.limbs = limbs;
  R.word_bits = word_bits;
  R.q = q;
  LIMB_TRY(err, hipMemsetAsync(flag, 0, sizeof(int), s));
  LIMB_TRY(err, launch_rns_check(R, a, a_words, flag, s));
  if (b_words) LIMB_TRY(err, launch_rns_check(R, b, b_words, flag, s));
  int bad = 0;
  LIMB_TRY(err, hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, s));
  LIMB_TRY(err, hipStreamSynchronize(s));
  if (bad) {
    set_err(err, msg);
    return NTTMUL_ERANGE;
  }
  return NTTMUL_OK;
}

namespace {

// the first failure of a host form's steps, as "<lib> <what>"
void step(char *err, int *st, hipError_t e, const char *lib, const char *what) {
  if (*st || e == hipSuccess) return;
  char text[64];
  snprintf(text, sizeof(text), "%s %s", lib, what);
  *st = fail(err, e, text);
}

}  // namespace

int staged_begin(char *err, const LimbDev &d, const char *lib, const Staged *ops, int count,
                 void **buf) {
  int st = NTTMUL_OK;
  for (int i = 0; i < count && !st; i++)
    if (ops[i].bytes) step(err, &st, hipMalloc(&buf[i], ops[i].bytes), lib, "host buffers");
  for (int i = 0; i < count && !st; i++)
    if (ops[i].src && ops[i].bytes)
      step(err, &st,
           hipMemcpyAsync(buf[i], ops[i].src, ops[i].bytes, hipMemcpyHostToDevice, d.stream), lib,
           "copy in");
  return st;
}

int staged_end(char *err, const LimbDev &d, const char *lib, const Staged *ops, int count,
               void **buf, int st) {
  for (int i = 0; i < count && !st; i++)
    if (ops[i].dst && ops[i].bytes)
      step(err, &st,
           hipMemcpyAsync(ops[i].dst, buf[i], ops[i].bytes, hipMemcpyDeviceToHost, d.stream), lib,
           "copy out");
  // (also after a failure: nothing of this call may still run when its buffers go)
  step(err, &st, hipStreamSynchronize(d.stream), lib, "synchronise");
  for (int i = 0; i < count; i++)
    if (buf[i]) (void)hipFree(buf[i]);
  return st;
}

int copy_name(const std::string &name, char *buf, size_t cap) {
  if (cap) {
    const size_t k = name.size() < cap - 1 ? name.size() : cap - 1;
    memcpy(buf, name.data(), k);
    buf[k] = 0;
  }
  return (int)name.size();
}

void fill_info(const Plan &P, int ndev, int kernel, nttmul_info *info) {
  info->n = P.n;
  info->logn = P.logn;
  info->q = P.q;
  info->psi = P.psi;
  info->omega = P.omega;
  info->inv_psi = P.inv_psi;
  info->inv_omega = P.inv_omega;
  info->inv_n = P.inv_n;
  info->word_bits = (uint32_t)P.word_bits;
  info->ndev = ndev;
  info->kernel = kernel;
  info->cyclic = 0;
}

}  // namespace nttmul
