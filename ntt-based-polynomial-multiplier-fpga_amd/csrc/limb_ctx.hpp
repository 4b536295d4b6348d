// limb_ctx.hpp — the host runtime the limb-aware libraries share (rns.cpp, bconv.cpp, rnsmp.cpp,
// galois.cpp, ks.cpp; in lib/libnttmul_rns.so and every library built on it): the device guard,
// the error text, the devices of a context from its params, and the shapes of a call — on the
// caller's device buffers and stream, or staged from host buffers on the context's own stream.
// Plain functions over plain fields: a library passes its handle's `err` buffer and its device
// entries, never the handle, and keeps what only it has (tables, scratch, argument checks).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <string>

#include "nttmul.h"
#include "planner.hpp"

namespace nttmul {

constexpr int kMaxDev = 16;        // devices of one context
constexpr size_t kErrBytes = 256;  // a handle's `char err[kErrBytes]`

struct DeviceGuard {  // restores the caller's current device on scope exit
  int prev = -1;
  DeviceGuard() { (void)hipGetDevice(&prev); }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// "<what>: <HIP's message>" into err (one writer at a time); NTTMUL_ENOMEM or NTTMUL_EHIP
int fail(char *err, hipError_t e, const char *what);
// a status message of our own (same lock as fail)
void set_err(char *err, const char *msg);

#define LIMB_TRY(err, expr)                            \
  do {                                                 \
    hipError_t _e = (expr);                            \
    if (_e != hipSuccess) return fail(err, _e, #expr); \
  } while (0)

// What every library keeps per device, as the member `base` of its own device entry
struct LimbDev {
  int id = -1;
  hipStream_t stream = nullptr;  // the host forms' stream
  uint64_t *q = nullptr;         // the moduli (range check)
  int *flag = nullptr;           // range-check result
};

// The devices a create serves, from the params' first_dev / ndev / NTTMUL_FLAG_SHARE_DEVICES and
// the machine's device count: entry i is device id(i)
struct DevRange {
  int first = 0, ndev = 0, count = 0;
  int id(int i) const { return first + i % (count - first); }
};
// NTTMUL_ENODEV without a device or for a range the machine does not have
int select_devices(const nttmul_params &p, DevRange *R);
// A create whose device setup failed with st: "<lib>: <err>" on stderr; the status create returns
// (a HIP failure at create means the device is not usable: NTTMUL_ENODEV)
int create_failed(const char *lib, const char *err, int st);

// hipMalloc *dst and copy `bytes` from host memory (create: the current device's tables)
int upload(char *err, void **dst, const void *src, size_t bytes);

template <class Dev>
Dev *find_dev(Dev *dev, int ndev, int id) {
  for (int i = 0; i < ndev; i++)
    if (dev[i].base.id == id) return &dev[i];
  return nullptr;
}

// The *_device forms: run(d) with the context's entry for device `id` current
template <class Dev, class Run>
int on_device(char *err, Dev *dev, int ndev, int id, Run run) {
  Dev *d = find_dev(dev, ndev, id);
  if (!d) return NTTMUL_ENODEV;
  DeviceGuard guard;
  LIMB_TRY(err, hipSetDevice(d->base.id));
  return run(*d);
}

// *_destroy: per device, synchronise the context's own stream (not the caller's streams), let
// free_owned(d) free what the library allocated there (base.q and base.flag too), destroy the stream
template <class Dev, class Free>
void destroy_devices(Dev *dev, int ndev, Free free_owned) {
  DeviceGuard guard;
  for (int i = 0; i < ndev; i++) {
    LimbDev &d = dev[i].base;
    if (d.id < 0) continue;
    (void)hipSetDevice(d.id);
    if (d.stream) (void)hipStreamSynchronize(d.stream);
    free_owned(dev[i]);
    if (d.stream) (void)hipStreamDestroy(d.stream);
  }
}
inline void free_each(std::initializer_list<void *> ptrs) {
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
}

// The NTTMUL_FLAG_VALIDATE check on stream s (k_rns_check_range, rns.hip): every word of a (and of
// b when b_words) below its limb's modulus, q[(i >> logn) mod limbs].  Synchronises s.
// NTTMUL_ERANGE with msg as the error text.
int check_range(char *err, int *flag, const uint64_t *q, uint32_t limbs, uint32_t logn,
                int word_bits, const void *a, size_t a_words, const void *b, size_t b_words,
                const char *msg, hipStream_t s);

// One operand of a host form: `bytes` of device memory owned by the call (none for 0 bytes),
// filled from src before the run when src is set, copied to dst after it when dst is set
struct Staged {
  const void *src;
  void *dst;
  size_t bytes;
};
// The two halves of staged_op.  staged_end synchronises d.stream before it frees, also after a
// failure: nothing of the call may still run when its buffers go.
int staged_begin(char *err, const LimbDev &d, const char *lib, const Staged *ops, int count,
                 void **buf);
int staged_end(char *err, const LimbDev &d, const char *lib, const Staged *ops, int count,
               void **buf, int st);

// The host forms, on device entry d: allocate, copy in, run(buf) with buf[i] the device buffer of
// ops[i] (enqueued on d.stream), copy out, synchronise, free.  `lib` prefixes the error texts
// ("rns host buffers").
template <class Run>
int staged_op(char *err, const LimbDev &d, const char *lib, const Staged *ops, int count, Run run) {
  DeviceGuard guard;
  LIMB_TRY(err, hipSetDevice(d.id));
  void *buf[3] = {nullptr, nullptr, nullptr};
  int st = staged_begin(err, d, lib, ops, count, buf);
  if (!st) st = run(buf);
  return staged_end(err, d, lib, ops, count, buf, st);
}

// *_kernel_name's tail: name into buf (truncated to cap - 1 characters and terminated when cap);
// the full length
int copy_name(const std::string &name, char *buf, size_t cap);

// *_limb_info: one limb's plan as nttmul_get_info reports a plain context's
void fill_info(const Plan &P, int ndev, int kernel, nttmul_info *info);

}  // namespace nttmul
