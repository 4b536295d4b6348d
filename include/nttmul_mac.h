/*
 * nttmul_mac.h — products and dot products against NTT-domain operands: lib/libnttmul_mac.so
 * (not libnttmul.so).
 *
 * libnttmul_mac.so holds the whole C ABI of include/nttmul.h with the same kernels, plus the entry
 * points below and the kernel behind them (csrc/mac_dev.hpp k_mac).  A context is created with the
 * nttmul_create* of that library.
 *
 * For a context of degree n <= 4096 and p < batch
 *
 *     c[p] = INTT( sum over t < terms of  NTT(a[p][t]) o b_hat[shared ? 0 : p][t] )
 *
 * where NTT is the context's nttmul_forward_* (standard order in, bit-reversed out), INTT its
 * nttmul_inverse_* (scaled by n^-1) and o the coefficient-wise product mod q; on a
 * NTTMUL_FLAG_CYCLIC context the same formula uses the cyclic transforms.  One launch: terms
 * forward transforms, one inverse, no intermediate written.
 *
 *   a      [batch][terms][n], standard order, canonical
 *   b_hat  [batch][terms][n], or [terms][n] when shared != 0: exactly the element order and range
 *          nttmul_forward_* writes (bit-reversed, canonical [0, q)).  Any canonical vector is
 *          accepted, whether or not it is the transform of something.
 *   c      [batch][n], standard order, canonical.  c must not overlap a or b_hat.
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_footprint.py).  Alignment: operands need the
 * alignment of their word only.  Aliasing: none is allowed here; c must not overlap a or b_hat,
 * not even exactly.  Footprint: a call writes exactly batch * n words of c and nothing else in
 * caller memory; a and b_hat are never written.
 *
 * terms = 1 multiplies by an NTT-domain operand.  With b_hat = forward(b) the result equals, bit
 * for bit, the sum over t of nttmul_multiply(a[p][t], b[..][t]) mod q.
 *
 * Status: batch = 0 is a successful no-op.  terms = 0, a NULL context, a NULL operand with
 * batch > 0, a word size other than 32 or 64, or 32-bit words for q >= 2^32 return NTTMUL_EINVAL,
 * decided before any device access.  n > 4096 returns NTTMUL_EUNSUPPORTED.  With
 * NTTMUL_FLAG_VALIDATE a and b_hat are range-checked on the device (NTTMUL_ERANGE).
 *
 * Out of scope here: n > 4096 (forward launches into scratch, a coefficient-wise
 * multiply-accumulate and the existing inverse, sub-batched through scratch_mb); an opaque
 * prepared-operand format that would keep the product kernels' base blocks; the resident device
 * server and the issue-priority rule, which keep describing plain products only
 * (nttmul_last_kernel_name does not report these calls).
 */
#ifndef NTTMUL_MAC_H
#define NTTMUL_MAC_H

#include "nttmul.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device-resident operands on HIP device `dev` (one of the context's), enqueued on `stream`;
 * asynchronous, as nttmul_multiply_batch_device (with NTTMUL_FLAG_VALIDATE it waits for the range
 * check).  word_bits: 32 or 64, the word size of a, b_hat and c. */
int nttmul_mac_ntt_device(nttmul_ctx *ctx, void *c, const void *a, const void *b_hat,
                          size_t batch, uint32_t terms, int shared, int word_bits, int dev,
                          void *stream);

/* Host buffers.  Deliberately simple: the context's first device only, operands copied to device
 * buffers owned by the call, the device path, a copy back and a synchronise.  No chunk pipeline
 * and no multi-device split: a caller with large batches keeps them on the device. */
int nttmul_mac_ntt_u32(nttmul_ctx *ctx, uint32_t *c, const uint32_t *a, const uint32_t *b_hat,
                       size_t batch, uint32_t terms, int shared);
int nttmul_mac_ntt_u64(nttmul_ctx *ctx, uint64_t *c, const uint64_t *a, const uint64_t *b_hat,
                       size_t batch, uint32_t terms, int shared);

/* The kernel a call with word_bits-wide words dispatches to, in the format of nttmul_kernel_name,
 * e.g. "k_mac<Arith32P,u32,u32,12>" (the shared form is a stride of the same kernel).  Returns
 * the untruncated length, or a negative status. */
int nttmul_mac_kernel_name(const nttmul_ctx *ctx, int word_bits, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_MAC_H */
