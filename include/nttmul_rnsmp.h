/*
 * nttmul_rnsmp.h — limb-aware multi-pass RNS for 4096 < n <= 65536: lib/libnttmul_rnsmp.so (not
 * libnttmul_rns.so, not libnttmul_bconv.so).
 *
 * libnttmul_rnsmp.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h, nttmul_rns.h and
 * nttmul_bconv.h with the same kernels, plus the entry points below and the kernels behind them
 * (csrc/rnsmp_dev.hpp k_rnsmp_cols_fwd, k_rnsmp_rows, k_rnsmp_xform, k_rnsmp_mac,
 * k_rnsmp_cols_inv).
 *
 * An nttmul_rnsmp context holds L = limbs distinct primes q_0 .. q_{L-1} for one degree
 * n in {8192, 16384, 32768, 65536}, the degrees at which an RNS basis of 31- or 62-bit primes is
 * used in earnest.  n <= 4096 stays with nttmul_rns_* (include/nttmul_rns.h), whose semantics
 * these calls keep.  A batch is one array [batch][limbs][n]: polynomial p of limb l starts at
 * word (p L + l) n.  A plain context runs a product of this size as three launches (column pass,
 * rows of 4096, column pass), so L plain contexts need 3 L launches on L limb-major arrays; here
 * every pass is one launch over all limbs (grid: workgroups x limbs):
 *
 *   multiply  3 launches   c[p][l] = a[p][l] * b[p][l]           in Z_{q_l}[x]/(x^n + 1)
 *   forward   2 launches   standard order in, bit-reversed canonical out    (nttmul_forward_*)
 *   inverse   2 launches   bit-reversed in, scaled by n^-1, standard canonical out
 *   mac_ntt   3 launches for any number of terms
 *             c[p][l] = INTT_l( sum over t < terms of NTT_l(a[p][t][l]) o b_hat[p or 0][t][l] );
 *             a [batch][terms][limbs][n],  b_hat [batch][terms][limbs][n], or [terms][limbs][n]
 *             when shared != 0.  The plain ABI has no counterpart at these degrees
 *             (nttmul_mac_ntt_* stops at n = 4096).
 *
 * Per limb the results are the existing library's, bit for bit: limb l of every result equals
 * what a plain context nttmul_create(n, q_l) returns for that limb's operands.  The forward
 * output is bit-reversed and canonical, the inverse output scaled by n^-1, canonical and in
 * standard order.  b_hat is exactly what nttmul_rnsmp_forward_* writes, which per limb is what
 * the plain nttmul_forward_* writes; any canonical b_hat is accepted.
 *
 * Each limb takes psi = nttmul_smallest_psi(n, q_l), as nttmul_create does.
 *
 * Word size.  Either every q_l < 2^31 and all operands are 32-bit words, or every q_l >= 2^32
 * (q_l < 2^62) and all operands are 64-bit words; nttmul_rnsmp_info.word_bits says which.
 *
 * Status, all decided before any device access: NTTMUL_EINVAL for a NULL context, limbs of 0 or
 * above NTTMUL_RNS_MAX_LIMBS, an n that is not a power of two or below 256, a q_l that is not
 * prime, not 1 mod 2n or >= 2^62, two equal primes, non-zero params->q or params->psi, terms = 0,
 * or a NULL operand with batch > 0.  NTTMUL_EUNSUPPORTED for a valid n <= 4096 (use nttmul_rns_*),
 * for n > 65536, for NTTMUL_FLAG_CYCLIC, for any q_l in [2^31, 2^32) and for mixed classes.
 * batch = 0 is a successful no-op.  NTTMUL_ENODEV as in nttmul.h (no device, or `dev` not one of
 * the context's).
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_rnsmp_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  out == in is allowed for the two transforms (in place): every pass moves
 *     between caller memory and the context's scratch, so the pass that reads a sub-batch's `in`
 *     has finished before the pass that writes its `out` starts.  c must not overlap a, b or b_hat.
 *     Partial overlap of two operands is never allowed.
 *   Footprint.  A call writes exactly batch * limbs * n words of its output and nothing else in
 *     caller memory; inputs are never written.
 *
 * Scratch.  The intermediates of the passes live in a scratch that belongs to the context (per
 * device), allocated on first use.  params->scratch_mb has the meaning it has in nttmul.h
 * (default 512): at most that many MiB per scratch buffer; a larger batch runs in sub-batches of
 * whole polynomials, where for the mac's a "whole" means all limbs and all terms of a polynomial.
 * A sub-batch is never smaller than one polynomial: the scratch grows to hold it.  The scratch is
 * handed between streams by an event: a call on stream B after a call on stream A waits for A's
 * last kernel.  One context serves one host thread at a time.
 * nttmul_rnsmp_destroy does not wait for the streams passed to the *_device calls: synchronise
 * them first, a kernel still queued there would read freed tables.
 *
 * NTTMUL_FLAG_VALIDATE range-checks every operand word against its own limb's modulus on the
 * device (word i belongs to limb (i / n) mod limbs) and returns NTTMUL_ERANGE; the call then
 * waits for the check.
 *
 * These calls use neither the resident device server nor the issue-priority rule.
 *
 * Out of scope here:
 *   - n <= 4096 (include/nttmul_rns.h);
 *   - the square 256 x 256 split and tiled intermediates that the plain library uses for 64-bit
 *     words at n = 65536: both classes take the 2^(logn - 12) x 4096 split here (same results;
 *     the plain library priced the difference at 5 .. 7 % for that one shape);
 *   - base conversion above n = 4096 (nttmul_bconv_* keeps its own limit);
 *   - 64-bit storage of 32-bit limbs, and the class 2^31 <= q < 2^32;
 *   - a chunked or multi-device host path (the host forms below are deliberately simple);
 *   - cyclic contexts (NTTMUL_FLAG_CYCLIC), the device server, issue priority.
 */
#ifndef NTTMUL_RNSMP_H
#define NTTMUL_RNSMP_H

#include "nttmul_rns.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nttmul_rnsmp nttmul_rnsmp;

typedef struct {
  uint32_t n, logn, limbs;
  uint32_t word_bits;  /* 32: every q_l < 2^31; 64: every q_l >= 2^32.  The word of every operand */
  int ndev;
  uint32_t scratch_mb; /* MiB per scratch buffer (params->scratch_mb, or the default) */
} nttmul_rnsmp_info;

/* params: n, ndev, first_dev, flags and scratch_mb as for nttmul_create_sized (params_size
 * likewise); params->q and params->psi must be 0; the other dispatch knobs are ignored.
 * q[0 .. limbs): the moduli, in limb order. */
int nttmul_rnsmp_create(nttmul_rnsmp **r, const nttmul_params *params, size_t params_size,
                        const uint64_t *q, uint32_t limbs);
void nttmul_rnsmp_destroy(nttmul_rnsmp *r);
const char *nttmul_rnsmp_last_error(const nttmul_rnsmp *r);
int nttmul_rnsmp_get_info(const nttmul_rnsmp *r, nttmul_rnsmp_info *info);
/* q, psi, omega, ... of one limb, as nttmul_get_info of a plain context of (n, q_limb) */
int nttmul_rnsmp_limb_info(const nttmul_rnsmp *r, uint32_t limb, nttmul_info *info);

/* Device-resident operands of info.word_bits-wide words on HIP device `dev` (one of the
 * context's), enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE they wait for the
 * range check; a call that grows the scratch waits for the scratch's last use).
 * a, b, c, in, out: [batch][limbs][n]. */
int nttmul_rnsmp_multiply_device(nttmul_rnsmp *r, void *c, const void *a, const void *b,
                                 size_t batch, int dev, void *stream);
int nttmul_rnsmp_forward_device(nttmul_rnsmp *r, void *out, const void *in, size_t batch, int dev,
                                void *stream);
int nttmul_rnsmp_inverse_device(nttmul_rnsmp *r, void *out, const void *in, size_t batch, int dev,
                                void *stream);
int nttmul_rnsmp_mac_ntt_device(nttmul_rnsmp *r, void *c, const void *a, const void *b_hat,
                                size_t batch, uint32_t terms, int shared, int dev, void *stream);

/* Host buffers.  Deliberately simple, as nttmul_rns_*: the context's first device, device buffers
 * owned by the call, the device path, a copy back and a synchronise. */
int nttmul_rnsmp_multiply(nttmul_rnsmp *r, void *c, const void *a, const void *b, size_t batch);
int nttmul_rnsmp_forward(nttmul_rnsmp *r, void *out, const void *in, size_t batch);
int nttmul_rnsmp_inverse(nttmul_rnsmp *r, void *out, const void *in, size_t batch);
int nttmul_rnsmp_mac_ntt(nttmul_rnsmp *r, void *c, const void *a, const void *b_hat, size_t batch,
                         uint32_t terms, int shared);

/* The launch sequence of an operation (op: 0 multiply, 1 forward, 2 inverse, 3 mac), the kernels
 * joined by " + " as nttmul_kernel_name joins a multi-pass product's, e.g.
 * "k_rnsmp_cols_fwd<Arith32P,u32,1,2> + k_rnsmp_rows<Arith32P,1> + k_rnsmp_cols_inv<Arith32P,u32,1>"
 * (the number after the word: L1 = logn - 12; k_rnsmp_cols_fwd's last: polynomials per column,
 * k_rnsmp_xform's last: 0 forward, 1 inverse).  Each name is the kernel's full template argument
 * list.  Returns the untruncated length, or a negative status. */
int nttmul_rnsmp_kernel_name(const nttmul_rnsmp *r, int op, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_RNSMP_H */
