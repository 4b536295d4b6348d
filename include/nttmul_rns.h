/*
 * nttmul_rns.h — one launch over all limbs of an RNS basis: lib/libnttmul_rns.so (not
 * libnttmul.so, not libnttmul_mac.so).
 *
 * libnttmul_rns.so holds the whole C ABI of include/nttmul.h and include/nttmul_mac.h with the
 * same kernels, plus the entry points below and the kernels behind them (csrc/rns_dev.hpp
 * k_rns_rows, k_rns_xform, k_rns_mac).
 *
 * An nttmul_rns context holds L = limbs distinct primes q_0 .. q_{L-1} for one degree n <= 4096.
 * A polynomial modulo Q = q_0 q_1 .. q_{L-1} is stored as L residue limbs of n words, limb l
 * reduced mod q_l, and a batch is one array [batch][limbs][n]: polynomial p of limb l starts at
 * word (p L + l) n.  Every operation is one kernel launch over the whole array (grid: workgroups
 * over the batch x limbs), where L plain contexts need L launches on L limb-major arrays.
 *
 * Per limb the results are the existing library's, bit for bit: limb l of every result equals
 * what a plain context nttmul_create(n, q_l) returns for that limb's operands.
 *
 *   multiply  c[p][l] = a[p][l] * b[p][l]                      in Z_{q_l}[x]/(x^n + 1)
 *   forward   standard order in, bit-reversed canonical out     (nttmul_forward_*)
 *   inverse   bit-reversed in, scaled by n^-1, standard canonical out  (nttmul_inverse_*)
 *   mac_ntt   c[p][l] = INTT_l( sum over t < terms of NTT_l(a[p][t][l]) o b_hat[p or 0][t][l] )
 *             (nttmul_mac.h, per limb);  a [batch][terms][limbs][n],  b_hat [batch][terms][limbs][n],
 *             or [terms][limbs][n] when shared != 0; any canonical b_hat is accepted
 *
 * Each limb takes psi = nttmul_smallest_psi(n, q_l), as nttmul_create does.
 *
 * Word size.  Either every q_l < 2^31 and all operands are 32-bit words, or every q_l >= 2^32
 * (q_l < 2^62) and all operands are 64-bit words; nttmul_rns_info.word_bits says which.  Mixed
 * classes, and any q_l in [2^31, 2^32), return NTTMUL_EUNSUPPORTED.
 *
 * Status, all decided before any device access: NTTMUL_EINVAL for a NULL context, limbs of 0 or
 * above NTTMUL_RNS_MAX_LIMBS, a q_l that nttmul_create would refuse (not prime, not 1 mod 2n,
 * >= 2^62; or an n it refuses), two equal primes, non-zero params->q or params->psi, terms = 0,
 * or a NULL operand with batch > 0.  NTTMUL_EUNSUPPORTED for a valid n above 4096, for
 * NTTMUL_FLAG_CYCLIC and for the word classes above.  batch = 0 is a successful no-op.
 * NTTMUL_ENODEV as in nttmul.h (no device, or `dev` not one of the context's).
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  out == in is allowed for the two transforms (in place).  c must not overlap a, b
 *     or b_hat.  Partial overlap of two operands is never allowed.
 *   Footprint.  A call writes exactly batch * limbs * n words of its output and nothing else in
 *     caller memory; inputs are never written.
 *
 * NTTMUL_FLAG_VALIDATE range-checks every operand word against its own limb's modulus on the
 * device (word i belongs to limb (i / n) mod limbs) and returns NTTMUL_ERANGE; the call then
 * waits for the check.
 *
 * These calls use neither the resident device server nor the issue-priority rule: every launch
 * issues oldest-first.
 *
 * Out of scope here:
 *   - n > 4096 (the column passes of the multi-pass product are not limb-aware); that is
 *     include/nttmul_rnsmp.h, lib/libnttmul_rnsmp.so;
 *   - 64-bit storage of 32-bit limbs, and the class 2^31 <= q < 2^32;
 *   - CRT reconstruction (base conversion between bases: include/nttmul_bconv.h,
 *     lib/libnttmul_bconv.so);
 *   - a chunked or multi-device host path (the host forms below are deliberately simple);
 *   - cyclic contexts (NTTMUL_FLAG_CYCLIC).
 */
#ifndef NTTMUL_RNS_H
#define NTTMUL_RNS_H

#include "nttmul_mac.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nttmul_rns nttmul_rns;
#define NTTMUL_RNS_MAX_LIMBS 64

typedef struct {
  uint32_t n, logn, limbs;
  uint32_t word_bits;  /* 32: every q_l < 2^31; 64: every q_l >= 2^32.  The word of every operand */
  int ndev;
} nttmul_rns_info;

/* params: n, ndev, first_dev and flags as for nttmul_create_sized (params_size likewise);
 * params->q and params->psi must be 0; the dispatch knobs are ignored.  q[0 .. limbs): the
 * moduli, in limb order. */
int nttmul_rns_create(nttmul_rns **r, const nttmul_params *params, size_t params_size,
                      const uint64_t *q, uint32_t limbs);
void nttmul_rns_destroy(nttmul_rns *r);
const char *nttmul_rns_last_error(const nttmul_rns *r);
int nttmul_rns_get_info(const nttmul_rns *r, nttmul_rns_info *info);
/* q, psi, omega, ... of one limb, as nttmul_get_info of a plain context of (n, q_limb) */
int nttmul_rns_limb_info(const nttmul_rns *r, uint32_t limb, nttmul_info *info);

/* Device-resident operands of info.word_bits-wide words on HIP device `dev` (one of the
 * context's), enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE they wait for the
 * range check).  a, b, c, in, out: [batch][limbs][n]. */
int nttmul_rns_multiply_device(nttmul_rns *r, void *c, const void *a, const void *b, size_t batch,
                               int dev, void *stream);
int nttmul_rns_forward_device(nttmul_rns *r, void *out, const void *in, size_t batch, int dev,
                              void *stream);
int nttmul_rns_inverse_device(nttmul_rns *r, void *out, const void *in, size_t batch, int dev,
                              void *stream);
int nttmul_rns_mac_ntt_device(nttmul_rns *r, void *c, const void *a, const void *b_hat,
                              size_t batch, uint32_t terms, int shared, int dev, void *stream);

/* Host buffers.  Deliberately simple, as nttmul_mac_ntt_u32 / _u64: the context's first device,
 * device buffers owned by the call, the device path, a copy back and a synchronise. */
int nttmul_rns_multiply(nttmul_rns *r, void *c, const void *a, const void *b, size_t batch);
int nttmul_rns_forward(nttmul_rns *r, void *out, const void *in, size_t batch);
int nttmul_rns_inverse(nttmul_rns *r, void *out, const void *in, size_t batch);
int nttmul_rns_mac_ntt(nttmul_rns *r, void *c, const void *a, const void *b_hat, size_t batch,
                       uint32_t terms, int shared);

/* The kernel an operation dispatches to (op: 0 multiply, 1 forward, 2 inverse, 3 mac), in the
 * format of nttmul_kernel_name, e.g. "k_rns_rows<Arith32P3,u32,12>", "k_rns_xform<Arith64,u64,10,1>"
 * (the last argument: 0 forward, 1 inverse), "k_rns_mac<Arith32P,u32,8>".  Returns the untruncated
 * length, or a negative status. */
int nttmul_rns_kernel_name(const nttmul_rns *r, int op, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_RNS_H */
