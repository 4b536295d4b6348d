/*
 * nttmul_mdntt.h — ModDown and rescale on NTT-domain limbs: lib/libnttmul_mdntt.so (not
 * libnttmul_hoist.so, nor any of the older libraries).
 *
 * libnttmul_mdntt.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h, nttmul_rns.h,
 * nttmul_bconv.h, nttmul_rnsmp.h, nttmul_galois.h, nttmul_ks.h, nttmul_macn.h and nttmul_hoist.h
 * with the same kernels, plus the entry points below and the kernels behind them
 * (csrc/mdntt_dev.hpp k_mdntt_*).
 *
 * An nttmul_mdntt context holds, for one power-of-two n in 256 .. 65536, the basis
 * Q = (q_0 .. q_{L-1}) and the special basis P = (p_0 .. p_{K-1}), disjoint from Q and of the
 * same word class.  The extended basis is ordered Q, then P (as nttmul_ks.h).  Write
 * Ph_j = P / p_j.  Every limb of the input is a transform: bit-reversed NTT order, canonical
 * words, what nttmul_rns_forward / nttmul_rnsmp_forward write for that limb's modulus.  So is
 * every limb of the output.
 * The moduli of a context may be of any sizes within their word class and in any order
 * (tests/test_gpu_bases.py).
 *
 *   moddown  x_hat [batch][L + K][n] -> out [batch][L][n]
 *              y_j       = INTT_{p_j}(x_hat[p][L + j]) (Ph_j^-1 mod p_j) mod p_j     coefficient order
 *              r_l[k]    = (sum over j of y_j[k] Ph_j) mod q_l       the unreduced-alpha conversion
 *              out[p][l] = (x_hat[p][l] - NTT_{q_l}(r_l)) (P^-1 mod q_l) mod q_l
 *
 * out equals nttmul_rns(mp)_forward over Q of nttmul_ks_moddown of nttmul_rns(mp)_inverse over
 * Q u P of x_hat, bit for bit: the subtraction and the factor P^-1 are linear and per limb, so
 * they commute with the forward transform, and both results are the canonical residue of one
 * integer.  Only the K special limbs are transformed back: L + K transforms instead of 2L + K,
 * and two launches (n <= 4096) or four (n > 4096) instead of three or five.
 *
 * K = 1 with P = {the last prime} is the CKKS rescale from level L + 1 to level L in its floor
 * form, and it is exact: out = NTT(floor(X / p) mod q_l) for the CRT value X of the input over
 * Q u {p}.  It is not BGV's: the subtrahend [X]_p is not 0 modulo the plaintext modulus, so the
 * message in the low bits does not survive it (nttmul_tmd.h, lib/libnttmul_tmd.so, has BGV's
 * ModDown and rescale on the same operands).
 *
 * Word size, as nttmul_rns.h: every modulus of both bases below 2^31 (32-bit words) or every one
 * in [2^32, 2^62) (64-bit words); nttmul_mdntt_info.word_bits says which.
 *
 * Status, all decided before any device access: nttmul_ks_create's without the digit width, in
 * the same order.  NTTMUL_EINVAL: for each basis a NULL argument, limbs of 0 or above
 * NTTMUL_RNS_MAX_LIMBS, an n that is not a power of two or below 256, a modulus that is not
 * prime, not 1 mod 2n or >= 2^62, non-zero params->q or params->psi, a prime that occurs twice,
 * within a basis or in both; then q_limbs + p_limbs > NTTMUL_RNS_MAX_LIMBS.
 * NTTMUL_EUNSUPPORTED: n > 65536, NTTMUL_FLAG_CYCLIC, a modulus in [2^31, 2^32), mixed classes
 * within or across Q and P, and a basis nttmul_rns_create would refuse at that degree.  A call
 * returns NTTMUL_EINVAL for a NULL context or a NULL operand with batch > 0; batch = 0 is a
 * successful no-op.  NTTMUL_ENODEV as in nttmul.h (no device, or `dev` not one of the context's).
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_mdntt_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  out must not overlap x_hat.
 *   Footprint.  The call writes exactly batch * L * n words of out and nothing else in caller
 *     memory; x_hat is never written.
 *   Addressing.  Every offset is computed in 64 bits: batch * (L + K) * n may pass 2^32 words.
 *
 * Scratch, as nttmul_rnsmp.h: the intermediates (the K coefficient-order limbs y, and above
 * n = 4096 the column-passed r as well) live in a scratch the context owns per device, bounded by
 * params->scratch_mb (0: 512) per buffer: a larger batch runs as sub-batches of whole polynomials
 * on the same stream, never less than one polynomial.  Uses of the scratch are ordered by an
 * event whatever stream they were enqueued on; a context serves one host thread at a time.
 * NTTMUL_FLAG_VALIDATE range-checks x_hat over its L + K limbs on the device first (the
 * k_rns_check_range of nttmul_rns.h) and returns NTTMUL_ERANGE without touching out; the call
 * then waits for the check.  nttmul_mdntt_destroy waits for the last use of the scratch, not for
 * the streams passed to the *_device calls: synchronise them first.
 *
 * Out of scope here:
 *   - rounding instead of flooring (nttmul_xconv.h, lib/libnttmul_xconv.so, has the rounded
 *     ModDown on the same operands);
 *   - a P part in coefficient order, or a coefficient-order output;
 *   - NTT-domain output of nttmul_*_macn_ntt / nttmul_*_hoist_ntt (nttmul_ksntt.h,
 *     lib/libnttmul_ksntt.so, has the hoisted mac with NTT-domain output and the ModUp in front of
 *     it, so that the whole key switch ends here);
 *   - exact conversion (the alpha correction: nttmul_xconv.h as well);
 *   - cyclic contexts (NTTMUL_FLAG_CYCLIC), the class 2^31 <= q < 2^32;
 *   - a chunked or multi-device host path (the host form below is deliberately simple);
 *   - a bench.py mode (tools/bench_mdntt.py measures this call).
 */
#ifndef NTTMUL_MDNTT_H
#define NTTMUL_MDNTT_H

#include "nttmul_hoist.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nttmul_mdntt nttmul_mdntt;

typedef struct {
  uint32_t n, logn, q_limbs, p_limbs;
  uint32_t word_bits;  /* 32: every modulus < 2^31; 64: every modulus >= 2^32.  The word of every operand */
  int ndev;
  uint32_t scratch_mb; /* the bound of one scratch buffer, in MiB */
} nttmul_mdntt_info;

/* params: n, ndev, first_dev, flags and scratch_mb as for nttmul_rnsmp_create (params_size
 * likewise); params->q and params->psi must be 0; the dispatch knobs are ignored.
 * q[0 .. q_limbs) and p[0 .. p_limbs): the two bases, in limb order. */
int nttmul_mdntt_create(nttmul_mdntt **m, const nttmul_params *params, size_t params_size,
                        const uint64_t *q, uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs);
void nttmul_mdntt_destroy(nttmul_mdntt *m);
const char *nttmul_mdntt_last_error(const nttmul_mdntt *m);
int nttmul_mdntt_get_info(const nttmul_mdntt *m, nttmul_mdntt_info *info);

/* Device-resident operands of info.word_bits-wide words on HIP device `dev` (one of the
 * context's), enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE it waits for the
 * range check).  x_hat [batch][L + K][n] -> out [batch][L][n]. */
int nttmul_mdntt_moddown_device(nttmul_mdntt *m, void *out, const void *x_hat, size_t batch,
                                int dev, void *stream);

/* Host buffers.  Deliberately simple, as nttmul_ks_*: the context's first device, device buffers
 * owned by the call, the device path, a copy back and a synchronise. */
int nttmul_mdntt_moddown(nttmul_mdntt *m, void *out, const void *x_hat, size_t batch);

/* The kernels a sub-batch launches, joined by " + ", in the format of nttmul_rnsmp_kernel_name:
 * "k_mdntt_inv<Arith32P,u32,12> + k_mdntt_fwd<Arith32P,u32,12>", or above n = 4096
 * "k_mdntt_inv_rows<Arith64,u64,1> + k_rnsmp_cols_inv<Arith64,u64,1> +
 * k_mdntt_cols_fwd<Arith64,u64,1> + k_mdntt_rows<Arith64,u64,1>".  Returns the untruncated
 * length, or a negative status. */
int nttmul_mdntt_kernel_name(const nttmul_mdntt *m, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_MDNTT_H */
