/*
 * nttmul_tmd.h — BGV's plaintext-preserving ModDown and rescale on NTT-domain limbs:
 * lib/libnttmul_tmd.so (not libnttmul_ctlin.so, nor any of the older libraries).
 *
 * libnttmul_tmd.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h, nttmul_rns.h,
 * nttmul_bconv.h, nttmul_rnsmp.h, nttmul_galois.h, nttmul_ks.h, nttmul_macn.h, nttmul_hoist.h,
 * nttmul_mdntt.h, nttmul_ksntt.h, nttmul_lintrans.h, nttmul_ctmul.h, nttmul_xconv.h,
 * nttmul_level.h and nttmul_ctlin.h with the same kernels, plus the entry points below and the
 * kernels behind them (csrc/tmd_dev.hpp k_tmd_*).
 *
 * An nttmul_tmd context holds, for one power-of-two n in 256 .. 65536, the basis
 * Q = (q_0 .. q_{L-1}), the basis P = (p_0 .. p_{K-1}), disjoint from Q and of the same word
 * class, and a plaintext modulus t.  The extended basis is ordered Q, then P (as nttmul_mdntt.h).
 * Write Ph_j = P / p_j.  Every limb of the input is a transform: bit-reversed NTT order, canonical
 * words, what nttmul_rns_forward / nttmul_rnsmp_forward write for that limb's modulus.  So is
 * every limb of the output.  The moduli of a context may be of any sizes within their word class
 * and in any order (tests/test_gpu_tmd_bases.py).
 *
 * Why.  In BGV the message sits in the low bits, c_0 + c_1 s = m + t e (mod Q).  Every other
 * division by P here subtracts a multiple of P that is only congruent to X modulo P
 * (nttmul_mdntt_moddown the uncorrected sum S, nttmul_xconv_moddown the centred c), and a
 * subtrahend that is not 0 modulo t destroys m.  This one subtracts d with d = X (mod P) and
 * d = 0 (mod t).
 *
 *   moddown  x_hat [batch][L + K][n] -> out [batch][L][n].  For the CRT value X of the input over
 *            Q u P, per coefficient:
 *              y_j  = [X]_{p_j} (Ph_j^-1 mod p_j) mod p_j
 *              S    = sum over j of y_j Ph_j      = [X]_P + alpha P, 0 <= alpha < K: an exact integer
 *              v    = (-S P^-1) mod t             = sum over j of y_j g_j mod t, g_j = (-p_j^-1) mod t
 *              u    = v if v <= (t - 1) / 2 else v - t         the centred representative
 *              d    = S + u P
 *              out[p][l] = NTT_{q_l}((X - d) / P mod q_l)
 *            Per limb that is (x_hat[p][l] - NTT_{q_l}(r_l)) (P^-1 mod q_l) with
 *            r_l = sum_j y_j (Ph_j mod q_l) + u (P mod q_l): nttmul_mdntt_moddown's chain with one
 *            more product in the sum, and out = nttmul_mdntt_moddown(x_hat) - NTT_{q_l}(u mod q_l),
 *            bit for bit.
 *
 * Consequences.
 *   - P out = X (mod t): the message is multiplied by P^-1 mod t.  That factor is
 *     nttmul_tmd_info.msg_factor; the caller tracks it (it accumulates as a product over the
 *     calls a ciphertext went through), or picks every p_j = 1 (mod t), where it is 1.
 *   - |X / P - out| <= K + (t + 1) / 2 per coefficient: what the floor form costs (K) plus the
 *     correction's (t - 1) / 2, where a centred d would give (1 + t) / 2.  Everything is integer
 *     arithmetic: there is no guard band, and the result is exact for every input.
 *   - K = 1 with P = {the last prime} is the BGV rescale from level L + 1 to level L.
 *   - The merged context of INTEGRATION.md section 2k works as before: q[:L-1] and
 *     (q_{L-1},) + p.
 *
 * The plaintext modulus.  t is odd, t >= 3, t < 2^31 on 32-bit words and t < 2^62 on 64-bit
 * words (the target-modulus range of the conversion sum's accumulator, csrc/tmd_dev.hpp), and
 * no p_j or q_l divides it.  t need not be prime.
 *
 * Word size, as nttmul_rns.h: every modulus of both bases below 2^31 (32-bit words) or every one
 * in [2^32, 2^62) (64-bit words); nttmul_tmd_info.word_bits says which.
 *
 * Status, all decided before any device access, in this order: nttmul_mdntt_create's, in its
 * order; NTTMUL_EINVAL for t < 3; NTTMUL_EUNSUPPORTED for an even t; NTTMUL_EINVAL for t at or
 * above the class bound; NTTMUL_EINVAL for a t that is 0 modulo some p_j or q_l.  A call returns
 * NTTMUL_EINVAL for a NULL context or a NULL operand with batch > 0; batch = 0 is a successful
 * no-op.  NTTMUL_ENODEV as in nttmul.h (no device, or `dev` not one of the context's).
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_tmd_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  out must not overlap x_hat.
 *   Footprint.  A call writes exactly batch * L * n words of out and nothing else in caller
 *     memory; x_hat is never written.
 *   Addressing.  Every offset is computed in 64 bits: batch * (L + K) * n may pass 2^32 words.
 *
 * Scratch, as nttmul_mdntt.h: the intermediates (the K coefficient-order limbs y, and above
 * n = 4096 the column-passed sums as well) live in a scratch the context owns per device, bounded
 * by params->scratch_mb (0: 512) per buffer: a larger batch runs as sub-batches of whole
 * polynomials on the same stream, never less than one polynomial.  Uses of the scratch are ordered
 * by an event whatever stream they were enqueued on; a context serves one host thread at a time.
 * NTTMUL_FLAG_VALIDATE range-checks x_hat over its L + K limbs on the device first (the
 * k_rns_check_range of nttmul_rns.h) and returns NTTMUL_ERANGE without touching out; the call
 * then waits for the check.  nttmul_tmd_destroy waits for the last use of the scratch, not for
 * the streams passed to the *_device calls: synchronise them first.
 *
 * Out of scope here:
 *   - an even t (the Montgomery reduction of the mod-t sum needs an odd modulus, and the centred
 *     representative a tie rule);
 *   - the centred variant, d built on nttmul_xconv.h's c instead of S (a rounding term of
 *     (1 + t) / 2 instead of K + (t + 1) / 2, for a guard band and doubles in the kernel);
 *   - a coefficient-order input or output;
 *   - u computed once per coefficient in a pass of its own (each of the L target-limb workgroups
 *     recomputes it; tools/bench_tmd.py measures what that costs);
 *   - cyclic contexts (NTTMUL_FLAG_CYCLIC), the class 2^31 <= q < 2^32;
 *   - a chunked or multi-device host path (the host form below is deliberately simple);
 *   - a bench.py mode (tools/bench_tmd.py measures this call).
 */
#ifndef NTTMUL_TMD_H
#define NTTMUL_TMD_H

#include "nttmul_ctlin.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nttmul_tmd nttmul_tmd;

typedef struct {
  uint32_t n, logn, q_limbs, p_limbs;
  uint32_t word_bits;  /* 32: every modulus < 2^31; 64: every modulus >= 2^32.  The word of every operand */
  int ndev;
  uint32_t scratch_mb; /* the bound of one scratch buffer, in MiB */
  uint64_t t;          /* the plaintext modulus */
  uint64_t msg_factor; /* P^-1 mod t: P out = X (mod t) */
} nttmul_tmd_info;

/* params: n, ndev, first_dev, flags and scratch_mb as for nttmul_mdntt_create (params_size
 * likewise); params->q and params->psi must be 0; the dispatch knobs are ignored.
 * q[0 .. q_limbs) and p[0 .. p_limbs): the two bases, in limb order.  t: the plaintext modulus. */
int nttmul_tmd_create(nttmul_tmd **m, const nttmul_params *params, size_t params_size,
                      const uint64_t *q, uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs,
                      uint64_t t);
void nttmul_tmd_destroy(nttmul_tmd *m);
const char *nttmul_tmd_last_error(const nttmul_tmd *m);
int nttmul_tmd_get_info(const nttmul_tmd *m, nttmul_tmd_info *info);

/* Device-resident operands of info.word_bits-wide words on HIP device `dev` (one of the
 * context's), enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE it waits for the
 * range check).  x_hat [batch][L + K][n] -> out [batch][L][n]. */
int nttmul_tmd_moddown_device(nttmul_tmd *m, void *out, const void *x_hat, size_t batch, int dev,
                              void *stream);

/* Host buffers.  Deliberately simple, as nttmul_mdntt_moddown: the context's first device, device
 * buffers owned by the call, the device path, a copy back and a synchronise. */
int nttmul_tmd_moddown(nttmul_tmd *m, void *out, const void *x_hat, size_t batch);

/* Host-only, no device: the plain constants of (q, p, t), each output optional (NULL skips it).
 * yscale [K]: Ph_j^-1 mod p_j.  g [K]: -p_j^-1 mod t.  w [K + 2][L]: Ph_j mod q_l, in row K
 * P mod q_l and in row K + 1 -P mod q_l.  v [L]: P^-1 mod q_l.  msg_factor: P^-1 mod t.
 * Returns the status nttmul_tmd_create would return before any device access. */
int nttmul_tmd_plan(const nttmul_params *params, size_t params_size, const uint64_t *q,
                    uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs, uint64_t t,
                    uint64_t *yscale, uint64_t *g, uint64_t *w, uint64_t *v,
                    uint64_t *msg_factor);

/* The kernels a sub-batch launches, joined by " + ", in the format of nttmul_mdntt_kernel_name:
 * "k_mdntt_inv<Arith32P,u32,12> + k_tmd_fwd<Arith32P,u32,12>", or above n = 4096
 * "k_mdntt_inv_rows<Arith64,u64,1> + k_rnsmp_cols_inv<Arith64,u64,1> +
 * k_tmd_cols_fwd<Arith64,u64,1> + k_mdntt_rows<Arith64,u64,1>".  Returns the untruncated length,
 * or a negative status. */
int nttmul_tmd_kernel_name(const nttmul_tmd *m, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_TMD_H */
