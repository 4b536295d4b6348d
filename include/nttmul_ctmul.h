/*
 * nttmul_ctmul.h — the product of two ciphertexts on NTT-domain limbs: the tensor terms and the
 * relinearisation, formed in Q u P before ModDown: lib/libnttmul_ctmul.so (not
 * libnttmul_lintrans.so, nor any of the older libraries).
 *
 * libnttmul_ctmul.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h, nttmul_rns.h,
 * nttmul_bconv.h, nttmul_rnsmp.h, nttmul_galois.h, nttmul_ks.h, nttmul_macn.h, nttmul_hoist.h,
 * nttmul_mdntt.h, nttmul_ksntt.h and nttmul_lintrans.h with the same kernels, plus the entry points
 * below and the kernels behind them (csrc/ctmul_dev.hpp k_ctmul_high, k_ctmul_relin).
 *
 * An nttmul_ctmul context holds, for one power-of-two n in 256 .. 65536, the basis
 * Q = (q_0 .. q_{L-1}) and the special basis P = (p_0 .. p_{K-1}), disjoint from Q and of the same
 * word class.  The extended basis is ordered Q, then P, M = L + K limbs m_0 .. m_{M-1}.  Every
 * limb of every operand is a transform: bit-reversed NTT order, canonical words, what
 * nttmul_rns_forward / nttmul_rnsmp_forward write for that limb's modulus.  The context needs no
 * twiddles, no digit width and no scratch.
 * The moduli of a context may be of any sizes within their word class and in any order
 * (tests/test_gpu_bases.py).
 *
 * A ciphertext is its two components over Q, [2][L][n]; x_hat and y_hat hold `pairs` of them per
 * batch entry, [batch][pairs][2][L][n].  pairs = 1 is the plain product; pairs > 1 is a dot
 * product of ciphertexts, sum over s of x_s (x) y_s, which pays for one relinearisation.
 * y_hat == x_hat (the same pointer) is the square.
 *
 *   high   x_hat, y_hat [batch][pairs][2][L][n]
 *       -> d2_hat [batch][L][n]
 *
 *            d2_hat[p][l][j] = (sum over s of x_hat[p][s][1][l][j] y_hat[p][s][1][l][j]) mod q_l
 *
 *          the s^2 term of the product, nttmul_ksntt_modup's x_hat as it stands.
 *
 *   relin  up_hat  [batch][terms][M][n]   the raised digits of d2_hat (nttmul_ksntt_modup's up_hat)
 *          key_hat [2][terms][M][n]       the relinearisation key (s^2 -> s), b then a, shared by
 *                                         the batch
 *          x_hat, y_hat                   as above
 *       -> c_hat   [batch][2][M][n]
 *
 *            c_hat[p][i][l][j] = (sum over t of up_hat[p][t][l][j] key_hat[i][t][l][j]
 *                                 + [l < L] (P mod q_l) e_i[p][l][j]) mod m_l
 *            e_0 = sum over s of x[s][0] y[s][0]
 *            e_1 = sum over s of (x[s][0] y[s][1] + x[s][1] y[s][0])
 *
 *          the key switch of d2 plus P (d0, d1): P x is 0 in the limbs of P and becomes x again
 *          under ModDown.  One nttmul_mdntt_moddown over batch 2 polynomials of c_hat returns the
 *          relinearised product (c_0', c_1') over Q in NTT order.  The nttmul_mdntt context built
 *          on (q_0 .. q_{L-2}) and (q_{L-1}, p_0 .. p_{K-1}) reads the same [M] limb order and
 *          divides by P q_{L-1} instead: the product rescaled, over L - 1 limbs.  Multiply,
 *          relinearise and rescale are then high, nttmul_ksntt_modup, relin and one ModDown:
 *          1 + 2 + 1 + 2 launches at n <= 4096 and 1 + 4 + 1 + 4 above, with no coefficient-order
 *          intermediate in caller memory.
 *
 * Outputs are canonical; a modular sum of exact products is exact, so the definitions pin every
 * word.  Each operation is one element-wise launch at every n, no transform and no scratch.  Both
 * x_hat and y_hat are required: the form without a tensor term is nttmul_lintrans_apply with
 * k = {1}.
 *
 * Word size, as nttmul_rns.h: every modulus of both bases below 2^31 (32-bit words) or every one
 * in [2^32, 2^62) (64-bit words); nttmul_ctmul_info.word_bits says which.
 *
 * Status, all decided before any device access.  nttmul_ctmul_create: nttmul_lintrans_create's,
 * in the same order.  NTTMUL_EINVAL: for each basis a NULL argument, limbs of 0 or above
 * NTTMUL_RNS_MAX_LIMBS, an n that is not a power of two or below 256, a modulus that is not prime,
 * not 1 mod 2n or >= 2^62, non-zero params->q or params->psi, a prime that occurs twice, within a
 * basis or in both; then q_limbs + p_limbs > NTTMUL_RNS_MAX_LIMBS.  NTTMUL_EUNSUPPORTED:
 * n > 65536, NTTMUL_FLAG_CYCLIC, a modulus in [2^31, 2^32), mixed classes within or across Q and
 * P, and a basis nttmul_rns_create would refuse at that degree.  The calls, in this order:
 * NTTMUL_EINVAL for a NULL context; pairs = 0; terms = 0 (relin); a NULL operand with batch > 0
 * (high: d2_hat, x_hat, y_hat; relin: c_hat, up_hat, key_hat, x_hat, y_hat).  batch = 0 is then a
 * successful no-op.  NTTMUL_ENODEV as in nttmul.h (no device, or `dev` not one of the context's).
 * NTTMUL_FLAG_VALIDATE range-checks every operand over its limbs on the device first (the
 * k_rns_check_range of nttmul_rns.h; y_hat == x_hat is checked once) and returns NTTMUL_ERANGE
 * without touching the output; the call then waits for the check.
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_ctmul_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  The output must overlap no input.  Inputs may alias each other.
 *   Footprint.  high writes exactly batch * L * n words of d2_hat, relin exactly
 *     batch * 2 * M * n words of c_hat, and nothing else in caller memory; the inputs are never
 *     written.
 *   Addressing.  Every offset is computed in 64 bits: batch * terms * M * n and
 *     batch * pairs * 2 * L * n may pass 2^32 words.
 *
 * Out of scope here:
 *   - high fused into the loads of nttmul_ksntt_modup's inverse kernels;
 *   - a key, or a plaintext operand, per batch entry;
 *   - ciphertext x plaintext, ciphertext sums and constants (no key): nttmul_ctlin.h,
 *     lib/libnttmul_ctlin.so, nttmul_ctlin_combine;
 *   - three-component ciphertexts: their sums are nttmul_ctlin.h's combine with comps = 3 and
 *     all three terms of a product its tensor; as inputs of a product they stay out of scope;
 *   - rounding in ModDown, and exact conversion (the alpha correction): both are nttmul_xconv.h,
 *     lib/libnttmul_xconv.so, whose moddown reads what this header's calls write;
 *   - cyclic contexts (NTTMUL_FLAG_CYCLIC), the class 2^31 <= q < 2^32;
 *   - a chunked or multi-device host path (the host forms below are deliberately simple);
 *   - a bench.py mode (tools/bench_ctmul.py measures these calls).
 */
#ifndef NTTMUL_CTMUL_H
#define NTTMUL_CTMUL_H

#include "nttmul_lintrans.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nttmul_ctmul nttmul_ctmul;

typedef struct {
  uint32_t n, logn, q_limbs, p_limbs;
  uint32_t word_bits;  /* 32: every modulus < 2^31; 64: every modulus >= 2^32.  The word of every operand */
  int ndev;
} nttmul_ctmul_info;

#define NTTMUL_CTMUL_HIGH 0
#define NTTMUL_CTMUL_RELIN 1

/* params: n, ndev, first_dev and flags as for nttmul_lintrans_create (params_size likewise);
 * params->q and params->psi must be 0; scratch_mb and the dispatch knobs are ignored.
 * q[0 .. q_limbs) and p[0 .. p_limbs): the two bases, in limb order. */
int nttmul_ctmul_create(nttmul_ctmul **ct, const nttmul_params *params, size_t params_size,
                        const uint64_t *q, uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs);
void nttmul_ctmul_destroy(nttmul_ctmul *ct);
const char *nttmul_ctmul_last_error(const nttmul_ctmul *ct);
int nttmul_ctmul_get_info(const nttmul_ctmul *ct, nttmul_ctmul_info *info);

/* Device-resident operands of info.word_bits-wide words on HIP device `dev` (one of the
 * context's), enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE they wait for the
 * range check). */
int nttmul_ctmul_high_device(nttmul_ctmul *ct, void *d2_hat, const void *x_hat, const void *y_hat,
                             size_t batch, uint32_t pairs, int dev, void *stream);
int nttmul_ctmul_relin_device(nttmul_ctmul *ct, void *c_hat, const void *up_hat,
                              const void *key_hat, const void *x_hat, const void *y_hat,
                              size_t batch, uint32_t pairs, uint32_t terms, int dev, void *stream);

/* Host buffers.  Deliberately simple, as nttmul_lintrans_apply: the context's first device, device
 * buffers owned by the call, the device path, a copy back and a synchronise. */
int nttmul_ctmul_high(nttmul_ctmul *ct, void *d2_hat, const void *x_hat, const void *y_hat,
                      size_t batch, uint32_t pairs);
int nttmul_ctmul_relin(nttmul_ctmul *ct, void *c_hat, const void *up_hat, const void *key_hat,
                       const void *x_hat, const void *y_hat, size_t batch, uint32_t pairs,
                       uint32_t terms);

/* The kernel `op` (NTTMUL_CTMUL_HIGH or NTTMUL_CTMUL_RELIN) launches, in the format of
 * nttmul_lintrans_kernel_name: "k_ctmul_relin<Arith64,u64>".  Returns the untruncated length, or a
 * negative status (NTTMUL_EINVAL for another op). */
int nttmul_ctmul_kernel_name(const nttmul_ctmul *ct, int op, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_CTMUL_H */
