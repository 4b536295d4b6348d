/*
 * nttmul_lintrans.h — the weighted sum of rotations of a hybrid key switch, formed in Q u P before
 * ModDown: lib/libnttmul_lintrans.so (not libnttmul_ksntt.so, nor any of the older libraries).
 *
 * libnttmul_lintrans.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h, nttmul_rns.h,
 * nttmul_bconv.h, nttmul_rnsmp.h, nttmul_galois.h, nttmul_ks.h, nttmul_macn.h, nttmul_hoist.h,
 * nttmul_mdntt.h and nttmul_ksntt.h with the same kernels, plus the entry points below and the
 * kernel behind them (csrc/lintrans_dev.hpp k_lintrans).
 *
 * An nttmul_lintrans context holds, for one power-of-two n in 256 .. 65536, the basis
 * Q = (q_0 .. q_{L-1}) and the special basis P = (p_0 .. p_{K-1}), disjoint from Q and of the same
 * word class.  The extended basis is ordered Q, then P, M = L + K limbs m_0 .. m_{M-1}.  Every
 * limb of every operand is a transform: bit-reversed NTT order, canonical words, what
 * nttmul_rns_forward / nttmul_rnsmp_forward write for that limb's modulus.  The context needs no
 * twiddles and no digit width.
 * The moduli of a context may be of any sizes within their word class and in any order
 * (tests/test_gpu_bases.py).
 *
 *   apply  a_hat  [batch][terms][M][n]         the raised digits (nttmul_ksntt_modup's up_hat)
 *          b_hat  [rots][comps][terms][M][n]   the keys, shared by the batch (nttmul_ksntt_mac's)
 *          k      [rots]                       host memory, odd, 0 < k < 2n
 *          w_hat  [rots][M][n] or NULL         the diagonals over Q u P, shared by the batch
 *          c0_hat [batch][L][n] or NULL        the ciphertext's c_0 part over Q
 *       -> c_hat  [batch][comps][M][n]
 *
 *            c_hat[p][i][l][j] = (sum over r of w_hat[r][l][j] (sum over t of
 *                                    a_hat[p][t][l][src_{k_r}(j)] b_hat[r][i][t][l][j]
 *                                  + [i = 0 and l < L] (P mod q_l) c0_hat[p][l][src_{k_r}(j)])) mod m_l
 *
 *          with src_k the slot permutation of nttmul_galois_ntt.  w_hat = NULL: every weight is 1,
 *          the plain rotate-and-sum.  c0_hat = NULL: that term is dropped.  The c_0 term is the
 *          usual trick: P x is 0 in the limbs of P and becomes x again under ModDown.  With c0_hat
 *          given, one nttmul_mdntt_moddown over batch comps polynomials of c_hat returns the whole
 *          linear transform (c_0', c_1') over Q in NTT order: one ModDown for any number of
 *          rotations, where nttmul_ksntt_mac leaves batch rots comps polynomials to it.  Outputs
 *          are canonical; a modular sum of exact products is exact, so the definition pins every
 *          word.  One element-wise launch at every n, no transform and no scratch.
 *
 *          The identity rotation of a diagonal product needs no key: the caller adds
 *          diag_0 o (c_0, c_1) to the ModDown output in Q afterwards (k = 1 with a key also works
 *          and costs a term).
 *
 * Word size, as nttmul_rns.h: every modulus of both bases below 2^31 (32-bit words) or every one
 * in [2^32, 2^62) (64-bit words); nttmul_lintrans_info.word_bits says which.
 *
 * Status, all decided before any device access.  nttmul_lintrans_create: nttmul_ksntt_create's,
 * in the same order, without the digit width's.  NTTMUL_EINVAL: for each basis a NULL argument,
 * limbs of 0 or above NTTMUL_RNS_MAX_LIMBS, an n that is not a power of two or below 256, a
 * modulus that is not prime, not 1 mod 2n or >= 2^62, non-zero params->q or params->psi, a prime
 * that occurs twice, within a basis or in both; then q_limbs + p_limbs > NTTMUL_RNS_MAX_LIMBS.
 * NTTMUL_EUNSUPPORTED: n > 65536, NTTMUL_FLAG_CYCLIC, a modulus in [2^31, 2^32), mixed classes
 * within or across Q and P, and a basis nttmul_rns_create would refuse at that degree.  apply's
 * statuses are nttmul_ksntt_mac_device's, in its order: NTTMUL_EINVAL for a NULL context;
 * terms = 0; comps = 0 or comps > NTTMUL_MACN_MAX_COMPS; rots = 0 or rots > NTTMUL_HOIST_MAX_ROTS;
 * a NULL k; an even k[r], k[r] = 0 or k[r] >= 2n for an r < rots; a NULL c_hat, a_hat or b_hat
 * with batch > 0.  w_hat and c0_hat may be NULL, with the meaning above.  batch = 0 is then a
 * successful no-op.  NTTMUL_ENODEV as in nttmul.h (no device, or `dev` not one of the context's).
 * NTTMUL_FLAG_VALIDATE range-checks every operand that is given over its limbs on the device first
 * (the k_rns_check_range of nttmul_rns.h) and returns NTTMUL_ERANGE without touching the output;
 * the call then waits for the check.
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_lintrans_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  The output must overlap no input.
 *   Footprint.  apply writes exactly batch * comps * M * n words of c_hat and nothing else in
 *     caller memory; the inputs are never written.
 *   Addressing.  Every offset is computed in 64 bits: batch * terms * M * n may pass 2^32 words.
 *
 * Out of scope here:
 *   - a b_hat or a w_hat per batch entry;
 *   - more than NTTMUL_MACN_MAX_COMPS components;
 *   - BSGS giant steps: a second apply over the first's ModDown output, nothing new;
 *   - rounding in ModDown, and exact conversion (the alpha correction): both are nttmul_xconv.h,
 *     lib/libnttmul_xconv.so, whose moddown reads what this header's calls write;
 *   - cyclic contexts (NTTMUL_FLAG_CYCLIC), the class 2^31 <= q < 2^32;
 *   - a chunked or multi-device host path (the host form below is deliberately simple);
 *   - a bench.py mode (tools/bench_lintrans.py measures this call).
 */
#ifndef NTTMUL_LINTRANS_H
#define NTTMUL_LINTRANS_H

#include "nttmul_ksntt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nttmul_lintrans nttmul_lintrans;

typedef struct {
  uint32_t n, logn, q_limbs, p_limbs;
  uint32_t word_bits;  /* 32: every modulus < 2^31; 64: every modulus >= 2^32.  The word of every operand */
  int ndev;
} nttmul_lintrans_info;

/* params: n, ndev, first_dev and flags as for nttmul_ksntt_create (params_size likewise);
 * params->q and params->psi must be 0; scratch_mb and the dispatch knobs are ignored.
 * q[0 .. q_limbs) and p[0 .. p_limbs): the two bases, in limb order. */
int nttmul_lintrans_create(nttmul_lintrans **lt, const nttmul_params *params, size_t params_size,
                           const uint64_t *q, uint32_t q_limbs, const uint64_t *p,
                           uint32_t p_limbs);
void nttmul_lintrans_destroy(nttmul_lintrans *lt);
const char *nttmul_lintrans_last_error(const nttmul_lintrans *lt);
int nttmul_lintrans_get_info(const nttmul_lintrans *lt, nttmul_lintrans_info *info);

/* Device-resident operands of info.word_bits-wide words on HIP device `dev` (one of the
 * context's), enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE it waits for the range
 * check).  w_hat and c0_hat may be NULL. */
int nttmul_lintrans_apply_device(nttmul_lintrans *lt, void *c_hat, const void *a_hat,
                                 const void *b_hat, const void *w_hat, const void *c0_hat,
                                 const uint32_t *rot, uint32_t rots, size_t batch, uint32_t terms,
                                 uint32_t comps, int dev, void *stream);

/* Host buffers.  Deliberately simple, as nttmul_ksntt_mac: the context's first device, device
 * buffers owned by the call, the device path, a copy back and a synchronise. */
int nttmul_lintrans_apply(nttmul_lintrans *lt, void *c_hat, const void *a_hat, const void *b_hat,
                          const void *w_hat, const void *c0_hat, const uint32_t *rot,
                          uint32_t rots, size_t batch, uint32_t terms, uint32_t comps);

/* The kernel apply launches, in the format of nttmul_ksntt_kernel_name:
 * "k_lintrans<Arith64,u64,2,1>" (the last two arguments are comps and whether w_hat is given).
 * Returns the untruncated length, or a negative status (NTTMUL_EINVAL for comps outside 1 ..
 * NTTMUL_MACN_MAX_COMPS). */
int nttmul_lintrans_kernel_name(const nttmul_lintrans *lt, uint32_t comps, int weighted, char *buf,
                                size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_LINTRANS_H */
