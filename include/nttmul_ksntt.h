/*
 * nttmul_ksntt.h — ModUp and the key mac of a hybrid key switch on NTT-domain limbs:
 * lib/libnttmul_ksntt.so (not libnttmul_mdntt.so, nor any of the older libraries).
 *
 * libnttmul_ksntt.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h, nttmul_rns.h,
 * nttmul_bconv.h, nttmul_rnsmp.h, nttmul_galois.h, nttmul_ks.h, nttmul_macn.h, nttmul_hoist.h and
 * nttmul_mdntt.h with the same kernels, plus the entry points below and the kernels behind them
 * (csrc/ksntt_dev.hpp k_ksntt_*).
 *
 * An nttmul_ksntt context holds what an nttmul_ks context holds, for one power-of-two n in
 * 256 .. 65536: the basis Q = (q_0 .. q_{L-1}), the special basis P = (p_0 .. p_{K-1}), disjoint
 * from Q and of the same word class, and the digit width alpha = digit_limbs.  Digit d is
 * D_d = (q_{d alpha} .. q_{min((d + 1) alpha, L) - 1}), dnum = ceil(L / alpha) of them (the last
 * may be shorter); Dh_i = D_d / q_i for the limb i of digit d.  The extended basis is ordered Q,
 * then P, M = L + K limbs m_0 .. m_{M-1}.  Every limb of every operand is a transform:
 * bit-reversed NTT order, canonical words, what nttmul_rns_forward / nttmul_rnsmp_forward write
 * for that limb's modulus.
 * The moduli of a context may be of any sizes within their word class and in any order
 * (tests/test_gpu_bases.py).
 *
 *   modup  x_hat [batch][L][n] -> up_hat [batch][dnum][M][n]
 *            y_i             = INTT_{q_i}(x_hat[p][i]) (Dh_i^-1 mod q_i) mod q_i      coefficient order
 *            up_hat[p][d][m] = NTT_m((sum over i in D_d of y_i Dh_i) mod m)             m not in D_d
 *            up_hat[p][d][m] = x_hat[p][m]                                              m in D_d
 *          up_hat equals nttmul_rns(mp)_forward over Q u P of nttmul_ks_modup of
 *          nttmul_rns(mp)_inverse over Q of x_hat, bit for bit: on a digit's own limbs the
 *          conversion returns the coefficient-order limb itself, whose transform is the input.
 *          dnum (L + K) transforms (L inverse, dnum (L + K) - L forward: the own limbs are
 *          copies) instead of L + dnum (L + K), two launches
 *          (n <= 4096) or four (n > 4096) instead of three or five, and the raised digits never
 *          exist in coefficient order in caller memory.  It is the a_hat of the call below and of
 *          nttmul_*_hoist_ntt with terms = dnum.
 *
 *   mac    a_hat [batch][terms][M][n], b_hat [rots][comps][terms][M][n] shared by the batch,
 *          k [rots] in host memory -> c_hat [batch][rots][comps][M][n]
 *            c_hat[p][r][i][l][j] = (sum over t of a_hat[p][t][l][src_{k_r}(j)] b_hat[r][i][t][l][j]) mod m_l
 *          with src_k the slot permutation of nttmul_galois_ntt.  The hoisted mac of
 *          nttmul_hoist.h with its output left in the NTT domain: c_hat equals
 *          nttmul_rns(mp)_forward of nttmul_*_hoist_ntt's c, bit for bit.  One launch at every n
 *          and no transform.  k = {1} is the plain pointwise multiply-accumulate over RNS limbs.
 *          c_hat is what nttmul_mdntt_moddown_device reads with batch rots comps polynomials.
 *
 * Word size, as nttmul_rns.h: every modulus of both bases below 2^31 (32-bit words) or every one
 * in [2^32, 2^62) (64-bit words); nttmul_ksntt_info.word_bits says which.
 *
 * Status, all decided before any device access.  nttmul_ksntt_create: nttmul_ks_create's, in the
 * same order.  NTTMUL_EINVAL: for each basis a NULL argument, limbs of 0 or above
 * NTTMUL_RNS_MAX_LIMBS, an n that is not a power of two or below 256, a modulus that is not
 * prime, not 1 mod 2n or >= 2^62, non-zero params->q or params->psi, a prime that occurs twice,
 * within a basis or in both; then digit_limbs = 0 or > q_limbs, or q_limbs + p_limbs >
 * NTTMUL_RNS_MAX_LIMBS.  NTTMUL_EUNSUPPORTED: n > 65536, NTTMUL_FLAG_CYCLIC, a modulus in
 * [2^31, 2^32), mixed classes within or across Q and P, and a basis nttmul_rns_create would
 * refuse at that degree.  modup returns NTTMUL_EINVAL for a NULL context or a NULL operand with
 * batch > 0.  mac's statuses are nttmul_rns_hoist_ntt_device's, in its order: NTTMUL_EINVAL for a
 * NULL context; terms = 0; comps = 0 or comps > NTTMUL_MACN_MAX_COMPS; rots = 0 or rots >
 * NTTMUL_HOIST_MAX_ROTS; a NULL k; an even k[r], k[r] = 0 or k[r] >= 2n for an r < rots; a NULL
 * operand with batch > 0.  batch = 0 is then a successful no-op.  NTTMUL_ENODEV as in nttmul.h
 * (no device, or `dev` not one of the context's).
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_ksntt_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  The output must overlap no input.
 *   Footprint.  modup writes exactly batch * dnum * M * n words of up_hat, mac exactly
 *     batch * rots * comps * M * n words of c_hat, and nothing else in caller memory; the inputs
 *     are never written.  Above n = 4096 modup passes its column-passed sums through up_hat
 *     before the row pass overwrites them in place: every word of up_hat is final when the
 *     call's work completes, and none is meaningful before.
 *   Addressing.  Every offset is computed in 64 bits: batch * dnum * M * n may pass 2^32 words.
 *
 * Scratch (modup only; mac has none), as nttmul_mdntt.h: the L coefficient-order limbs y (above
 * n = 4096 also the inverse rows' output, as large) live in a scratch the context owns per
 * device, bounded by params->scratch_mb (0: 512) per buffer: a larger batch runs as sub-batches of
 * whole polynomials on the same stream, never less than one polynomial.  Uses of the scratch are
 * ordered by an event whatever stream they were enqueued on; a context serves one host thread at
 * a time.  NTTMUL_FLAG_VALIDATE range-checks x_hat over its L limbs, or a_hat and b_hat over
 * their M limbs, on the device first (the k_rns_check_range of nttmul_rns.h) and returns
 * NTTMUL_ERANGE without touching the output; the call then waits for the check.
 * nttmul_ksntt_destroy waits for the last use of the scratch, not for the streams passed to the
 * *_device calls: synchronise them first.
 *
 * Out of scope here:
 *   - rounding in ModDown, and exact conversion (the alpha correction): both are nttmul_xconv.h,
 *     lib/libnttmul_xconv.so, whose moddown reads what this header's calls write;
 *   - a b_hat per batch entry, or more than NTTMUL_MACN_MAX_COMPS components;
 *   - summing the rotations before ModDown (rotate-and-sum in Q u P): nttmul_lintrans.h's
 *     nttmul_lintrans_apply, in lib/libnttmul_lintrans.so;
 *   - cyclic contexts (NTTMUL_FLAG_CYCLIC), the class 2^31 <= q < 2^32;
 *   - a chunked or multi-device host path (the host forms below are deliberately simple);
 *   - a bench.py mode (tools/bench_ksntt.py measures these calls).
 */
#ifndef NTTMUL_KSNTT_H
#define NTTMUL_KSNTT_H

#include "nttmul_mdntt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nttmul_ksntt nttmul_ksntt;

typedef struct {
  uint32_t n, logn, q_limbs, p_limbs, digit_limbs, digits;
  uint32_t word_bits;  /* 32: every modulus < 2^31; 64: every modulus >= 2^32.  The word of every operand */
  int ndev;
  uint32_t scratch_mb; /* the bound of one scratch buffer, in MiB */
} nttmul_ksntt_info;

/* params: n, ndev, first_dev, flags and scratch_mb as for nttmul_mdntt_create (params_size
 * likewise); params->q and params->psi must be 0; the dispatch knobs are ignored.
 * q[0 .. q_limbs) and p[0 .. p_limbs): the two bases, in limb order; digit_limbs = alpha. */
int nttmul_ksntt_create(nttmul_ksntt **k, const nttmul_params *params, size_t params_size,
                        const uint64_t *q, uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs,
                        uint32_t digit_limbs);
void nttmul_ksntt_destroy(nttmul_ksntt *k);
const char *nttmul_ksntt_last_error(const nttmul_ksntt *k);
int nttmul_ksntt_get_info(const nttmul_ksntt *k, nttmul_ksntt_info *info);

/* Device-resident operands of info.word_bits-wide words on HIP device `dev` (one of the
 * context's), enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE they wait for the
 * range check). */
int nttmul_ksntt_modup_device(nttmul_ksntt *k, void *up_hat, const void *x_hat, size_t batch,
                              int dev, void *stream);
int nttmul_ksntt_mac_device(nttmul_ksntt *k, void *c_hat, const void *a_hat, const void *b_hat,
                            const uint32_t *rot, uint32_t rots, size_t batch, uint32_t terms,
                            uint32_t comps, int dev, void *stream);

/* Host buffers.  Deliberately simple, as nttmul_mdntt_moddown: the context's first device, device
 * buffers owned by the call, the device path, a copy back and a synchronise. */
int nttmul_ksntt_modup(nttmul_ksntt *k, void *up_hat, const void *x_hat, size_t batch);
int nttmul_ksntt_mac(nttmul_ksntt *k, void *c_hat, const void *a_hat, const void *b_hat,
                     const uint32_t *rot, uint32_t rots, size_t batch, uint32_t terms,
                     uint32_t comps);

#define NTTMUL_KSNTT_MODUP 0
#define NTTMUL_KSNTT_MAC 1

/* The kernels a sub-batch of `op` launches, joined by " + ", in the format of
 * nttmul_mdntt_kernel_name.  modup (comps is ignored):
 * "k_mdntt_inv<Arith32P,u32,12> + k_ksntt_fwd<Arith32P,u32,12>", or above n = 4096
 * "k_mdntt_inv_rows<Arith64,u64,1> + k_rnsmp_cols_inv<Arith64,u64,1> +
 * k_ksntt_cols_fwd<Arith64,u64,1> + k_ksntt_rows<Arith64,u64,1>"; mac:
 * "k_ksntt_mac<Arith32P,u32,2>" (the last argument is comps).  Returns the untruncated length, or
 * a negative status (NTTMUL_EINVAL for another op, or for comps outside 1 ..
 * NTTMUL_MACN_MAX_COMPS with op = NTTMUL_KSNTT_MAC). */
int nttmul_ksntt_kernel_name(const nttmul_ksntt *k, int op, uint32_t comps, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_KSNTT_H */
