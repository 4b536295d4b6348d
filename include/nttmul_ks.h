/*
 * nttmul_ks.h — digit ModUp and ModDown for hybrid key switching: lib/libnttmul_ks.so (not
 * libnttmul_galois.so, nor any of the older libraries).
 *
 * libnttmul_ks.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h, nttmul_rns.h,
 * nttmul_bconv.h, nttmul_rnsmp.h and nttmul_galois.h with the same kernels, plus the entry points
 * below and the kernel behind them (csrc/ks_dev.hpp k_ks_modup; ModDown launches the k_bconv of
 * nttmul_bconv.h).
 *
 * An nttmul_ks context holds, for one power-of-two n in 256 .. 65536, the basis
 * Q = (q_0 .. q_{L-1}), the special basis P = (p_0 .. p_{K-1}), disjoint from Q and of the same
 * word class, and a digit width alpha = digit_limbs, 1 <= alpha <= L.  Digit d is the set of
 * limbs D_d = [d alpha, min((d + 1) alpha, L)); there are dnum = ceil(L / alpha) digits and the
 * last one may be shorter.  The extended basis is ordered q_0 .. q_{L-1}, p_0 .. p_{K-1}: the
 * order nttmul_bconv_moddown expects, `to` limbs first and `from` limbs after them.  Write D_d
 * also for the product of its primes, and Dh_i = D_{d(i)} / q_i for the digit d(i) of limb i.
 * Operands are polynomial-major arrays of residue limbs in coefficient (standard) order: these
 * are not transforms.  Every input word is canonical (below its own limb's modulus) and so is
 * every output word.
 * The moduli of a context may be of any sizes within their word class and in any order
 * (tests/test_gpu_bases.py).
 *
 *   modup    in [batch][L][n] -> out [batch][dnum][L + K][n]
 *              y_i             = in[p][i][k] (Dh_i^-1 mod q_i) mod q_i             for i in D_d
 *              out[p][d][m][k] = (sum over i in D_d of y_i Dh_i) mod the m-th modulus of Q u P
 *            The integer sum is x_d + u D_d, where x_d in [0, D_d) is the CRT value of the digit
 *            and 0 <= u < |D_d|: the unreduced-alpha conversion of nttmul_bconv.h.  For m in D_d
 *            the formula itself yields in[p][m][k], because D_d = 0 mod q_m: the digit's own
 *            limbs pass through bit for bit.  out is exactly nttmul_*_mac_ntt's operand
 *            a [batch][terms][limbs][n] with terms = dnum and limbs = L + K; the key is the
 *            shared b_hat [terms][limbs][n].
 *   moddown  x [batch][L + K][n] -> out [batch][L][n]
 *            nttmul_bconv_moddown with from = P and to = Q, at any n in 256 .. 65536:
 *              out[p][i][k] = (x[p][i][k] - convert(x[p][L .. L+K))[i][k]) (P^-1 mod q_i) mod q_i
 *
 * With them a hybrid key switch is modup, nttmul_rns_mac_ntt_device or
 * nttmul_rnsmp_mac_ntt_device (shared = 1, terms = dnum) once per key component, and moddown of
 * each result, on device-resident data with no re-layout in between.
 *
 * Word size, as nttmul_rns.h: every modulus of both bases below 2^31 (32-bit words) or every one
 * in [2^32, 2^62) (64-bit words); nttmul_ks_info.word_bits says which.
 *
 * Status, all decided before any device access.  NTTMUL_EINVAL: what nttmul_galois_create
 * returns it for, for each basis (a NULL argument, limbs of 0 or above NTTMUL_RNS_MAX_LIMBS, so
 * p_limbs = 0 too, an n that is not a power of two or below 256, a modulus that is not prime, not
 * 1 mod 2n or >= 2^62, non-zero params->q or params->psi), a prime that occurs twice, within a
 * basis or in both, digit_limbs = 0 or > q_limbs, and q_limbs + p_limbs > NTTMUL_RNS_MAX_LIMBS
 * (the extended basis has to fit one nttmul_rns or nttmul_rnsmp context).  NTTMUL_EUNSUPPORTED:
 * n > 65536, NTTMUL_FLAG_CYCLIC, a modulus in [2^31, 2^32), mixed classes within or across Q and
 * P, and a basis the mac_ntt context of that degree would refuse (32-bit words at n = 4096:
 * nttmul_rns_create's condition on every modulus).  A call returns NTTMUL_EINVAL for a NULL
 * context or a NULL operand with batch > 0; batch = 0 is a successful no-op.  NTTMUL_ENODEV as in
 * nttmul.h (no device, or `dev` not one of the context's).
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_ks_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  out must not overlap the input.
 *   Footprint.  modup writes exactly batch * dnum * (L + K) * n words of out, moddown exactly
 *     batch * L * n, and nothing else in caller memory; inputs are never written.
 *   Addressing.  Polynomial and digit offsets are computed in 64 bits:
 *     batch * dnum * (L + K) * n may pass 2^32 words.
 *
 * Every device call is one launch.  A context has no scratch and no state between calls; it
 * serves one host thread at a time.  NTTMUL_FLAG_VALIDATE range-checks the input words against
 * their own limb's modulus on the device first (the k_rns_check_range of nttmul_rns.h, over the
 * input's own limb count: L for modup, L + K for moddown) and returns NTTMUL_ERANGE; the call
 * then waits for the check.  nttmul_ks_destroy does not wait for the streams passed to the
 * *_device calls: synchronise them first.
 *
 * Out of scope here:
 *   - one call that runs the whole key switch on scratch of its own;
 *   - a mac that shares the forward transforms between the two key components: that is
 *     nttmul_macn.h (lib/libnttmul_macn.so), whose one call replaces the two mac_ntt calls above;
 *   - NTT-domain input or output, that is a fused inverse -> modup -> forward pipeline (ModUp of
 *     NTT-domain limbs is nttmul_ksntt.h, lib/libnttmul_ksntt.so; ModDown of NTT-domain limbs is
 *     nttmul_mdntt.h, lib/libnttmul_mdntt.so);
 *   - exact conversion (the alpha correction), and rounding instead of flooring in moddown;
 *   - raising nttmul_bconv_create's own n limit (it stays at 4096);
 *   - cyclic contexts (NTTMUL_FLAG_CYCLIC), the class 2^31 <= q < 2^32;
 *   - a chunked or multi-device host path (the host forms below are deliberately simple);
 *   - a bench.py mode (tools/bench_ks.py measures these calls).
 */
#ifndef NTTMUL_KS_H
#define NTTMUL_KS_H

#include "nttmul_galois.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nttmul_ks nttmul_ks;

typedef struct {
  uint32_t n, logn, q_limbs, p_limbs, digit_limbs, digits;
  uint32_t word_bits;  /* 32: every modulus < 2^31; 64: every modulus >= 2^32.  The word of every operand */
  int ndev;
} nttmul_ks_info;

/* params: n, ndev, first_dev and flags as for nttmul_create_sized (params_size likewise);
 * params->q and params->psi must be 0; the dispatch knobs are ignored.
 * q[0 .. q_limbs) and p[0 .. p_limbs): the two bases, in limb order; digit_limbs: alpha. */
int nttmul_ks_create(nttmul_ks **k, const nttmul_params *params, size_t params_size,
                     const uint64_t *q, uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs,
                     uint32_t digit_limbs);
void nttmul_ks_destroy(nttmul_ks *k);
const char *nttmul_ks_last_error(const nttmul_ks *k);
int nttmul_ks_get_info(const nttmul_ks *k, nttmul_ks_info *info);

/* Host only, needs no device: the validation of nttmul_ks_create with its statuses, and the
 * plain constants a context's device tables are derived from (a NULL table is skipped), with
 * L = q_limbs, K = p_limbs, dnum = ceil(L / digit_limbs) and m over the extended basis:
 *   inv[i]                  = Dh_i^-1 mod q_i                                   [L]
 *   w[i * (L + K) + m]      = Dh_i mod m-th modulus                             [L][L + K]
 *   gadget[d * (L + K) + m] = P (Q / D_d) ((Q / D_d)^-1 mod D_d) mod m-th       [dnum][L + K]
 *                             the factor a key generator multiplies s' by in digit d
 *   pinv, pw, Pinv          = inv, w, binv of nttmul_bconv_plan(from = P, to = Q)
 *                                                                               [K], [K][L], [L] */
int nttmul_ks_plan(const nttmul_params *params, size_t params_size, const uint64_t *q,
                   uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs, uint32_t digit_limbs,
                   uint64_t *inv, uint64_t *w, uint64_t *gadget, uint64_t *pinv, uint64_t *pw,
                   uint64_t *Pinv);

/* Device-resident operands of info.word_bits-wide words on HIP device `dev` (one of the
 * context's), enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE they wait for the
 * range check).  One kernel launch each.
 * modup: in [batch][L][n] -> out [batch][dnum][L + K][n].
 * moddown: in [batch][L + K][n] -> out [batch][L][n]. */
int nttmul_ks_modup_device(nttmul_ks *k, void *out, const void *in, size_t batch, int dev,
                           void *stream);
int nttmul_ks_moddown_device(nttmul_ks *k, void *out, const void *in, size_t batch, int dev,
                             void *stream);

/* Host buffers.  Deliberately simple, as nttmul_bconv_*: the context's first device, device
 * buffers owned by the call, the device path, a copy back and a synchronise. */
int nttmul_ks_modup(nttmul_ks *k, void *out, const void *in, size_t batch);
int nttmul_ks_moddown(nttmul_ks *k, void *out, const void *in, size_t batch);

/* The kernel an operation dispatches to (op: 0 modup, 1 moddown), in the format of
 * nttmul_bconv_kernel_name: "k_ks_modup<u32>", "k_ks_modup<u64>"; moddown reuses "k_bconv<u32,1>"
 * or "k_bconv<u64,1>".  Returns the untruncated length, or a negative status. */
int nttmul_ks_kernel_name(const nttmul_ks *k, int op, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_KS_H */
