/*
 * nttmul_xconv.h — exact base extension and rounded ModDown on NTT-domain limbs:
 * lib/libnttmul_xconv.so (not libnttmul_ctmul.so, nor any of the older libraries).
 *
 * libnttmul_xconv.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h, nttmul_rns.h,
 * nttmul_bconv.h, nttmul_rnsmp.h, nttmul_galois.h, nttmul_ks.h, nttmul_macn.h, nttmul_hoist.h,
 * nttmul_mdntt.h, nttmul_ksntt.h, nttmul_lintrans.h and nttmul_ctmul.h with the same kernels, plus
 * the entry points below and the kernels behind them (csrc/xconv_dev.hpp k_xconv_*).
 *
 * An nttmul_xconv context holds, for one power-of-two n in 256 .. 65536, the basis
 * Q = (q_0 .. q_{L-1}), the basis P = (p_0 .. p_{K-1}), disjoint from Q and of the same word
 * class, and a scale t >= 1.  The extended basis is ordered Q, then P (as nttmul_mdntt.h).  Write
 * Ph_j = P / p_j.  Every limb of every operand is a transform: bit-reversed NTT order, canonical
 * words, what nttmul_rns_forward / nttmul_rnsmp_forward write for that limb's modulus.
 * The moduli of a context may be of any sizes within their word class and in any order
 * (tests/test_gpu_xconv_bases.py).
 *
 * Both operations rest on the centred residue of an integer modulo P, which the fast conversion
 * of nttmul_bconv.h / nttmul_mdntt.h leaves uncorrected.  For a coefficient whose residues of
 * t X modulo the p_j are known,
 *              y_j  = [t X]_{p_j} (Ph_j^-1 mod p_j) mod p_j
 *              S    = sum over j of y_j Ph_j            = t X mod P, plus alpha P with 0 <= alpha < K
 *              phi  = sum over j of y_j / p_j           = S / P
 *              a    = floor(phi + 1/2)                  in 0 .. K
 *              c    = S - a P                           the representative in [-(P-1)/2, (P-1)/2]
 * P is odd, so phi + 1/2 is never an integer and no tie exists.
 *
 *   extend   p_hat [batch][K][n] over P -> out [batch][L][n] over Q
 *              out[p][l] = NTT_{q_l}(c mod q_l)
 *            with c the centred representative of the CRT value of t (input) mod P.  t = 1 is the
 *            exact basis extension; K = 1 is ModRaise, the centred lift of one limb.
 *
 *   moddown  x_hat [batch][L + K][n] -> out [batch][L][n]
 *              out[p][l] = NTT_{q_l}(round(t X / P) mod q_l)
 *            for the CRT value X of the input over Q u P: (t X - c) / P = round(t X / P).  Per limb
 *            that is (x_hat[p][l] - NTT_{q_l}(c t^-1)) (t P^-1 mod q_l).  t = 1 is the rounded
 *            ModDown, and the rounded rescale at K = 1; t > 1 with the roles (Q, P) := (B, Q) is
 *            BFV's scale-and-round.  The merged context of INTEGRATION.md section 2k works as
 *            before: q[:L-1] and (q_{L-1},) + p.
 *
 * The contract on a.  a needs more than a word of precision, so the contract has a guard band:
 * eps = K 2^-band_log2 (nttmul_xconv_info.band_log2; 46 in this library, csrc/xconv_dev.hpp and
 * DESIGN.md section 4 derive it).  For every coefficient with |frac(phi) - 1/2| > eps the output
 * is the exact value above.  Inside the band c is one of the two candidates c or c +- P, the same
 * one in all L limbs: moddown's output is round(t X / P) or its neighbour, extend's c or c +- P.
 * Every workgroup of a call computes a from the same y in the same fixed order with explicit
 * fused multiply-adds, so the choice never differs between limbs.
 *
 * Word size, as nttmul_rns.h: every modulus of both bases below 2^31 (32-bit words) or every one
 * in [2^32, 2^62) (64-bit words); nttmul_xconv_info.word_bits says which.
 *
 * Status, all decided before any device access: nttmul_mdntt_create's, in the same order; then
 * NTTMUL_EINVAL for a scale of 0, of 2^62 or above, or that is 0 modulo some q_l.  A call returns
 * NTTMUL_EINVAL for a NULL context or a NULL operand with batch > 0; batch = 0 is a successful
 * no-op.  NTTMUL_ENODEV as in nttmul.h (no device, or `dev` not one of the context's).
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_xconv_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  out must not overlap the input.
 *   Footprint.  A call writes exactly batch * L * n words of out and nothing else in caller
 *     memory; the input is never written.
 *   Addressing.  Every offset is computed in 64 bits: batch * (L + K) * n may pass 2^32 words.
 *
 * Scratch, as nttmul_mdntt.h: the intermediates (the K coefficient-order limbs y, and above
 * n = 4096 the column-passed sums as well) live in a scratch the context owns per device, bounded
 * by params->scratch_mb (0: 512) per buffer: a larger batch runs as sub-batches of whole
 * polynomials on the same stream, never less than one polynomial.  Uses of the scratch are ordered
 * by an event whatever stream they were enqueued on; a context serves one host thread at a time.
 * NTTMUL_FLAG_VALIDATE range-checks the input over its limbs on the device first (the
 * k_rns_check_range of nttmul_rns.h) and returns NTTMUL_ERANGE without touching out; the call
 * then waits for the check.  nttmul_xconv_destroy waits for the last use of the scratch, not for
 * the streams passed to the *_device calls: synchronise them first.
 *
 * Out of scope here:
 *   - BGV's t-correcting ModDown (nttmul_tmd.h, lib/libnttmul_tmd.so, has it on the same operands,
 *     built on the uncorrected sum S instead of the centred c);
 *   - a computed once per coefficient in a pass of its own (each of the L target-limb workgroups
 *     recomputes it; tools/bench_xconv.py measures what that costs);
 *   - a coefficient-order input or output;
 *   - cyclic contexts (NTTMUL_FLAG_CYCLIC), the class 2^31 <= q < 2^32;
 *   - a chunked or multi-device host path (the host forms below are deliberately simple);
 *   - a bench.py mode (tools/bench_xconv.py measures these calls).
 */
#ifndef NTTMUL_XCONV_H
#define NTTMUL_XCONV_H

#include "nttmul_ctmul.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nttmul_xconv nttmul_xconv;

typedef struct {
  uint32_t n, logn, q_limbs, p_limbs;
  uint32_t word_bits;  /* 32: every modulus < 2^31; 64: every modulus >= 2^32.  The word of every operand */
  int ndev;
  uint32_t scratch_mb; /* the bound of one scratch buffer, in MiB */
  uint32_t band_log2;  /* the guard band of a is eps = p_limbs 2^-band_log2 */
  uint64_t scale;      /* t */
} nttmul_xconv_info;

/* params: n, ndev, first_dev, flags and scratch_mb as for nttmul_mdntt_create (params_size
 * likewise); params->q and params->psi must be 0; the dispatch knobs are ignored.
 * q[0 .. q_limbs) and p[0 .. p_limbs): the two bases, in limb order.  scale: t. */
int nttmul_xconv_create(nttmul_xconv **x, const nttmul_params *params, size_t params_size,
                        const uint64_t *q, uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs,
                        uint64_t scale);
void nttmul_xconv_destroy(nttmul_xconv *x);
const char *nttmul_xconv_last_error(const nttmul_xconv *x);
int nttmul_xconv_get_info(const nttmul_xconv *x, nttmul_xconv_info *info);

/* Device-resident operands of info.word_bits-wide words on HIP device `dev` (one of the
 * context's), enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE they wait for the
 * range check).  p_hat [batch][K][n] -> out [batch][L][n]; x_hat [batch][L + K][n] -> out
 * [batch][L][n]. */
int nttmul_xconv_extend_device(nttmul_xconv *x, void *out, const void *p_hat, size_t batch,
                               int dev, void *stream);
int nttmul_xconv_moddown_device(nttmul_xconv *x, void *out, const void *x_hat, size_t batch,
                                int dev, void *stream);

/* Host buffers.  Deliberately simple, as nttmul_mdntt_moddown: the context's first device, device
 * buffers owned by the call, the device path, a copy back and a synchronise. */
int nttmul_xconv_extend(nttmul_xconv *x, void *out, const void *p_hat, size_t batch);
int nttmul_xconv_moddown(nttmul_xconv *x, void *out, const void *x_hat, size_t batch);

/* Host-only, no device: the plain constants of (q, p, scale), each output optional (NULL skips
 * it).  yscale [K]: t Ph_j^-1 mod p_j.  w_ext [K + 1][L]: Ph_j mod q_l, and in row K -P mod q_l.
 * w_md [K + 1][L]: Ph_j t^-1 mod q_l, and in row K -P t^-1 mod q_l.  v [L]: t P^-1 mod q_l.
 * Returns the status nttmul_xconv_create would return before any device access. */
int nttmul_xconv_plan(const nttmul_params *params, size_t params_size, const uint64_t *q,
                      uint32_t q_limbs, const uint64_t *p, uint32_t p_limbs, uint64_t scale,
                      uint64_t *yscale, uint64_t *w_ext, uint64_t *w_md, uint64_t *v);

#define NTTMUL_XCONV_EXTEND 0
#define NTTMUL_XCONV_MODDOWN 1

/* The kernels a sub-batch of `op` launches, joined by " + ", in the format of
 * nttmul_mdntt_kernel_name: extend "k_mdntt_inv<Arith32P,u32,12> + k_xconv_fwd<Arith32P,u32,12,0>",
 * or above n = 4096 "k_mdntt_inv_rows<Arith64,u64,1> + k_rnsmp_cols_inv<Arith64,u64,1> +
 * k_xconv_cols_fwd<Arith64,u64,1> + k_xconv_rows<Arith64,u64,1>"; moddown
 * "k_mdntt_inv<Arith32P,u32,12> + k_xconv_fwd<Arith32P,u32,12,1>", or above n = 4096
 * "... + k_xconv_cols_fwd<Arith64,u64,1> + k_mdntt_rows<Arith64,u64,1>".  Returns the untruncated
 * length, or a negative status (NTTMUL_EINVAL for another op). */
int nttmul_xconv_kernel_name(const nttmul_xconv *x, int op, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_XCONV_H */
