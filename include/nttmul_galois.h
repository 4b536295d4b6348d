/*
 * nttmul_galois.h — Galois automorphisms over all limbs of an RNS basis: lib/libnttmul_galois.so
 * (not libnttmul_rnsmp.so, nor any of the older libraries).
 *
 * libnttmul_galois.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h, nttmul_rns.h,
 * nttmul_bconv.h and nttmul_rnsmp.h with the same kernels, plus the entry points below and the
 * kernels behind them (csrc/galois_dev.hpp k_galois_coeff, k_galois_ntt, k_galois_ntt_many).
 *
 * The automorphism sigma_k : a(x) -> a(x^k) mod (x^n + 1), k odd, 0 < k < 2n, is the step that
 * turns a key switch into a slot rotation (k = 5^step mod 2n) or a conjugation (k = 2n - 1), and
 * what a hoisted rotation applies to the digits before nttmul_*_mac_ntt.  It is pure data movement:
 *
 *   coefficient order   coefficient i goes to e = i k mod 2n: stored at e when e < n, negated at
 *                       e - n otherwise.  As a gather: out[j] = +-in[i0 mod n], i0 = j k^-1 mod 2n,
 *                       negated when i0 >= n.  Outputs are canonical: a negated word x gives
 *                       q_l - x, a negated 0 gives 0.
 *   NTT order           slot j of the forward transforms of this project (bit-reversed, canonical:
 *                       what nttmul_rns_forward_* / nttmul_rnsmp_forward_* write and mac_ntt reads
 *                       as b_hat) is a(psi^(2 brv(j) + 1)), brv reversing log2 n bits.  sigma_k is
 *                       the permutation out_hat[j] = in_hat[src(j)],
 *                       src(j) = brv(((k (2 brv(j) + 1)) mod 2n - 1) / 2): no arithmetic on values,
 *                       no modulus.  It maps every aligned block of 2^m consecutive slots onto one
 *                       aligned block of 2^m slots.
 *
 * so that, per limb, nttmul_*_forward(sigma_k(a)) == galois_ntt(nttmul_*_forward(a), k), bit for
 * bit.
 *
 * An nttmul_galois context holds L = limbs distinct primes for one power-of-two n in 256 .. 65536:
 * one context spans the degrees of nttmul_rns_* (n <= 4096) and nttmul_rnsmp_* (above).  Operands
 * are [batch][limbs][n] as everywhere: polynomial p of limb l starts at word (p L + l) n.
 *
 * Word size.  Either every q_l < 2^31 and all operands are 32-bit words, or every q_l >= 2^32
 * (q_l < 2^62) and all operands are 64-bit words; nttmul_galois_info.word_bits says which.
 *
 * Status, all decided before any device access: NTTMUL_EINVAL for a NULL context, limbs of 0 or
 * above NTTMUL_RNS_MAX_LIMBS, an n that is not a power of two or below 256, a q_l that is not
 * prime, not 1 mod 2n or >= 2^62, two equal primes, non-zero params->q or params->psi, an even k,
 * k = 0, k >= 2n, count = 0, count > NTTMUL_GALOIS_MAX_COUNT, or a NULL operand with batch > 0.
 * NTTMUL_EUNSUPPORTED for n > 65536, for NTTMUL_FLAG_CYCLIC, for any q_l in [2^31, 2^32) and for
 * mixed classes.  batch = 0 is a successful no-op; k = 1 is a valid copy.  NTTMUL_ENODEV as in
 * nttmul.h (no device, or `dev` not one of the context's).
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_galois_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  out must not overlap in: a permutation has no in-place form here.
 *   Footprint.  A call writes exactly count * batch * limbs * n words of its output (count = 1 for
 *     the single calls) and nothing else in caller memory; inputs are never written.
 *   Addressing.  Polynomial base offsets are computed in 64 bits; inside a polynomial 32 bits
 *     suffice (2n is a power of two, so the wrap-around of k (2 r + 1) in 32 bits is harmless).
 *
 * Every device call is one launch (grid: workgroups x limbs) and uses no scratch, no table of
 * indices and no twiddles: the indices are computed per lane.  NTTMUL_FLAG_VALIDATE range-checks
 * the input words against their own limb's modulus on the device first (the k_rns_check_range of
 * nttmul_rns.h: word i belongs to limb (i / n) mod limbs) and returns NTTMUL_ERANGE; the call then
 * waits for the check.  One context serves one host thread at a time.  nttmul_galois_destroy does
 * not wait for the streams passed to the *_device calls: synchronise them first.
 *
 * Out of scope here:
 *   - automorphisms fused into the transforms (fused into the mac against NTT-domain operands:
 *     include/nttmul_hoist.h, lib/libnttmul_hoist.so);
 *   - a coefficient-order `many`;
 *   - in-place forms;
 *   - cyclic contexts (NTTMUL_FLAG_CYCLIC), the class 2^31 <= q < 2^32;
 *   - a chunked or multi-device host path (the host forms below are deliberately simple);
 *   - a bench.py mode.
 */
#ifndef NTTMUL_GALOIS_H
#define NTTMUL_GALOIS_H

#include "nttmul_rnsmp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NTTMUL_GALOIS_MAX_COUNT 16

typedef struct nttmul_galois nttmul_galois;

typedef struct {
  uint32_t n, logn, limbs;
  uint32_t word_bits;  /* 32: every q_l < 2^31; 64: every q_l >= 2^32.  The word of every operand */
  int ndev;
} nttmul_galois_info;

/* params: n, ndev, first_dev and flags as for nttmul_create_sized (params_size likewise);
 * params->q and params->psi must be 0; the dispatch knobs are ignored.
 * q[0 .. limbs): the moduli, in limb order. */
int nttmul_galois_create(nttmul_galois **g, const nttmul_params *params, size_t params_size,
                         const uint64_t *q, uint32_t limbs);
void nttmul_galois_destroy(nttmul_galois *g);
const char *nttmul_galois_last_error(const nttmul_galois *g);
int nttmul_galois_get_info(const nttmul_galois *g, nttmul_galois_info *info);
/* q, psi, omega, ... of one limb, as nttmul_get_info of a plain context of (n, q_limb) */
int nttmul_galois_limb_info(const nttmul_galois *g, uint32_t limb, nttmul_info *info);

/* Host only (no device, no context).
 * nttmul_galois_element: *k = 5^step mod 2n (a negative step: powers of 5^-1 mod 2n), times
 * 2n - 1 mod 2n when conjugate != 0.  NTTMUL_EINVAL for an n that is not a power of two in
 * 256 .. 65536, or a NULL k.
 * nttmul_galois_plan: the index tables the kernels compute per lane, n entries each (a NULL table
 * is skipped):  out[j] = (coeff_neg[j] ? -in : in)[coeff_src[j]]  in coefficient order,
 * out_hat[j] = in_hat[ntt_src[j]] in NTT order.  NTTMUL_EINVAL for such an n, an even k, k = 0 or
 * k >= 2n. */
int nttmul_galois_element(uint32_t n, int64_t step, int conjugate, uint32_t *k);
int nttmul_galois_plan(uint32_t n, uint32_t k, uint32_t *coeff_src, uint8_t *coeff_neg,
                       uint32_t *ntt_src);

/* Device-resident operands of info.word_bits-wide words on HIP device `dev` (one of the
 * context's), enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE they wait for the
 * range check).  One launch each.  in, out: [batch][limbs][n].
 * nttmul_galois_ntt_many_device: `count` automorphisms k[0 .. count) of one input in one launch,
 * out [count][batch][limbs][n]; k is read during the call (passed to the kernel by value: no
 * device table, no synchronisation).  Each input word is read once and written count times.
 * count = 1 gives nttmul_galois_ntt_device's result. */
int nttmul_galois_coeff_device(nttmul_galois *g, void *out, const void *in, uint32_t k,
                               size_t batch, int dev, void *stream);
int nttmul_galois_ntt_device(nttmul_galois *g, void *out, const void *in, uint32_t k, size_t batch,
                             int dev, void *stream);
int nttmul_galois_ntt_many_device(nttmul_galois *g, void *out, const void *in, const uint32_t *k,
                                  uint32_t count, size_t batch, int dev, void *stream);

/* Host buffers.  Deliberately simple, as nttmul_rns_*: the context's first device, device buffers
 * owned by the call, the device path, a copy back and a synchronise. */
int nttmul_galois_coeff(nttmul_galois *g, void *out, const void *in, uint32_t k, size_t batch);
int nttmul_galois_ntt(nttmul_galois *g, void *out, const void *in, uint32_t k, size_t batch);

/* The kernel of an operation (op: 0 coeff, 1 ntt, 2 ntt_many with `count` automorphisms; count is
 * ignored for 0 and 1), in the format of nttmul_rnsmp_kernel_name, e.g. "k_galois_coeff<u32,0>"
 * (the number: log2 of the residue classes mod M a limb polynomial is split in so that one class,
 * n / M words, fits the kernel's LDS stage; chosen by n and the word, 0 = staged whole),
 * "k_galois_ntt<u64>", "k_galois_ntt_many<u32>".  Returns the untruncated length, or a negative
 * status. */
int nttmul_galois_kernel_name(const nttmul_galois *g, int op, uint32_t count, char *buf,
                              size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_GALOIS_H */
