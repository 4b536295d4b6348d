/*
 * nttmul_hoist.h — hoisted rotations: the mac against NTT-domain operands with `a` already in the
 * NTT domain and the automorphism fused into its load: lib/libnttmul_hoist.so (not
 * libnttmul_macn.so, nor any of the older libraries).
 *
 * libnttmul_hoist.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h, nttmul_rns.h,
 * nttmul_bconv.h, nttmul_rnsmp.h, nttmul_galois.h, nttmul_ks.h and nttmul_macn.h with the same
 * kernels, plus the entry points below and the kernels behind them (csrc/hoist_dev.hpp
 * k_rns_hoist, k_rnsmp_hoist).  They work on the existing contexts, nttmul_rns (n <= 4096) and
 * nttmul_rnsmp (4096 < n <= 65536): there is no new context type.  A context must come from this
 * library's own nttmul_rns_create / nttmul_rnsmp_create.
 *
 *   c[p][r][i][l] = INTT_l( sum over t < terms of a_hat[p][t][l][src_{k_r}(j)] o b_hat[r][i][t][l][j] )
 *                                                                      for r < rots, i < comps
 *   a_hat  [batch][terms][limbs][n]          NTT order, canonical: nttmul_*_forward over the
 *                                            batch * terms polynomials nttmul_ks_modup writes, as
 *                                            it stands
 *   b_hat  [rots][comps][terms][limbs][n]    NTT order, canonical, shared by the batch (the
 *                                            rotation keys); any canonical vector is accepted
 *   k      [rots]                            odd, 0 < k < 2n; read during the call and passed to
 *                                            the kernel by value, as nttmul_galois_ntt_many's
 *   c      [batch][rots][comps][limbs][n]    coefficient order, canonical: what
 *                                            nttmul_ks_moddown_device reads with
 *                                            batch * rots * comps polynomials
 *
 * src_k(j) is the NTT-order permutation of sigma_k : a(x) -> a(x^k) (nttmul_galois.h:
 * nttmul_galois_ntt(a_hat, k)[j] = a_hat[src_k(j)], nttmul_galois_plan's ntt_src).  Result (r, i)
 * equals, bit for bit, the same context's mac_ntt of nttmul_galois_coeff(a, k_r) against
 * b_hat[r][i], for a_hat = forward(a): both are the canonical representative of the same residue.
 * k = 1 is the identity, so rots = 1, k = {1} is the plain pointwise mac and inverse on an
 * NTT-domain a.
 *
 * What is saved.  R rotations of one ciphertext as R key switches run R (dnum + 2) transforms per
 * limb polynomial and R base conversions (galois_coeff, modup, macn_ntt, moddown each time).
 * Hoisted, the digits are raised and transformed once and every rotation runs only its inverse
 * transforms: modup, forward over batch * dnum, one hoist_ntt (terms = dnum, comps = 2), moddown
 * over batch * rots * 2.  That is dnum + 2 R transforms and one modup.
 *
 * Range contract.  Per arithmetic class it is k_mac's (csrc/mac_dev.hpp), per accumulator: every
 * word of a_hat and of b_hat canonical (below its own limb's modulus), which is inside the range
 * the products accept from a forward transform; each accumulator stays canonical (32-bit words)
 * or in [0, 2q) (64-bit words) by one conditional subtraction per term.
 *
 * Status, all decided before any device access, in this order.  NTTMUL_EINVAL: a NULL context;
 * terms = 0; comps = 0 or comps > NTTMUL_MACN_MAX_COMPS; rots = 0 or rots > NTTMUL_HOIST_MAX_ROTS;
 * a NULL k; an even k[r], k[r] = 0 or k[r] >= 2n for an r < rots; a NULL operand with batch > 0.
 * batch = 0 is then a successful no-op.  NTTMUL_ENODEV as in nttmul.h (no device, or `dev` not one
 * of the context's).  With NTTMUL_FLAG_VALIDATE the words of a_hat and of all of b_hat are
 * range-checked on the device first (the k_rns_check_range of nttmul_rns.h) and the call returns
 * NTTMUL_ERANGE without touching c; the call then waits for the check.  The error text is the
 * context's (nttmul_rns_last_error / nttmul_rnsmp_last_error).
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_hoist_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  c must overlap neither a_hat nor b_hat.
 *   Footprint.  A call writes exactly batch * rots * comps * limbs * n words of c and nothing else
 *     in caller memory; inputs are never written.
 *   Addressing.  Polynomial, term, rotation and component offsets are computed in 64 bits.
 *
 * Launches.  nttmul_rns: one.  nttmul_rnsmp: two per sub-batch -- k_rnsmp_hoist, which reads a_hat
 * and b_hat from caller memory, and the context's own k_rnsmp_cols_inv, which writes c.  The
 * sub-batch is the largest number of output units (p, r) whose units * comps polynomials do not
 * exceed the context's scratch_mb (never less than one); the scratch grows, is handed between
 * streams and is freed exactly as for the context's other operations, and a context still serves
 * one host thread at a time.
 *
 * Out of scope here:
 *   - a per-batch b_hat;
 *   - more than two components;
 *   - NTT-domain output (nttmul_ksntt_mac of nttmul_ksntt.h, lib/libnttmul_ksntt.so);
 *   - the rotation of the c_0 part of a ciphertext (nttmul_galois_coeff does it);
 *   - a fused modup or moddown;
 *   - a bench.py mode (tools/bench_hoist.py measures these calls).
 */
#ifndef NTTMUL_HOIST_H
#define NTTMUL_HOIST_H

#include "nttmul_macn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NTTMUL_HOIST_MAX_ROTS NTTMUL_GALOIS_MAX_COUNT

/* Device-resident operands of the context's word size on HIP device `dev` (one of the context's),
 * enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE they wait for the range check).
 * k is host memory. */
int nttmul_rns_hoist_ntt_device(nttmul_rns *r, void *c, const void *a_hat, const void *b_hat,
                                const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                                uint32_t comps, int dev, void *stream);
int nttmul_rnsmp_hoist_ntt_device(nttmul_rnsmp *r, void *c, const void *a_hat, const void *b_hat,
                                  const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                                  uint32_t comps, int dev, void *stream);

/* Host buffers.  Deliberately simple, as nttmul_rns_mac_ntt: the context's first device, device
 * buffers owned by the call, the device path, a copy back and a synchronise. */
int nttmul_rns_hoist_ntt(nttmul_rns *r, void *c, const void *a_hat, const void *b_hat,
                         const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                         uint32_t comps);
int nttmul_rnsmp_hoist_ntt(nttmul_rnsmp *r, void *c, const void *a_hat, const void *b_hat,
                           const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                           uint32_t comps);

/* The kernel(s) a call with `comps` dispatches to, in the format of nttmul_rns_kernel_name and
 * nttmul_rnsmp_kernel_name: "k_rns_hoist<Arith32P,u32,12,2>", or "k_rnsmp_hoist<Arith64,u64,4,2>
 * + k_rnsmp_cols_inv<Arith64,u64,4>" (one string).  Returns the untruncated length, or a negative
 * status. */
int nttmul_rns_hoist_kernel_name(const nttmul_rns *r, uint32_t comps, char *buf, size_t cap);
int nttmul_rnsmp_hoist_kernel_name(const nttmul_rnsmp *r, uint32_t comps, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_HOIST_H */
