/*
 * nttmul_macn.h — the mac against several NTT-domain operands with the forward transforms shared:
 * lib/libnttmul_macn.so (not libnttmul_ks.so, nor any of the older libraries).
 *
 * libnttmul_macn.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h, nttmul_rns.h,
 * nttmul_bconv.h, nttmul_rnsmp.h, nttmul_galois.h and nttmul_ks.h with the same kernels, plus the
 * entry points below and the kernels behind them (csrc/macn_dev.hpp k_rns_macn, k_rnsmp_macn).
 * They work on the existing contexts, nttmul_rns (n <= 4096) and nttmul_rnsmp (4096 < n <= 65536):
 * everything they need -- the limbs' tables and twiddles, the multi-pass scratch -- is already
 * there, so there is no new context type.  A context must come from this library's own
 * nttmul_rns_create / nttmul_rnsmp_create.
 *
 *   c[p][i][l] = INTT_l( sum over t < terms of NTT_l(a[p][t][l]) o b_hat[p or shared][i][t][l] )
 *                                                                                     for i < comps
 *   a      [batch][terms][limbs][n]           coefficient order, canonical: what nttmul_ks_modup
 *                                             writes, as it stands
 *   b_hat  [comps][terms][limbs][n] (shared != 0)  or  [batch][comps][terms][limbs][n]
 *                                             canonical words in the order nttmul_*_forward writes
 *   c      [batch][comps][limbs][n]           coefficient order, canonical
 *
 * Component i of every result equals, bit for bit, what the same context's mac_ntt returns for
 * b_hat[..][i]: both are the canonical representative of the same residue.  What is saved is the
 * work: a is read once and each of its terms transformed once, terms + comps transforms per limb
 * polynomial where comps mac_ntt calls run comps (terms + 1).  comps = 1 is the context's mac_ntt
 * itself (the k_rns_mac / k_rnsmp_mac path, no other kernel); comps = 2 is the new kernels.
 *
 * c's layout is the one nttmul_ks_moddown_device reads with batch * comps polynomials: the hybrid
 * key switch of nttmul_ks.h is modup, one macn_ntt (comps = 2, shared = 1, terms = dnum) and one
 * moddown over batch * 2, which writes the (c_0, c_1) pair [batch][2][L][n] with nothing laid out
 * again in between.  That is three launches at n <= 4096 and five above it.
 *
 * Range contract.  Per arithmetic class it is k_mac's (csrc/mac_dev.hpp), per accumulator: every
 * word of a and of b_hat canonical (below its own limb's modulus); a transformed word x in [0, 2q)
 * (32-bit words) or [0, 4q) (64-bit words) is read by every component and written by none; each
 * component's accumulator stays canonical (32-bit words) or in [0, 2q) (64-bit words) by one
 * conditional subtraction per term, exactly as the single accumulator of mac_ntt.  b_hat is read
 * as it is: any canonical vector is accepted, whether or not it is a transform.
 *
 * Status, all decided before any device access.  NTTMUL_EINVAL: a NULL context, terms = 0,
 * comps = 0 or comps > NTTMUL_MACN_MAX_COMPS, a NULL operand with batch > 0.  batch = 0 is a
 * successful no-op.  NTTMUL_ENODEV as in nttmul.h (no device, or `dev` not one of the context's).
 * With NTTMUL_FLAG_VALIDATE the words of a and of all of b_hat are range-checked on the device
 * first (the k_rns_check_range of nttmul_rns.h) and the call returns NTTMUL_ERANGE without
 * touching c; the call then waits for the check.  The error text is the context's
 * (nttmul_rns_last_error / nttmul_rnsmp_last_error).
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_macn_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  c must overlap neither a nor b_hat.
 *   Footprint.  A call writes exactly batch * comps * limbs * n words of c and nothing else in
 *     caller memory; inputs are never written.
 *   Addressing.  Polynomial, term and component offsets are computed in 64 bits.
 *
 * Launches.  nttmul_rns: one.  nttmul_rnsmp: three per sub-batch for any terms and comps -- the
 * context's own k_rnsmp_cols_fwd over batch * terms polynomials, k_rnsmp_macn, the context's own
 * k_rnsmp_cols_inv over batch * comps polynomials, which writes c.  The sub-batch is the largest
 * polynomial count for which neither batch * terms nor batch * comps polynomials exceed the
 * context's scratch_mb (never less than one); the scratch grows, is handed between streams and is
 * freed exactly as for the context's other operations, and a context still serves one host thread
 * at a time.
 *
 * Out of scope here:
 *   - more than two components;
 *   - NTT-domain a (the hoisted rotation is include/nttmul_hoist.h, lib/libnttmul_hoist.so: a
 *     pointwise mac on transformed digits with the automorphism fused into their load);
 *   - a fused modup -> mac or mac -> moddown;
 *   - one call that runs the whole key switch on scratch of its own;
 *   - a bench.py mode (tools/bench_macn.py measures these calls).
 */
#ifndef NTTMUL_MACN_H
#define NTTMUL_MACN_H

#include "nttmul_ks.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NTTMUL_MACN_MAX_COMPS 2

/* Device-resident operands of the context's word size on HIP device `dev` (one of the context's),
 * enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE they wait for the range check). */
int nttmul_rns_macn_ntt_device(nttmul_rns *r, void *c, const void *a, const void *b_hat,
                               size_t batch, uint32_t terms, uint32_t comps, int shared, int dev,
                               void *stream);
int nttmul_rnsmp_macn_ntt_device(nttmul_rnsmp *r, void *c, const void *a, const void *b_hat,
                                 size_t batch, uint32_t terms, uint32_t comps, int shared, int dev,
                                 void *stream);

/* Host buffers.  Deliberately simple, as nttmul_rns_mac_ntt: the context's first device, device
 * buffers owned by the call, the device path, a copy back and a synchronise. */
int nttmul_rns_macn_ntt(nttmul_rns *r, void *c, const void *a, const void *b_hat, size_t batch,
                        uint32_t terms, uint32_t comps, int shared);
int nttmul_rnsmp_macn_ntt(nttmul_rnsmp *r, void *c, const void *a, const void *b_hat, size_t batch,
                          uint32_t terms, uint32_t comps, int shared);

/* The kernel(s) a call with `comps` dispatches to, in the format of nttmul_rns_kernel_name and
 * nttmul_rnsmp_kernel_name: "k_rns_macn<Arith32P,u32,12,2>", or "k_rnsmp_cols_fwd<Arith64,u64,4,1>
 * + k_rnsmp_macn<Arith64,u64,4,2> + k_rnsmp_cols_inv<Arith64,u64,4>" (one string);
 * comps = 1 names the context's mac.  Returns the untruncated length, or a negative status. */
int nttmul_rns_macn_kernel_name(const nttmul_rns *r, uint32_t comps, char *buf, size_t cap);
int nttmul_rnsmp_macn_kernel_name(const nttmul_rnsmp *r, uint32_t comps, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_MACN_H */
