/*
 * nttmul_level.h — level views: the key switch, the linear transform and the relinearisation of
 * a context at any level of a modulus chain, reading keys and diagonals made once at the top
 * level: lib/libnttmul_level.so (not libnttmul_xconv.so, nor any of the older libraries).
 *
 * libnttmul_level.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h, nttmul_rns.h,
 * nttmul_bconv.h, nttmul_rnsmp.h, nttmul_galois.h, nttmul_ks.h, nttmul_macn.h, nttmul_hoist.h,
 * nttmul_mdntt.h, nttmul_ksntt.h, nttmul_lintrans.h, nttmul_ctmul.h and nttmul_xconv.h with the
 * same kernels, plus the entry points below and the kernels behind them (csrc/level_dev.hpp
 * k_level_mac, k_level_lintrans, k_level_relin, k_level_check_range).  It adds no handle: the
 * calls run on nttmul_ksntt, nttmul_lintrans and nttmul_ctmul contexts created through this
 * library.
 *
 * A context is built for one (Q, P, alpha): one level of a chain.  After a rescale the ciphertext
 * has one limb less, and the dense calls want their key operands dense at that level,
 * [..][terms][L + K][n] with terms = ceil(L / alpha).  Keys and encoded diagonals are made once,
 * for the whole chain q_0 .. q_{L_top - 1}.  Because the gadget of digit d, P (Q/D_d)
 * ((Q/D_d)^-1 mod D_d), is P mod q_i on the limbs of D_d and 0 on every other limb of Q u P, and
 * the digits of q[:L] are a prefix of the digits of q (the last one possibly shorter), the limbs
 * {0 .. L-1} u {L_top .. L_top + K - 1} of the terms 0 .. ceil(L / alpha) - 1 of a top-level key
 * are, word for word, the key made for (q[:L], p, alpha) from the same a and e
 * (tests/test_level_ref.py).  A view reads exactly those words where they lie.
 *
 *   typedef struct { uint32_t top_q_limbs, top_terms; } nttmul_level_view;
 *
 *   a viewed key            [rots][comps][top_terms][top_q_limbs + K][n]   (b_hat; key_hat: [2][..])
 *   a viewed diagonal set   [rots][top_q_limbs + K][n]                     (w_hat; no term index)
 *
 * A context of L <= top_q_limbs limbs of Q and K of P reads limb m of term t of component o at
 * limb top(m) of term t of component o, top(m) = m for m < L and m + (top_q_limbs - L) for
 * m >= L.  Nothing else of the operand is read by the device.  With top_q_limbs = L and
 * top_terms = terms the view is the identity and the call equals the dense call bit for bit.
 *
 * The caller guarantees, and the library cannot check:
 *   - the context's Q is the first L primes of the chain the operand was made for, in its order;
 *   - the context's P is that chain's P, in its order;
 *   - the context's digit width is the one the key was made with (or L, where L is smaller: a
 *     digit is never wider than Q).
 * A view over another chain computes, without an error, something else.
 *
 *   nttmul_ksntt_mac_view        nttmul_ksntt_mac with b_hat viewed
 *   nttmul_lintrans_apply_view   nttmul_lintrans_apply with b_hat and, when given, w_hat viewed;
 *                                one view serves both
 *   nttmul_ctmul_relin_view      nttmul_ctmul_relin with key_hat viewed
 *
 * Every other operand (a_hat, up_hat, c0_hat, x_hat, y_hat, c_hat) is dense at the context's own
 * level, as in the dense call.  The kernels are the dense kernels' bodies with the key addresses
 * formed from two wave-uniform strides and a limb shift; they move the same bytes.
 *
 * Status, all decided before any device access: the dense call's, in its order (nttmul_ksntt.h,
 * nttmul_lintrans.h, nttmul_ctmul.h), then NTTMUL_EINVAL for a NULL view; top_q_limbs below the
 * context's L; top_q_limbs + K above NTTMUL_RNS_MAX_LIMBS; top_terms below the call's terms.
 * batch = 0 is then a successful no-op.  NTTMUL_ENODEV as in nttmul.h.  NTTMUL_FLAG_VALIDATE
 * range-checks the dense operands as the dense call does and a viewed operand over exactly the
 * words the view selects, against the context's own moduli (k_level_check_range); words outside
 * the view are neither read nor checked.  NTTMUL_ERANGE leaves the output untouched.
 *
 * Caller memory, as in the dense calls (tests/test_gpu_level_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  The output must overlap no input.  Inputs may alias each other.
 *   Footprint.  Exactly the dense call's output words are written; the viewed operands are never
 *     written.
 *   Addressing.  Every offset is computed in 64 bits: rots * comps * top_terms *
 *     (top_q_limbs + K) * n may pass 2^32 words.
 *
 * Out of scope here:
 *   - keys of the coefficient-output chains (nttmul_rns_macn_ntt, nttmul_rns_hoist_ntt and their
 *     multi-pass forms);
 *   - sharing twiddles and tables between the contexts of a chain: one context per level stays
 *     the caller's, their tables are small next to the keys;
 *   - a host form that stages only the view's words (the host forms below are deliberately simple
 *     and copy the whole viewed operand to the device, where only the view's words are read);
 *   - a bench.py mode (tools/bench_level.py measures these calls).
 */
#ifndef NTTMUL_LEVEL_H
#define NTTMUL_LEVEL_H

#include "nttmul_xconv.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint32_t top_q_limbs; /* L_top >= the context's L: the limbs of Q the operand was made for */
  uint32_t top_terms;   /* >= terms of the call: the terms (digits) the key was made with */
} nttmul_level_view;

#define NTTMUL_LEVEL_MAC 0
#define NTTMUL_LEVEL_LINTRANS 1
#define NTTMUL_LEVEL_RELIN 2

/* Device-resident operands of the context's word on HIP device `dev` (one of the context's),
 * enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE they wait for the range check).
 * The arguments before `view` are the dense call's. */
int nttmul_ksntt_mac_view_device(nttmul_ksntt *ks, void *c_hat, const void *a_hat,
                                 const void *b_hat, const uint32_t *k, uint32_t rots, size_t batch,
                                 uint32_t terms, uint32_t comps, const nttmul_level_view *view,
                                 int dev, void *stream);
int nttmul_lintrans_apply_view_device(nttmul_lintrans *lt, void *c_hat, const void *a_hat,
                                      const void *b_hat, const void *w_hat, const void *c0_hat,
                                      const uint32_t *k, uint32_t rots, size_t batch,
                                      uint32_t terms, uint32_t comps,
                                      const nttmul_level_view *view, int dev, void *stream);
int nttmul_ctmul_relin_view_device(nttmul_ctmul *ct, void *c_hat, const void *up_hat,
                                   const void *key_hat, const void *x_hat, const void *y_hat,
                                   size_t batch, uint32_t pairs, uint32_t terms,
                                   const nttmul_level_view *view, int dev, void *stream);

/* Host buffers.  Deliberately simple, as the dense host forms: the context's first device, device
 * buffers owned by the call (the viewed operands whole), the device path, a copy back and a
 * synchronise. */
int nttmul_ksntt_mac_view(nttmul_ksntt *ks, void *c_hat, const void *a_hat, const void *b_hat,
                          const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                          uint32_t comps, const nttmul_level_view *view);
int nttmul_lintrans_apply_view(nttmul_lintrans *lt, void *c_hat, const void *a_hat,
                               const void *b_hat, const void *w_hat, const void *c0_hat,
                               const uint32_t *k, uint32_t rots, size_t batch, uint32_t terms,
                               uint32_t comps, const nttmul_level_view *view);
int nttmul_ctmul_relin_view(nttmul_ctmul *ct, void *c_hat, const void *up_hat,
                            const void *key_hat, const void *x_hat, const void *y_hat,
                            size_t batch, uint32_t pairs, uint32_t terms,
                            const nttmul_level_view *view);

/* The kernel the view form `op` (NTTMUL_LEVEL_MAC, NTTMUL_LEVEL_LINTRANS or NTTMUL_LEVEL_RELIN)
 * launches for degree n = 2^logn and word size word_bits (32 or 64), in the format of the
 * siblings: "k_level_mac<Arith64,u64,2>", "k_level_lintrans<Arith32P,u32,1,1>",
 * "k_level_relin<Arith64,u64>".  comps (1 or 2) and weighted are read by the ops that have them.
 * No context and no device is needed.  Returns the untruncated length, or a negative status
 * (NTTMUL_EINVAL for another op, logn outside 8 .. 16, another word size or comps). */
int nttmul_level_kernel_name(int op, uint32_t logn, uint32_t word_bits, uint32_t comps,
                             int weighted, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_LEVEL_H */
