/*
 * nttmul_ctlin.h — the steps between the keyed calls, on NTT-domain limbs: weighted sums of
 * ciphertexts (ciphertext + ciphertext, - ciphertext, ciphertext x constant, ciphertext x
 * plaintext, pt o ct + ct', a plaintext dot product, + plaintext, + constant) in one launch, and
 * all three terms of a ciphertext product: lib/libnttmul_ctlin.so (not libnttmul_level.so, nor any
 * of the older libraries).
 *
 * libnttmul_ctlin.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h, nttmul_rns.h,
 * nttmul_bconv.h, nttmul_rnsmp.h, nttmul_galois.h, nttmul_ks.h, nttmul_macn.h, nttmul_hoist.h,
 * nttmul_mdntt.h, nttmul_ksntt.h, nttmul_lintrans.h, nttmul_ctmul.h, nttmul_xconv.h and
 * nttmul_level.h with the same kernels, plus the entry points below and the kernels behind them
 * (csrc/ctlin_dev.hpp k_ctlin_combine, k_ctlin_tensor).
 *
 * An nttmul_ctlin context holds, for one power-of-two n in 256 .. 65536, one basis of L moduli
 * q_0 .. q_{L-1} of one word class, of any sizes and in any order.  A caller who works in Q u P
 * passes the L + K moduli as one basis.  Every limb of every operand is a transform: bit-reversed
 * NTT order, canonical words, what nttmul_rns_forward / nttmul_rnsmp_forward write for that
 * limb's modulus.  The context needs no twiddles and no scratch.
 *
 *   combine  terms[0 .. nterms): {x, w, kind}; x [batch][comps][L][n] (or NULL), comps in 1 .. 3
 *         -> out [batch][comps][L][n]
 *
 *              out[p][c][l][j] = (sum over i of W_i[l][j] X_i[p][c][l][j]) mod q_l
 *
 *            W_i is 1 for NTTMUL_CTLIN_ONE, w[l] for NTTMUL_CTLIN_SCALAR (w: [L] words, one
 *            constant per limb) and w[l][j] for NTTMUL_CTLIN_PLAIN (w: [L][n], an NTT-domain
 *            plaintext, shared by the batch and by the components).  X_i is x[p][c][l][j]; a term
 *            with x == NULL is a constant term, whose X is 1 for c = 0 and 0 otherwise: with PLAIN
 *            it adds a plaintext to component 0, with SCALAR a constant (the transform of a
 *            constant is the same word in every slot).  Subtraction and negation are SCALAR with
 *            q_l - 1.  The `terms` array is host memory in both forms and is read before the call
 *            returns; x, w and out are device memory in the _device form.
 *
 *   tensor   x_hat, y_hat [batch][pairs][2][L][n]
 *         -> d_hat [batch][3][L][n]
 *
 *              d_0 = sum over s of x[s][0] o y[s][0]
 *              d_1 = sum over s of (x[s][0] o y[s][1] + x[s][1] o y[s][0])
 *              d_2 = sum over s of x[s][1] o y[s][1]
 *
 *            all three terms of the product, what BFV needs in Q u B between nttmul_xconv_extend
 *            and nttmul_xconv_moddown.  y_hat == x_hat (the same pointer) is the square.  d_2 is
 *            nttmul_ctmul_high's output bit for bit and feeds nttmul_ksntt_modup as it does; (d_0,
 *            d_1) join the ModDown output through one combine.  With combine(comps = 3), sums of
 *            products of different ciphertexts are relinearised once: add the tensors first.
 *
 * Outputs are canonical; a modular sum of exact products is exact, so the definitions pin every
 * word.  Each operation is one element-wise launch at every n over all limbs and all terms.
 *
 * Word size, as nttmul_rns.h: every modulus below 2^31 (32-bit words) or every one in
 * [2^32, 2^62) (64-bit words); nttmul_ctlin_info.word_bits says which.
 *
 * Status, all decided before any device access.  nttmul_ctlin_create: nttmul_galois_create's, in
 * the same order.  combine, in this order: NTTMUL_EINVAL for a NULL context; nterms 0 or above
 * NTTMUL_CTLIN_MAX_TERMS; comps 0 or above NTTMUL_CTLIN_MAX_COMPS; NULL terms; then per term, in
 * index order: a kind above 2, a non-zero reserved, ONE with a non-NULL w, SCALAR or PLAIN with a
 * NULL w, ONE with a NULL x; then a NULL out with batch > 0.  batch = 0 is then a successful
 * no-op.  tensor: nttmul_ctmul_high's (a NULL context; pairs = 0; a NULL d_hat, x_hat or y_hat
 * with batch > 0).  NTTMUL_ENODEV as in nttmul.h (no device, or `dev` not one of the context's).
 * NTTMUL_FLAG_VALIDATE range-checks every x and every w over its limbs on the device first (the
 * k_rns_check_range of nttmul_rns.h) and returns NTTMUL_ERANGE without touching the output; the
 * call then waits for the check.
 *
 * Caller memory, as in nttmul.h (tests/test_gpu_ctlin_footprint.py).
 *   Alignment.  Operands need the alignment of their word only.
 *   Aliasing.  combine: out may be exactly one or more of the x_i (the same pointer: ct += ..);
 *     every other overlap of out with an x or a w is forbidden.  tensor: the output must overlap
 *     no input.  Inputs may alias each other.
 *   Footprint.  combine writes exactly batch * comps * L * n words of out, tensor exactly
 *     batch * 3 * L * n words of d_hat, and nothing else in caller memory; the inputs are never
 *     written (but for an x that is out).
 *   Addressing.  Every offset is computed in 64 bits.
 *
 * Out of scope here:
 *   - a plaintext or a scalar per batch entry, and a weight per component;
 *   - more than NTTMUL_CTLIN_MAX_TERMS terms or NTTMUL_CTLIN_MAX_COMPS components;
 *   - rotations (nttmul_lintrans.h) and anything with a key;
 *   - coefficient-order operands;
 *   - cyclic contexts (NTTMUL_FLAG_CYCLIC), the class 2^31 <= q < 2^32;
 *   - a chunked or multi-device host path (the host forms below are deliberately simple);
 *   - a bench.py mode (tools/bench_ctlin.py measures these calls).
 */
#ifndef NTTMUL_CTLIN_H
#define NTTMUL_CTLIN_H

#include "nttmul_level.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nttmul_ctlin nttmul_ctlin;

typedef struct {
  uint32_t n, logn, limbs;
  uint32_t word_bits;  /* 32: every modulus < 2^31; 64: every modulus >= 2^32.  The word of every operand */
  int ndev;
} nttmul_ctlin_info;

#define NTTMUL_CTLIN_MAX_TERMS 16
#define NTTMUL_CTLIN_MAX_COMPS 3

#define NTTMUL_CTLIN_ONE 0    /* weight 1 */
#define NTTMUL_CTLIN_SCALAR 1 /* w: [L] words, one constant per limb */
#define NTTMUL_CTLIN_PLAIN 2  /* w: [L][n], an NTT-domain plaintext, shared by batch and components */

typedef struct {
  const void *x; /* [batch][comps][L][n], or NULL: the constant term (SCALAR and PLAIN only) */
  const void *w; /* by kind; NULL for NTTMUL_CTLIN_ONE */
  uint32_t kind;
  uint32_t reserved; /* 0 */
} nttmul_ctlin_term;

#define NTTMUL_CTLIN_COMBINE 0
#define NTTMUL_CTLIN_TENSOR 1

/* params: n, ndev, first_dev and flags as for nttmul_galois_create (params_size likewise);
 * params->q and params->psi must be 0; scratch_mb and the dispatch knobs are ignored.
 * q[0 .. limbs): the basis, in limb order. */
int nttmul_ctlin_create(nttmul_ctlin **cl, const nttmul_params *params, size_t params_size,
                        const uint64_t *q, uint32_t limbs);
void nttmul_ctlin_destroy(nttmul_ctlin *cl);
const char *nttmul_ctlin_last_error(const nttmul_ctlin *cl);
int nttmul_ctlin_get_info(const nttmul_ctlin *cl, nttmul_ctlin_info *info);

/* Device-resident operands of info.word_bits-wide words on HIP device `dev` (one of the
 * context's), enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE they wait for the
 * range check). */
int nttmul_ctlin_combine_device(nttmul_ctlin *cl, void *out, const nttmul_ctlin_term *terms,
                                uint32_t nterms, size_t batch, uint32_t comps, int dev,
                                void *stream);
int nttmul_ctlin_tensor_device(nttmul_ctlin *cl, void *d_hat, const void *x_hat, const void *y_hat,
                               size_t batch, uint32_t pairs, int dev, void *stream);

/* Host buffers.  Deliberately simple, as nttmul_ctmul_high: the context's first device, device
 * buffers owned by the call (one per distinct x and w pointer; out is read from the host first
 * when it is one of the x), the device path, a copy back and a synchronise. */
int nttmul_ctlin_combine(nttmul_ctlin *cl, void *out, const nttmul_ctlin_term *terms,
                         uint32_t nterms, size_t batch, uint32_t comps);
int nttmul_ctlin_tensor(nttmul_ctlin *cl, void *d_hat, const void *x_hat, const void *y_hat,
                        size_t batch, uint32_t pairs);

/* The kernel `op` (NTTMUL_CTLIN_COMBINE with comps in 1 .. 3, or NTTMUL_CTLIN_TENSOR, comps
 * ignored) launches, in the format of nttmul_ctmul_kernel_name: "k_ctlin_combine<Arith64,u64,2>".
 * Returns the untruncated length, or a negative status (NTTMUL_EINVAL for another op or comps). */
int nttmul_ctlin_kernel_name(const nttmul_ctlin *cl, int op, uint32_t comps, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_CTLIN_H */
