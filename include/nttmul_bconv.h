/*
 * nttmul_bconv.h — RNS base conversion and ModDown in one launch: lib/libnttmul_bconv.so (not one
 * of the three older libraries).
 *
 * libnttmul_bconv.so holds the whole C ABI of include/nttmul.h, nttmul_mac.h and nttmul_rns.h with
 * the same kernels, plus the entry points below and the kernels behind them (csrc/bconv_dev.hpp
 * k_bconv).
 *
 * An nttmul_bconv converter holds two disjoint bases of one word class for one degree n <= 4096:
 * the `from` basis B = (b_0 .. b_{L-1}) and the `to` basis C = (c_0 .. c_{K-1}).  Write B also for
 * the product of the b_i and Bh_i = B / b_i.  Operands are polynomial-major arrays of residue
 * limbs as in nttmul_rns.h, [batch][limbs][n], in coefficient (standard) order: these are not
 * transforms.  Every input word is canonical (below its own limb's modulus) and so is every
 * output word.
 * The moduli of a context may be of any sizes within their word class and in any order
 * (tests/test_gpu_bases.py).
 *
 *   convert   in [batch][L][n] -> out [batch][K][n], the fast base conversion with unreduced alpha:
 *               y_i          = in[p][i][k] (Bh_i^-1 mod b_i) mod b_i
 *               out[p][j][k] = (sum over i of y_i Bh_i) mod c_j
 *             The sum is taken over the integers and equals x + alpha B, where x is the CRT value
 *             of the input in [0, B) and alpha = floor(sum over i of y_i / b_i) is in [0, L): the
 *             result is x mod c_j up to that multiple of B.
 *
 *   moddown   x [batch][K + L][n] -> out [batch][K][n]; the input's limb order is c_0 .. c_{K-1},
 *             then b_0 .. b_{L-1}:
 *               out[p][j][k] = (x[p][j][k] - convert(x[p][K .. K+L))[j][k]) (B^-1 mod c_j) mod c_j
 *             With X the CRT value of the whole input in [0, C B) this is
 *             (floor(X / B) - alpha) mod c_j with the alpha above.  For L = 1, alpha = 0 and the
 *             call is the exact rescale floor(X / b_0).  One launch: the subtraction and the
 *             product by B^-1 are the epilogue of the conversion kernel.
 *
 * Word size, as nttmul_rns.h: every modulus of both bases below 2^31 (32-bit words) or every one
 * in [2^32, 2^62) (64-bit words); nttmul_bconv_info.word_bits says which.
 *
 * Status, all decided before any device access: each basis must be one nttmul_rns_create accepts
 * for this n, with its statuses — NTTMUL_EINVAL for a NULL argument, limbs of 0 or above
 * NTTMUL_RNS_MAX_LIMBS, a modulus nttmul_create would refuse (not prime, not 1 mod 2n, >= 2^62; or
 * an n it refuses), non-zero params->q or params->psi, and a prime that occurs twice, within a
 * basis or in both; NTTMUL_EUNSUPPORTED for a valid n above 4096, NTTMUL_FLAG_CYCLIC, a modulus in
 * [2^31, 2^32) and mixed word classes within or across the two bases.  A call returns
 * NTTMUL_EINVAL for a NULL converter or a NULL operand with batch > 0; batch = 0 is a successful
 * no-op.  NTTMUL_ENODEV as in nttmul.h (no device, or `dev` not one of the converter's).
 *
 * Aliasing: out must not overlap the input.  Operands need the alignment of their word only.
 * Footprint: a call writes exactly batch * to_limbs * n words of out and nothing else in caller
 * memory; the input is never written (tests/test_gpu_footprint.py).
 *
 * NTTMUL_FLAG_VALIDATE range-checks every input word against its own limb's modulus on the device
 * and returns NTTMUL_ERANGE; the call then waits for the check.
 *
 * Out of scope here:
 *   - exact conversion, that is the alpha correction (floating-point as Halevi-Polyakov-Shoup, or
 *     a redundant modulus);
 *   - rounding instead of flooring in moddown (for NTT-domain limbs both are nttmul_xconv.h,
 *     lib/libnttmul_xconv.so);
 *   - NTT-domain inputs, or a fused inverse transform -> convert -> forward transform pipeline
 *     (for ModDown that is nttmul_mdntt.h, lib/libnttmul_mdntt.so);
 *   - n > 4096, the class 2^31 <= q < 2^32, and 64-bit storage of 32-bit limbs;
 *   - a chunked or multi-device host path (the host forms below are deliberately simple);
 *   - a bench.py mode (tools/bench_bconv.py measures these calls).
 */
#ifndef NTTMUL_BCONV_H
#define NTTMUL_BCONV_H

#include "nttmul_rns.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nttmul_bconv nttmul_bconv;

typedef struct {
  uint32_t n, from_limbs, to_limbs;
  uint32_t word_bits;  /* 32: every modulus < 2^31; 64: every modulus >= 2^32.  The word of every operand */
  int ndev;
} nttmul_bconv_info;

/* params: n, ndev, first_dev and flags as for nttmul_rns_create (params_size likewise);
 * params->q and params->psi must be 0.  from_q[0 .. from_limbs) and to_q[0 .. to_limbs): the two
 * bases, in limb order. */
int nttmul_bconv_create(nttmul_bconv **h, const nttmul_params *params, size_t params_size,
                        const uint64_t *from_q, uint32_t from_limbs, const uint64_t *to_q,
                        uint32_t to_limbs);
void nttmul_bconv_destroy(nttmul_bconv *h);
const char *nttmul_bconv_last_error(const nttmul_bconv *h);
int nttmul_bconv_get_info(const nttmul_bconv *h, nttmul_bconv_info *info);

/* Host-only, needs no device: the validation of nttmul_bconv_create with its statuses, and the
 * plain constants a converter's device tables are derived from:
 *   inv[i]                = Bh_i^-1 mod b_i     [from_limbs]
 *   w[i * to_limbs + j]   = Bh_i mod c_j        [from_limbs][to_limbs]
 *   binv[j]               = B^-1 mod c_j        [to_limbs] */
int nttmul_bconv_plan(const nttmul_params *params, size_t params_size, const uint64_t *from_q,
                      uint32_t from_limbs, const uint64_t *to_q, uint32_t to_limbs, uint64_t *inv,
                      uint64_t *w, uint64_t *binv);

/* Device-resident operands of info.word_bits-wide words on HIP device `dev` (one of the
 * converter's), enqueued on `stream`; asynchronous (with NTTMUL_FLAG_VALIDATE they wait for the
 * range check).  One kernel launch each. */
int nttmul_bconv_convert_device(nttmul_bconv *h, void *out, const void *in, size_t batch, int dev,
                                void *stream);
int nttmul_bconv_moddown_device(nttmul_bconv *h, void *out, const void *x, size_t batch, int dev,
                                void *stream);

/* Host buffers.  Deliberately simple, as nttmul_rns_multiply: the converter's first device, device
 * buffers owned by the call, the device path, a copy back and a synchronise. */
int nttmul_bconv_convert(nttmul_bconv *h, void *out, const void *in, size_t batch);
int nttmul_bconv_moddown(nttmul_bconv *h, void *out, const void *x, size_t batch);

/* The kernel an operation dispatches to (op: 0 convert, 1 moddown), in the format of
 * nttmul_kernel_name: "k_bconv<u32,0>", "k_bconv<u64,1>" (word, op).  Returns the untruncated
 * length, or a negative status. */
int nttmul_bconv_kernel_name(const nttmul_bconv *h, int op, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NTTMUL_BCONV_H */
