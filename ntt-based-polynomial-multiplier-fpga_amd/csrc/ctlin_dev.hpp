// ctlin_dev.hpp — the kernels of include/nttmul_ctlin.h (lib/libnttmul_ctlin.so only): a weighted
// sum of ciphertexts and the three terms of a ciphertext product.  Device code; the launchers are
// in ctlin.hip.  It reuses mont and canon_inv (modarith.hpp), mac_add (mac_dev.hpp),
// BconvArith<W>::mulc (bconv_dev.hpp), ks_arith (ksntt_dev.hpp) and CtVec (ctmul_dev.hpp)
// unchanged, inside their stated domains, and adds no function to them.
//
//   combine  out[p][c][l][j] = (sum_i W_i[l][j] X_i[p][c][l][j]) mod q_l
//            W_i = 1 (ONE), w_i[l] (SCALAR), w_i[l][j] (PLAIN); X_i = x_i[p][c][l][j], or for a
//            term without an x the constant [c = 0]
//   tensor   d_hat[p][0] = sum_s x[s][0] y[s][0],  d_hat[p][2] = sum_s x[s][1] y[s][1],
//            d_hat[p][1] = sum_s (x[s][0] y[s][1] + x[s][1] y[s][0])       (all [l][j], mod q_l)
//
// Both are k_ctmul_high's stream: element-wise, one launch at every n, no transform, no twiddle, no
// LDS, no barrier, no index table.  Grid (ceil(batch n / VEC / 256), L), the limb's constants by
// blockIdx.y.  A lane takes one vector of 16 bytes (4 words of 32 bits, 2 of 64: CtVec, declared
// with the word's alignment only) at slot j of one batch entry, and it takes that vector for every
// component: a plaintext vector is loaded once and used COMPS times.  Lanes past the last vector
// return at once (no barrier follows).
//
// k_ctlin_combine.  The term descriptors (16 x {x, w, kind}) travel by value in the kernel
// arguments: the loop over the terms and the branch on the kind are wave-uniform, the pointers
// live in SGPRs, a SCALAR's word w[l] is a block-uniform load.  A Montgomery product with a
// plaintext carries R^-1 and a ONE term carries none, so a lane keeps two accumulators per output
// word:
//   a1, at scale 1:    ONE terms by mac_add alone; SCALAR terms as mont(x, s R), with
//                      s R = mont(s, R^2 mod q_l) formed once per term from the limb's constant;
//                      the constant terms (s itself, or the plaintext's word) in component 0;
//   a2, at scale R^-1: PLAIN terms, mont(x, w).
// One mulc by R mod q_l per output word joins them, out = canon_inv(mac_add(a1, mulc(a2, R))); a
// call without a PLAIN term (T.plain = 0, uniform) skips the mulc.  Every x vector of a lane is
// read before its output vector is stored, and a lane reads of every x exactly the words it writes
// of out: out may be one or more of the x (the same pointer), so x and out carry no __restrict__.
//
// k_ctlin_tensor: four loads, four products and three stores per pair and slot; acc =
// mac_add(acc, mont(x, y)) over the pairs, then mulc by R mod q_l.  d_hat[p][2] is k_ctmul_high's
// d2_hat by the same operations in the same order.
//
// Range contract, per arithmetic class (x = a word of an x or of x_hat / y_hat, w = a word of a
// plaintext, s = a SCALAR's word, all canonical by the call's contract):
//   Arith32P  mont reduces its first operand from [0, 2q), the second may be any word below 2q,
//             the result is in [0, q): s R, mont(x, s R) and mont(x, w) are canonical.  mac_add
//             of two canonical words is canonical (their sum < 2q < 2^32), so a1 and a2 stay
//             canonical.  mulc(a2, R mod q) (Plantard, any 32-bit input) is canonical, the join
//             is one more mac_add, and canon_inv of a canonical word is that word.
//   Arith64   mont takes lazy words below 4q, canonicalises both and returns [0, 2q): s R,
//             mont(x, s R) and mont(x, w) are in [0, 2q).  mac_add takes two words in [0, 2q)
//             (a canonical x, s or w is one) and returns [0, 2q): a1 and a2 stay in [0, 2q).
//             mulc (Shoup takes any 64-bit word, one conditional subtraction) is canonical; the
//             join mac_add(a1, .) is in [0, 2q) and canon_inv takes [0, 2q) to [0, q).
//   The sums run over up to 16 terms or over the pairs; no bound on either is needed, every
//   addition is followed by its conditional subtraction.
// Polynomial offsets are 64-bit, slots 32-bit.
#pragma once
#include "ctlin.hpp"
#include "ctmul_dev.hpp"

namespace nttmul {

// Grid (ctlin_plan.hpp ctlin_grid wgx, L); vectors = batch n / VEC.  Vector g of limb l is words
// [j, j + VEC) of batch entry p = g / (n / VEC), j = (g mod (n / VEC)) VEC: (p, c) of every x and
// of out starts at word ((p COMPS + c) L + l) n, limb l of a plaintext at l n, all in 64 bits.
// to: BconvTo<W>[..] whose (v, vs) is the pair of R mod q_l; lc: ClLimb<W>[L].
template <class A, class IO, int COMPS>
__global__ __launch_bounds__(256) void k_ctlin_combine(
    const BconvTo<typename A::word> *__restrict__ to,
    const ClLimb<typename A::word> *__restrict__ lc, const ClTerms T, IO *out, size_t vectors,
    uint32_t L, uint32_t logn) {
  using W = typename A::word;
  constexpr int VEC = 16 / sizeof(IO);
  constexpr uint32_t LGV = VEC == 4 ? 2 : 1;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= vectors) return;
  const uint32_t l = blockIdx.y;
  const BconvTo<W> C = to[l];
  const A ar = ks_arith<A>(C);
  const W r2 = lc[l].r2;
  const uint32_t lgp = logn - LGV;  // vectors of a polynomial
  const size_t p = g >> lgp;
  const uint32_t j = (uint32_t)(g & (((size_t)1 << lgp) - 1)) << LGV;
  const size_t comp = (size_t)L << logn;  // a component of a batch entry
  const size_t xo = ((p * COMPS * L + l) << logn) + j;
  const size_t wo = ((size_t)l << logn) + j;
  W a1[COMPS][VEC], a2[COMPS][VEC];
#pragma unroll
  for (int c = 0; c < COMPS; c++)
#pragma unroll
    for (int k = 0; k < VEC; k++) a1[c][k] = a2[c][k] = 0;
  for (uint32_t i = 0; i < T.nterms; i++) {
    // (all three are wave-uniform)
    const IO *x = (const IO *)T.x[i], *w = (const IO *)T.w[i];
    const uint32_t kind = T.kind[i];
    if (!x) {  // the constant term: component 0 only
      if (kind == NTTMUL_CTLIN_SCALAR) {
        const W s = to_word<W>(w[l]);
#pragma unroll
        for (int k = 0; k < VEC; k++) a1[0][k] = mac_add(ar, a1[0][k], s);
      } else {
        const CtVec<IO> pv = *(const CtVec<IO> *)(w + wo);
#pragma unroll
        for (int k = 0; k < VEC; k++) a1[0][k] = mac_add(ar, a1[0][k], to_word<W>(pv.w[k]));
      }
      continue;
    }
    CtVec<IO> xv[COMPS];
#pragma unroll
    for (int c = 0; c < COMPS; c++) xv[c] = *(const CtVec<IO> *)(x + xo + c * comp);
    if (kind == NTTMUL_CTLIN_ONE) {
#pragma unroll
      for (int c = 0; c < COMPS; c++)
#pragma unroll
        for (int k = 0; k < VEC; k++) a1[c][k] = mac_add(ar, a1[c][k], to_word<W>(xv[c].w[k]));
    } else if (kind == NTTMUL_CTLIN_SCALAR) {
      const W sr = ar.mont(to_word<W>(w[l]), r2);  // s R
#pragma unroll
      for (int c = 0; c < COMPS; c++)
#pragma unroll
        for (int k = 0; k < VEC; k++)
          a1[c][k] = mac_add(ar, a1[c][k], ar.mont(to_word<W>(xv[c].w[k]), sr));
    } else {
      const CtVec<IO> pv = *(const CtVec<IO> *)(w + wo);
#pragma unroll
      for (int c = 0; c < COMPS; c++)
#pragma unroll
        for (int k = 0; k < VEC; k++)
          a2[c][k] =
              mac_add(ar, a2[c][k], ar.mont(to_word<W>(xv[c].w[k]), to_word<W>(pv.w[k])));
    }
  }
#pragma unroll
  for (int c = 0; c < COMPS; c++) {
    CtVec<IO> o;
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      W v = a1[c][k];
      if (T.plain) v = mac_add(ar, v, BconvArith<W>::mulc(a2[c][k], C.v, C.vs, C.c));  // a2 R
      o.w[k] = (IO)ar.canon_inv(v);
    }
    *(CtVec<IO> *)(out + xo + c * comp) = o;
  }
}

// Grid and vectors as above.  (p, s, i) of x_hat and y_hat starts at word
// (((p pairs + s) 2 + i) L + l) n, (p, c) of d_hat at ((p 3 + c) L + l) n, all in 64 bits.
// to: the context's BconvTo<W> table.
template <class A, class IO>
__global__ __launch_bounds__(256) void k_ctlin_tensor(
    const BconvTo<typename A::word> *__restrict__ to, const IO *xh, const IO *yh,
    IO *__restrict__ d, size_t vectors, uint32_t pairs, uint32_t L, uint32_t logn) {
  using W = typename A::word;
  constexpr int VEC = 16 / sizeof(IO);
  constexpr uint32_t LGV = VEC == 4 ? 2 : 1;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= vectors) return;
  const uint32_t l = blockIdx.y;
  const BconvTo<W> C = to[l];
  const A ar = ks_arith<A>(C);
  const uint32_t lgp = logn - LGV;  // vectors of a polynomial
  const size_t p = g >> lgp;
  const uint32_t j = (uint32_t)(g & (((size_t)1 << lgp) - 1)) << LGV;
  const size_t half = (size_t)L << logn;  // a component
  const size_t xo = ((p * pairs * 2 * L + l) << logn) + j;
  W d0[VEC], d1[VEC], d2[VEC];
#pragma unroll
  for (int k = 0; k < VEC; k++) d0[k] = d1[k] = d2[k] = 0;
  for (uint32_t q = 0; q < pairs; q++) {
    const size_t o = xo + (size_t)q * 2 * half;
    const CtVec<IO> x0 = *(const CtVec<IO> *)(xh + o), x1 = *(const CtVec<IO> *)(xh + o + half);
    const CtVec<IO> y0 = *(const CtVec<IO> *)(yh + o), y1 = *(const CtVec<IO> *)(yh + o + half);
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      const W a0 = to_word<W>(x0.w[k]), a1 = to_word<W>(x1.w[k]);
      const W b0 = to_word<W>(y0.w[k]), b1 = to_word<W>(y1.w[k]);
      d0[k] = mac_add(ar, d0[k], ar.mont(a0, b0));
      d1[k] = mac_add(ar, d1[k], ar.mont(a0, b1));
      d1[k] = mac_add(ar, d1[k], ar.mont(a1, b0));
      d2[k] = mac_add(ar, d2[k], ar.mont(a1, b1));
    }
  }
  CtVec<IO> o0, o1, o2;
#pragma unroll
  for (int k = 0; k < VEC; k++) {
    o0.w[k] = (IO)BconvArith<W>::mulc(d0[k], C.v, C.vs, C.c);  // acc R mod q
    o1.w[k] = (IO)BconvArith<W>::mulc(d1[k], C.v, C.vs, C.c);
    o2.w[k] = (IO)BconvArith<W>::mulc(d2[k], C.v, C.vs, C.c);
  }
  IO *dp = d + ((p * 3 * L + l) << logn) + j;
  *(CtVec<IO> *)dp = o0;
  *(CtVec<IO> *)(dp + half) = o1;
  *(CtVec<IO> *)(dp + 2 * half) = o2;
}

}  // namespace nttmul
