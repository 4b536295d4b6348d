// mac_dev.hpp — the fused multiply-accumulate against NTT-domain operands (include/nttmul_mac.h,
// lib/libnttmul_mac.so only):  c[p] = INTT( sum_t NTT(a[p][t]) o b_hat[p or 0][t] ),  n <= 4096.
// Device code; its launchers are in mac.hip.  It reuses the transform stages, exchanges and launch
// helpers of kernels_dev.hpp unchanged and adds no function to them.
#pragma once
#include "kernels_dev.hpp"

namespace nttmul {

// acc + m mod q in the range the class's inverse butterflies read (k_mac's range contract)
__device__ __forceinline__ uint32_t mac_add(const Arith32P &ar, uint32_t acc, uint32_t m) {
  return Arith32P::csub(acc + m, ar.q);  // [0, q) + [0, q) < 2^32 for q < 2^31
}
__device__ __forceinline__ uint32_t mac_add(const Arith32W &ar, uint32_t acc, uint32_t m) {
  return ar.addmod(acc, m);  // the 33-bit sum of two canonical values, by its carry
}
__device__ __forceinline__ uint64_t mac_add(const Arith64 &ar, uint64_t acc, uint64_t m) {
  return Arith64::csub(acc + m, 2 * ar.q);  // [0, 2q) + [0, 2q) < 2^64 for q < 2^62
}

// One thread group per output polynomial with the Groups<LOGS> register layout (16 coefficients
// per lane, PB = 256 / (n / 16) polynomials per 256-thread block, as k_xform).  Per term: a[p][t]
// is loaded in layout 0 (standard order), transformed completely (fwd_all with SKIP = 0: b_hat is
// a full transform, so the product kernel's base blocks do not apply), multiplied by the 16 words
// of b_hat at the addresses k_xform<..., DIR = 0> stores to (layout G - 1), and added to the
// accumulator.  One inverse transform of the sum, canonical store.
//
// Scale: P comes from make_params, F = n^-1 R.  Each Montgomery product carries one R^-1, so does
// their sum, and F in the last inverse stage cancels it together with n^-1.
//
// Range contract, per arithmetic class (x = fwd_all's output, b = a word of b_hat, m = mont(x, b),
// acc = the accumulator):
//   Arith32P  x in [0, 2q) (CT outputs; mont reduces its first operand), b canonical, m in [0, q).
//             acc stays canonical: acc + m < 2q < 2^32 for every q < 2^31, one conditional
//             subtraction per term.  The GS inverse reads canonical values.
//   Arith32W  x, b, m canonical (the class never leaves [0, q)); acc = addmod(acc, m), canonical.
//   Arith64   x in [0, 4q) (Harvey CT), b canonical; mont canonicalises both and returns [0, 2q).
//             acc stays in [0, 2q): acc + m < 4q < 2^64 for q < 2^62, one conditional subtraction
//             of 2q per term.  The Harvey GS inverse reads [0, 2q) (it forms x - y + 2q).
// b_hat is read as it is: any canonical vector is accepted, whether or not it is a transform.
//
// bpolys: polynomials of b_hat per output polynomial, `terms`, or 0 when one [terms][n] operand
// is shared by the batch (the shared form is a stride, not a second kernel).  a and c are touched
// once (non-temporal); b_hat loads stay temporal, because a shared operand is re-read by every
// block.  Threads past the batch end read unit 0 and never store.
template <class A, class TIn, class TOut, int LOGS>
__global__ __launch_bounds__(256) void k_mac(KParams<A> P, const TIn *__restrict__ a,
                                             const TIn *__restrict__ bh, TOut *__restrict__ c,
                                             size_t batch, uint32_t terms, uint32_t bpolys) {
  using W = typename A::word;
  using Gr = Groups<LOGS>;
  constexpr int N = Gr::N, TP = N / 16, PB = 256 / TP, G = Gr::G, NP = Gr::NP;
  __shared__ W lds[PB][NP];
  const int pb = threadIdx.x / TP, j = threadIdx.x % TP;
  const size_t p = (size_t)blockIdx.x * PB + pb;
  const bool live = p < batch;
  const size_t pl = live ? p : 0;
  const TIn *ap = a + pl * terms * N + Gr::base(0, j);
  const TIn *bp = bh + pl * bpolys * N + Gr::base(G - 1, j);
  W acc[16], y[16];
#pragma unroll
  for (int k = 0; k < 16; k++) acc[k] = 0;
  for (uint32_t t = 0; t < terms; t++, ap += N, bp += N) {
    W x[16], bv[16];
#pragma unroll
    for (int k = 0; k < 16; k++) x[k] = to_word<W>(ld_stream<true>(ap + Gr::off(0, k)));
    // 32-bit words: b_hat's loads fly during the transform.  64-bit words load them after it:
    // 32 more live registers through the transform put the kernel past 256 (one wave per SIMD)
    constexpr bool kEarlyB = sizeof(W) == 4;
    if constexpr (kEarlyB) {
#pragma unroll
      for (int k = 0; k < 16; k++) bv[k] = to_word<W>(bp[Gr::off(G - 1, k)]);
    }
    TwPair<W> zw[16];
    fwd_all<A, LOGS, 0, 1, 0>(P.ar, x, y, lds[pb], P.fw, j, 0, 0, zw);
    if constexpr (!kEarlyB) {
#pragma unroll
      for (int k = 0; k < 16; k++) bv[k] = to_word<W>(bp[Gr::off(G - 1, k)]);
    }
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = mac_add(P.ar, acc[k], P.ar.mont(x[k], bv[k]));
  }
  inv_all<A, LOGS, G - 1, true, 0>(P, acc, y, lds[pb], P.iw, j, 0, 0);
  if (live) {
    TOut *cp = c + p * N + Gr::base(0, j);
#pragma unroll
    for (int k = 0; k < 16; k++) {
      W v = acc[k];
      if (!A::kInvCanonical) v = P.ar.canon_inv(v);
      st_stream<true>(cp + Gr::off(0, k), (TOut)v);
    }
  }
}

}  // namespace nttmul
