// macn_dev.hpp — the mac against COMPS NTT-domain operands of include/nttmul_macn.h
// (lib/libnttmul_macn.so only):
//   c[p][i][l] = INTT_l( sum_t NTT_l(a[p][t][l]) o b_hat[p or shared][i][t][l] ),  i < COMPS,
// with the forward transforms of a shared by the components.  Device code; its launchers are in
// macn.hip.  k_rns_macn is k_rns_mac's body (rns_dev.hpp) and k_rnsmp_macn is k_rnsmp_mac's row
// pass (rnsmp_dev.hpp) with COMPS accumulators; the column passes above n = 4096 are
// k_rnsmp_cols_fwd and k_rnsmp_cols_inv themselves.  It reuses mac_add, fwd_all, inv_all and the
// load / store helpers unchanged and adds no function to kernels_dev.hpp or mac_dev.hpp.
//
// Per term: one load of a[p][t], one fwd_all; then per component the 16 words of that component's
// b_hat at the layout G - 1 addresses, one mont and one mac_add.  After the term loop, per
// component: one inv_all and one store.  Component i of b_hat starts i terms polynomials after
// component 0; bpolys (polynomials of b_hat per output polynomial) is COMPS terms, or 0 when one
// [COMPS][terms][limbs][n] operand is shared by the batch.
//
// Range contract, per arithmetic class and per accumulator: k_mac's (mac_dev.hpp).  x = fwd_all's
// output is read by every component's mont and written by none, so component i's accumulator
// sees exactly the sequence of (x, b) pairs k_rns_mac's sees for b_hat[..][i]:
//   Arith32P  x in [0, 2q), b canonical, m = mont(x, b) in [0, q); acc[i] stays canonical
//             (acc + m < 2q < 2^32, one conditional subtraction per term and component).
//   Arith64   x in [0, 4q), b canonical, m in [0, 2q); acc[i] stays in [0, 2q) (acc + m < 4q < 2^64,
//             one conditional subtraction of 2q per term and component), which the Harvey GS
//             inverse reads.
// k_rnsmp_macn's forward rows read the column pass's lazy words, as k_rnsmp_mac's do.
//
// Registers.  32-bit words keep k_mac's early b_hat loads, for all components (16 COMPS words in
// flight through the transform).  64-bit words load each component's 16 words after the
// transform and just before their products, so that at most one component's b_hat is live; all
// COMPS accumulators stay in registers through the transforms (form (a) of DESIGN.md §4: 204 to
// 230 VGPRs, two waves per SIMD, no private segment; parking one in LDS changed neither the
// register count nor the time).  Each component's row is stored as soon as its inverse is done,
// before the next component's inverse starts.
#pragma once
#include "rnsmp_dev.hpp"
#include "rns_dev.hpp"

namespace nttmul {

// f(integral_constant<int, I>) for I = 0 .. COMPS - 1: the components by compile-time recursion,
// not by a loop.  A loop over components around the 64-bit products is not fully unrolled (as
// base_mult_rec's note in kernels_dev.hpp says of loops that hold inline asm), and the
// accumulators, indexed at run time, would then live in a private segment.
template <int COMPS, int I = 0, class F>
__device__ __forceinline__ void each_comp(F &&f) {
  if constexpr (I < COMPS) {
    f(std::integral_constant<int, I>{});
    each_comp<COMPS, I + 1>(f);
  }
}

// n <= 4096.  Grid (ceil(batch / PB), limbs), as k_rns_mac.  Polynomial (p, t) of a starts at word
// ((p terms + t) L + l) n, (p, i, t) of b_hat at (((p bpolys) + i terms + t) L + l) n and (p, i)
// of c at ((p COMPS + i) L + l) n, all in 64 bits.  tab: make_params (scale F).
template <class A, class IO, int LOGS, int COMPS>
__global__ __launch_bounds__(256) void k_rns_macn(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const IO *__restrict__ a, const IO *__restrict__ bh, IO *__restrict__ c, size_t batch,
    uint32_t terms, uint32_t bpolys, uint32_t limbs) {
  using W = typename A::word;
  using Gr = Groups<LOGS>;
  constexpr int N = Gr::N, TP = N / 16, PB = 256 / TP, G = Gr::G, NP = Gr::NP;
  static_assert(COMPS >= 2, "COMPS = 1 is k_rns_mac");
  __shared__ W lds[PB][NP];
  const uint32_t l = blockIdx.y;
  const KParams<A> P = limb_params<A, N>(tab, tw, l);
  const int pb = threadIdx.x / TP, j = threadIdx.x % TP;
  const size_t p = (size_t)blockIdx.x * PB + pb;
  const bool live = p < batch;
  const size_t pl = live ? p : 0, step = (size_t)limbs * N, cstep = step * terms;
  const IO *ap = a + (pl * terms * limbs + l) * N + Gr::base(0, j);
  const IO *bp = bh + (pl * bpolys * limbs + l) * N + Gr::base(G - 1, j);
  W acc[COMPS][16], y[16];
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
#pragma unroll
    for (int k = 0; k < 16; k++) acc[i][k] = 0;
  });
  for (uint32_t t = 0; t < terms; t++, ap += step, bp += step) {
    W x[16], bv[COMPS][16];
#pragma unroll
    for (int k = 0; k < 16; k++) x[k] = to_word<W>(ld_stream<true>(ap + Gr::off(0, k)));
    // (k_mac: 32-bit words load b_hat before the transform, 64-bit words after it)
    constexpr bool kEarlyB = sizeof(W) == 4;
    if constexpr (kEarlyB) {
      each_comp<COMPS>([&](auto ci) {
        constexpr int i = decltype(ci)::value;
#pragma unroll
        for (int k = 0; k < 16; k++) bv[i][k] = to_word<W>(bp[i * cstep + Gr::off(G - 1, k)]);
      });
    }
    TwPair<W> zw[16];
    fwd_all<A, LOGS, 0, 1, 0>(P.ar, x, y, lds[pb], P.fw, j, 0, 0, zw);
    each_comp<COMPS>([&](auto ci) {
      constexpr int i = decltype(ci)::value;
      if constexpr (!kEarlyB) {
#pragma unroll
        for (int k = 0; k < 16; k++) bv[i][k] = to_word<W>(bp[i * cstep + Gr::off(G - 1, k)]);
      }
#pragma unroll
      for (int k = 0; k < 16; k++)
        acc[i][k] = mac_add(P.ar, acc[i][k], P.ar.mont(x[k], bv[i][k]));
    });
  }
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
    inv_all<A, LOGS, G - 1, true, 0>(P, acc[i], y, lds[pb], P.iw, j, 0, 0);
    if (live) {
      IO *cp = c + ((p * COMPS + i) * limbs + l) * N + Gr::base(0, j);
#pragma unroll
      for (int k = 0; k < 16; k++) {
        W v = acc[i][k];
        if (!A::kInvCanonical) v = P.ar.canon_inv(v);
        st_stream<true>(cp + Gr::off(0, k), (IO)v);
      }
    }
  });
}

// 4096 < n <= 65536: the row pass between k_rnsmp_cols_fwd<.., 1> over batch terms units and
// k_rnsmp_cols_inv over batch COMPS units.  Grid (batch << L1, limbs), as k_rnsmp_mac.  Row
// (p, row) of limb l: per term the column-passed row of a[p][t] from the scratch ta
// ([batch terms][limbs][n]); per component the row of b_hat[p or shared][i][t] from caller
// memory; COMPS rows to the output scratch tc ([batch COMPS][limbs][n], the layout of c, which
// k_rnsmp_cols_inv then writes in place of it).  tab: make_params (F is in k_rnsmp_cols_inv).
template <class A, class IO, int L1, int COMPS>
__global__ __launch_bounds__(256) void k_rnsmp_macn(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const typename A::word *__restrict__ ta, const IO *__restrict__ bh,
    typename A::word *__restrict__ tc, size_t units, uint32_t terms, uint32_t bpolys,
    uint32_t limbs) {
  using W = typename A::word;
  using Gr = Groups<kMpLogs>;
  constexpr int N = Gr::N, TP = N / 16, G = Gr::G, NP = Gr::NP;
  static_assert(TP == 256 && COMPS >= 2, "one row of 4096 per workgroup; COMPS = 1 is k_rnsmp_mac");
  __shared__ W lds[NP];
  const uint32_t l = blockIdx.y;
  const KParams<A> P = mp_limb_params<A>(tab, tw, l, kMpLogs + L1);
  const int j = threadIdx.x;
  const size_t u = blockIdx.x;
  if (u >= units) return;  // (grid = units exactly; block-uniform)
  const int row = (int)(u & ((1u << L1) - 1));
  const size_t p = u >> L1, step = (size_t)limbs << (kMpLogs + L1), cstep = step * terms;
  const W *ap = ta + mp_row_word<L1>(p * terms, row, limbs, l) + Gr::base(0, j);
  const IO *bp = bh + mp_row_word<L1>(p * bpolys, row, limbs, l) + Gr::base(G - 1, j);
  W acc[COMPS][16], y[16];
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
#pragma unroll
    for (int k = 0; k < 16; k++) acc[i][k] = 0;
  });
  for (uint32_t t = 0; t < terms; t++, ap += step, bp += step) {
    W x[16], bv[COMPS][16];
#pragma unroll
    for (int k = 0; k < 16; k++) x[k] = ap[Gr::off(0, k)];
    constexpr bool kEarlyB = sizeof(W) == 4;
    if constexpr (kEarlyB) {
      each_comp<COMPS>([&](auto ci) {
        constexpr int i = decltype(ci)::value;
#pragma unroll
        for (int k = 0; k < 16; k++) bv[i][k] = to_word<W>(bp[i * cstep + Gr::off(G - 1, k)]);
      });
    }
    TwPair<W> zw[16];
    fwd_all<A, kMpLogs, 0, 1, 0>(P.ar, x, y, lds, P.fw, j, row, L1, zw);
    each_comp<COMPS>([&](auto ci) {
      constexpr int i = decltype(ci)::value;
      if constexpr (!kEarlyB) {
#pragma unroll
        for (int k = 0; k < 16; k++) bv[i][k] = to_word<W>(bp[i * cstep + Gr::off(G - 1, k)]);
      }
#pragma unroll
      for (int k = 0; k < 16; k++)
        acc[i][k] = mac_add(P.ar, acc[i][k], P.ar.mont(x[k], bv[i][k]));
    });
  }
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
    inv_all<A, kMpLogs, G - 1, false, 0>(P, acc[i], y, lds, P.iw, j, row, L1);
    W *cp = tc + mp_row_word<L1>(p * COMPS + i, row, limbs, l) + Gr::base(0, j);
#pragma unroll
    for (int k = 0; k < 16; k++) cp[Gr::off(0, k)] = acc[i][k];
  });
}

}  // namespace nttmul
