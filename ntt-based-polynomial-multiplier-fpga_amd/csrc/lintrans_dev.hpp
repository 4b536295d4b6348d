// lintrans_dev.hpp — the kernel of include/nttmul_lintrans.h (lib/libnttmul_lintrans.so only): the
// weighted sum of the rotations of a key switch, formed in Q u P before ModDown.  Device code; its
// launcher is in lintrans.hip.  It reuses mont (modarith.hpp), mac_add (mac_dev.hpp),
// BconvArith<W>::mulc (bconv_dev.hpp), galois_slot (galois_dev.hpp), each_comp (macn_dev.hpp) and
// ks_arith (ksntt_dev.hpp) unchanged, inside their stated domains, and adds no function to them.
//
//   c_hat[p][i][l][j] = (sum_r w_hat[r][l][j] (sum_t a_hat[p][t][l][src_{k_r}(j)] b_hat[r][i][t][l][j]
//                         + [i = 0, l < L] (P mod q_l) c0_hat[p][l][src_{k_r}(j)])) mod m_l
//
// k_lintrans: element-wise, one launch at every n, no transform, no twiddle, no LDS, no barrier and
// no index table.  k_ksntt_mac's gather form (ksntt_dev.hpp: 256 threads, one slot per lane, every
// load of b_hat and every store one word per lane and contiguous over the wave, the load of a_hat
// the same cache lines permuted) with these differences:
//
//   The rotation is a loop inside the kernel, not a grid index.  Grid (workgroups, M).  A lane
//   keeps COMPS x V inner accumulators, reset per rotation and run over the terms with
//   mac_add(ar, acc, ar.mont(x, b)), and COMPS x V outer accumulators.  src_{k_r} is recomputed
//   per rotation with galois_slot from the kernel argument GaloisKs (a scalar load by r).
//
//   c_0 is one more term of component 0 with a constant operand: on the limbs l < L (blockIdx.y,
//   block-uniform), when c0_hat is given (a wave-uniform pointer test),
//   inner[0] = mac_add(inner[0], mont(c0_hat[src], P mod q_l)).  The limbs of P skip it.
//
//   WEIGHTED: outer = mac_add(outer, mont(inner, w)).  The result carries R^-2 and leaves through
//   one mulc by R^2 mod m per output word.  Unweighted: the inner accumulator is not reset between
//   rotations and is the result; it carries R^-1 and leaves through k_ksntt_mac's mulc by R mod m.
//
//   Which slices a workgroup takes.  Batch-sliced (the form the library builds): the V slices are
//   the same 256 slots of V consecutive batch entries.  Every word of b_hat and w_hat is loaded
//   once and used V times, so a term costs V + COMPS loads instead of V (1 + COMPS), the key is
//   re-read from the caches batch / V times instead of batch times, and galois_slot runs once per
//   rotation instead of once per slice.  blockIdx.x = g (n / 256) + s: s the range of 256 slots
//   (the faster index: the n / 256 workgroups that between them read every word of the run's
//   polynomials of a_hat once per rotation are adjacent in dispatch order), g the run of V
//   entries.  Built only for the A/B of tools/bench_lintrans.py: the run as the faster index
//   (NTTMUL_LINTRANS_RUN_FASTEST, blockIdx.x = s groups + g: the workgroups that share a range of
//   b_hat adjacent instead), V = 8 (NTTMUL_LINTRANS_V), and slot-sliced
//   (NTTMUL_LINTRANS_SLOT_SLICED, k_ksntt_mac's form: V consecutive ranges of 256 slots of one
//   polynomial, blockIdx.x V + v over the batch n / 256 slices).  DESIGN.md section 4 records
//   the A/B.
//
// Slices past the end read entry (slice) 0, always valid, instead of branching per load, and never
// store.
//
// Range contract, per arithmetic class (x = a word of a_hat or c0_hat, b = a word of b_hat or
// P mod q_l, w = a word of w_hat, all canonical by the call's contract; in = an inner, out = an
// outer accumulator):
//   Arith32P  m = mont(x, b) in [0, q) (mont reduces its first operand from [0, 2q), the second
//             may be any word below 2q); in = mac_add(in, m) stays canonical (in + m < 2q < 2^32).
//             mont(in, w): in canonical is inside mont's [0, 2q) for its first operand; the
//             product is in [0, q) and out stays canonical the same way.  The one step per output
//             word is mulc(acc, R mod q) or mulc(acc, R^2 mod q) (Plantard, any 32-bit input):
//             canonical.
//   Arith64   m in [0, 2q); in stays in [0, 2q) (in + m < 4q < 2^64, one conditional subtraction
//             of 2q).  mont(in, w): mont takes lazy words below 4q and canonicalises both; the
//             product is in [0, 2q) and out stays in [0, 2q).  mulc (Shoup takes any 64-bit word,
//             one conditional subtraction): canonical.
//   The sums run over rots (terms + 1) <= 16 (terms + 1) addends; no bound on terms is needed,
//   every addition is followed by its conditional subtraction.
// src_k(j) < n by construction, so every gathered word lies in the limb polynomial its base
// addresses.  Polynomial offsets are 64-bit, slots 32-bit.
#pragma once
#include "ksntt_dev.hpp"
#include "lintrans.hpp"

namespace nttmul {

// The three switches of the A/B libraries (Makefile ab-lintrans, measured by tools/bench_lintrans.py
// --lib); the library itself is built with none
#ifdef NTTMUL_LINTRANS_SLOT_SLICED
constexpr bool kLtSlotSliced = true;
#else
constexpr bool kLtSlotSliced = false;
#endif
#ifdef NTTMUL_LINTRANS_RUN_FASTEST
constexpr bool kLtRangeFastest = false;
#else
constexpr bool kLtRangeFastest = true;
#endif
#ifdef NTTMUL_LINTRANS_V
constexpr int kLtV = NTTMUL_LINTRANS_V;
#else
constexpr int kLtV = kLtSlices;
#endif

// Grid (lintrans_plan.hpp lintrans_grid wgx, M).  units: batch entries (batch-sliced) or slices of
// 256 slots (slot-sliced); groups = ceil(units / V).  (p, t) of a_hat starts at word
// ((p terms + t) M + l) n, (r, i, t) of b_hat at (((r COMPS + i) terms + t) M + l) n, r of w_hat
// at (r M + l) n, p of c0_hat at (p L + l) n, (p, i) of c_hat at ((p COMPS + i) M + l) n, all in
// 64 bits.  to: BconvTo<W>[..] over Q u P whose (v, vs) is the pair of R mod m; lc: LtLimb<W>[M].
template <class A, class IO, int COMPS, int WEIGHTED>
__global__ __launch_bounds__(256) void k_lintrans(
    const BconvTo<typename A::word> *__restrict__ to,
    const LtLimb<typename A::word> *__restrict__ lc, const IO *__restrict__ ah,
    const IO *__restrict__ bh, const IO *__restrict__ wh, const IO *__restrict__ c0,
    IO *__restrict__ c, GaloisKs ks, uint32_t rots, size_t units, uint32_t groups, uint32_t terms,
    uint32_t L, uint32_t limbs, uint32_t logn) {
  using W = typename A::word;
  static_assert(COMPS >= 1 && COMPS <= 2, "NTTMUL_MACN_MAX_COMPS");
  static_assert(WEIGHTED == 0 || WEIGHTED == 1, "w_hat is given or not");
  constexpr int V = kLtV;
  constexpr int BV = kLtSlotSliced ? V : 1;  // distinct slot ranges (loads of b_hat, w_hat) per term
  const uint32_t l = blockIdx.y;
  const BconvTo<W> C = to[l];
  const LtLimb<W> E = lc[l];
  const A ar = ks_arith<A>(C);
  const uint32_t lgs = logn - 8, sh = 32 - logn, mask2 = (2u << logn) - 1;
  const size_t step = (size_t)limbs << logn, cstep = step * terms, rstep = cstep * COMPS;
  const bool with_c0 = c0 != nullptr && l < L;  // (block-uniform)
  bool live[V];
  uint32_t j[BV];
  const IO *ap[V], *zp[V], *bp[BV], *wp[BV];
  IO *cp[V];
#pragma unroll
  for (int v = 0; v < V; v++) {
    size_t p;
    uint32_t jv;
    if constexpr (kLtSlotSliced) {
      const size_t s = (size_t)blockIdx.x * V + v;
      live[v] = s < units;
      const size_t sl = live[v] ? s : 0;
      p = sl >> lgs;
      jv = ((uint32_t)(sl & (((size_t)1 << lgs) - 1)) << 8) + threadIdx.x;
    } else {
      const uint32_t g = kLtRangeFastest ? blockIdx.x >> lgs : blockIdx.x % groups;
      const uint32_t s = kLtRangeFastest ? blockIdx.x & ((1u << lgs) - 1) : blockIdx.x / groups;
      const size_t e = (size_t)g * V + v;
      live[v] = e < units;
      p = live[v] ? e : 0;
      jv = (s << 8) + threadIdx.x;
    }
    if (v < BV) {
      j[v] = jv;
      bp[v] = bh + ((size_t)l << logn) + jv;
      wp[v] = WEIGHTED ? wh + ((size_t)l << logn) + jv : nullptr;
    }
    ap[v] = ah + ((p * terms * limbs + l) << logn);
    zp[v] = with_c0 ? c0 + ((p * L + l) << logn) : nullptr;
    cp[v] = c + ((p * COMPS * limbs + l) << logn) + jv;
  }
  W in[COMPS][V], out[COMPS][V];
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
#pragma unroll
    for (int v = 0; v < V; v++) in[i][v] = out[i][v] = 0;
  });
  for (uint32_t r = 0; r < rots; r++) {
    const uint32_t kr = ks.k[r];
    uint32_t src[BV];
#pragma unroll
    for (int u = 0; u < BV; u++) src[u] = galois_slot(j[u], kr, sh, mask2);
    if constexpr (WEIGHTED) {
      each_comp<COMPS>([&](auto ci) {
        constexpr int i = decltype(ci)::value;
#pragma unroll
        for (int v = 0; v < V; v++) in[i][v] = 0;
      });
    }
    const size_t ro = (size_t)r * rstep;
    for (uint32_t t = 0; t < terms; t++) {
      const size_t o = (size_t)t * step;
      W x[V], bv[COMPS][BV];
#pragma unroll
      for (int v = 0; v < V; v++) x[v] = to_word<W>(ap[v][o + src[v % BV]]);
      each_comp<COMPS>([&](auto ci) {
        constexpr int i = decltype(ci)::value;
#pragma unroll
        for (int u = 0; u < BV; u++) bv[i][u] = to_word<W>(bp[u][ro + i * cstep + o]);
      });
      each_comp<COMPS>([&](auto ci) {
        constexpr int i = decltype(ci)::value;
#pragma unroll
        for (int v = 0; v < V; v++)
          in[i][v] = mac_add(ar, in[i][v], ar.mont(x[v], bv[i][v % BV]));
      });
    }
    if (with_c0) {
#pragma unroll
      for (int v = 0; v < V; v++)
        in[0][v] = mac_add(ar, in[0][v], ar.mont(to_word<W>(zp[v][src[v % BV]]), E.pq));
    }
    if constexpr (WEIGHTED) {
      W w[BV];
#pragma unroll
      for (int u = 0; u < BV; u++) w[u] = to_word<W>(wp[u][(size_t)r * step]);
      each_comp<COMPS>([&](auto ci) {
        constexpr int i = decltype(ci)::value;
#pragma unroll
        for (int v = 0; v < V; v++)
          out[i][v] = mac_add(ar, out[i][v], ar.mont(in[i][v], w[v % BV]));
      });
    }
  }
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
#pragma unroll
    for (int v = 0; v < V; v++) {
      if (!live[v]) continue;
      if constexpr (WEIGHTED)  // out R^2 mod m
        cp[v][i * step] = (IO)BconvArith<W>::mulc(out[i][v], E.r2, E.r2s, C.c);
      else                     // in R mod m
        cp[v][i * step] = (IO)BconvArith<W>::mulc(in[i][v], C.v, C.vs, C.c);
    }
  });
}

}  // namespace nttmul
