// hoist_dev.hpp — the hoisted rotations of include/nttmul_hoist.h (lib/libnttmul_hoist.so only):
//   c[p][r][i][l] = INTT_l( sum_t a_hat[p][t][l][src_{k_r}(j)] o b_hat[r][i][t][l][j] ),
//                                                                        r < rots, i < COMPS,
// the mac against NTT-domain operands with a already in the NTT domain and the automorphism
// sigma_{k_r} applied while it is loaded.  Device code; its launchers are in hoist.hip.
// k_rns_hoist is k_rns_macn's body (macn_dev.hpp) without fwd_all and k_rnsmp_hoist is
// k_rnsmp_macn's row pass without the forward column pass and without fwd_all; the column pass
// after it is k_rnsmp_cols_inv itself.  It reuses inv_all, mac_add, each_comp, galois_slot
// (galois_dev.hpp) and the load / store helpers unchanged and adds no function to them.
//
// Per term: the 16 words of a_hat[p][t] a lane would hold after fwd_all (the inverse's input
// layout, slot Gr::base(G - 1, j) + Gr::off(G - 1, k)), each from slot src_k of that slot; then per
// component the 16 words of b_hat[r][i][t] at the slots themselves, one mont and one mac_add.
// After the term loop, per component: one inv_all and one store.  The 16 source slots are computed
// once per workgroup, before the term loop: they depend on the lane and the rotation alone.
//
// Locality and the form of the gather.  At group G - 1 a lane holds 16 consecutive slots
// (Gr::base(G - 1, j) = 16 j), and src_k maps an aligned block of 2^m slots onto an aligned block
// of 2^m slots (galois_dev.hpp).  A lane's 16 sources therefore fill one aligned 16-word block and
// a wave's one aligned 1024-word segment: the cache lines a contiguous load would touch, permuted.
// Above n = 4096 the slot is taken over all logn bits, so the source of a row of 4096 is one other
// row, permuted.  The first form built loaded the 16 words one by one at their source slots: 16
// single-word loads per lane and term, each instruction of a wave touching 64 different lines,
// and the kernel was bound by them (no faster per rotation than k_rns_macn
// with its forward transforms, on 32-bit words).  hoist_load instead loads the lane's source block
// whole, 16 consecutive words as b_hat's are loaded, and permutes it inside the lane: the words
// go to the lane's own 17-word slot of the LDS row inv_all uses afterwards (NP >= 17 lanes' worth)
// and come back in the order of the 16 four-bit positions src_k leaves inside the block, packed
// in one 64-bit register.  No other lane reads the slot, so no barrier is needed around it; one
// barrier after the term loop keeps the first exchange of inv_all, which writes the whole row,
// behind the last slot read of every wave.  k = 1 is the identity and skips the LDS pass (the
// branch is uniform: k_r is a kernel argument).
//
// Workgroup order.  The rotation varies fastest across workgroups (blockIdx.x = unit rots + r, the
// unit being a workgroup's polynomials or a polynomial's row), the limb slowest (blockIdx.y).
// a_hat[p][.][l] is read by every rotation and streams through once per limb; with the rotation
// fastest its rots readers run at about the same time, so one of them reads it from memory and
// the others from cache.  b_hat[.][.][.][l], rots COMPS terms n words, is read by every p and stays
// cached while the limb's workgroups run.  (With p fastest, a_hat, the large operand, would be
// swept rots times.)  Both operands are read by other workgroups, so their loads stay temporal;
// c is written once and streams.
//
// Range contract, per arithmetic class and per accumulator: k_mac's (mac_dev.hpp).  A canonical
// a_hat word is inside the range mont accepts from fwd_all:
//   Arith32P  x canonical (inside [0, 2q)), b canonical, m = mont(x, b) in [0, q); acc[i] stays
//             canonical (acc + m < 2q < 2^32, one conditional subtraction per term and component).
//   Arith64   x canonical (inside [0, 4q)), b canonical, m in [0, 2q); acc[i] stays in [0, 2q)
//             (acc + m < 4q < 2^64, one conditional subtraction of 2q per term and component),
//             which the Harvey GS inverse reads.
// Neither operand is checked to be a transform: any canonical vectors are accepted.
//
// Addressing.  src_k(j) < n for every j and k by construction (a bit reversal of a value below
// n), so every gathered word lies inside the limb polynomial its base addresses.  Polynomial
// offsets are 64-bit, slots 32-bit.
#pragma once
#include "galois_dev.hpp"
#include "macn_dev.hpp"

namespace nttmul {

// The source block and the positions inside it, for the lane whose slots are j0 + off(k):
// src_k(j0 + off(k)) = *blk + ((perm >> 4 k) & 15)
template <class Gr>
__device__ __forceinline__ uint64_t hoist_sources(uint32_t j0, uint32_t kr, uint32_t sh,
                                                  uint32_t mask2, uint32_t *blk) {
  uint64_t perm = 0;
  uint32_t first = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const uint32_t s = galois_slot(j0 + (uint32_t)Gr::off(Gr::G - 1, k), kr, sh, mask2);
    if (k == 0) first = s;
    perm |= (uint64_t)(s & 15u) << (4 * k);
  }
  *blk = first & ~15u;
  return perm;
}

// x[k] = block[(perm >> 4 k) & 15] for the 16 consecutive words at `block`; slot: the lane's own 17
// words of LDS.  identity (wave-uniform): the block is the lane's own slots, in off's order
template <class Gr, class W, class IO>
__device__ __forceinline__ void hoist_load(W (&x)[16], const IO *__restrict__ block, W *slot,
                                           uint64_t perm, bool identity) {
  if (identity) {
#pragma unroll
    for (int k = 0; k < 16; k++) x[k] = to_word<W>(block[Gr::off(Gr::G - 1, k)]);
    return;
  }
  W v[16];
#pragma unroll
  for (int k = 0; k < 16; k++) v[k] = to_word<W>(block[k]);
#pragma unroll
  for (int k = 0; k < 16; k++) slot[k] = v[k];
#pragma unroll
  for (int k = 0; k < 16; k++) x[k] = slot[(uint32_t)(perm >> (4 * k)) & 15u];
}

// n <= 4096.  Grid (ceil(batch / PB) rots, limbs): workgroup blockIdx.x takes rotation
// blockIdx.x mod rots of the PB polynomials from (blockIdx.x / rots) PB.  Polynomial (p, t) of
// a_hat starts at word ((p terms + t) L + l) n, (r, i, t) of b_hat at
// (((r COMPS + i) terms + t) L + l) n and (p, r, i) of c at (((p rots + r) COMPS + i) L + l) n, all
// in 64 bits.  ks.k[r]: wave-uniform, from the kernel argument.  tab: make_params (scale F).
template <class A, class IO, int LOGS, int COMPS>
__global__ __launch_bounds__(256) void k_rns_hoist(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const IO *__restrict__ ah, const IO *__restrict__ bh, IO *__restrict__ c, GaloisKs ks,
    uint32_t rots, size_t batch, uint32_t terms, uint32_t limbs) {
  using W = typename A::word;
  using Gr = Groups<LOGS>;
  constexpr int N = Gr::N, TP = N / 16, PB = 256 / TP, G = Gr::G, NP = Gr::NP;
  static_assert(COMPS >= 1 && COMPS <= 2, "NTTMUL_MACN_MAX_COMPS");
  __shared__ W lds[PB][NP];
  const uint32_t l = blockIdx.y, r = blockIdx.x % rots, kr = ks.k[r];
  const KParams<A> P = limb_params<A, N>(tab, tw, l);
  const int pb = threadIdx.x / TP, j = threadIdx.x % TP;
  const size_t p = (size_t)(blockIdx.x / rots) * PB + pb;
  const bool live = p < batch;
  const size_t pl = live ? p : 0, step = (size_t)limbs * N, cstep = step * terms;
  static_assert(NP >= 17 * TP, "a 17-word slot per lane in the polynomial's LDS row");
  uint32_t blk;
  const uint64_t perm =
      hoist_sources<Gr>((uint32_t)Gr::base(G - 1, j), kr, 32 - LOGS, 2u * N - 1, &blk);
  const IO *ap = ah + (pl * terms * limbs + l) * N + blk;
  const IO *bp = bh + ((size_t)r * COMPS * terms * limbs + l) * N + Gr::base(G - 1, j);
  W *slot = lds[pb] + 17 * j;
  W acc[COMPS][16], y[16];
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
#pragma unroll
    for (int k = 0; k < 16; k++) acc[i][k] = 0;
  });
  for (uint32_t t = 0; t < terms; t++, ap += step, bp += step) {
    W x[16];
    hoist_load<Gr>(x, ap, slot, perm, kr == 1);
    each_comp<COMPS>([&](auto ci) {
      constexpr int i = decltype(ci)::value;
      W bv[16];
#pragma unroll
      for (int k = 0; k < 16; k++) bv[k] = to_word<W>(bp[i * cstep + Gr::off(G - 1, k)]);
#pragma unroll
      for (int k = 0; k < 16; k++) acc[i][k] = mac_add(P.ar, acc[i][k], P.ar.mont(x[k], bv[k]));
    });
  }
  __syncthreads();  // (every wave's last slot read, before the exchanges write the row)
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
    inv_all<A, LOGS, G - 1, true, 0>(P, acc[i], y, lds[pb], P.iw, j, 0, 0);
    if (live) {
      IO *cp = c + (((p * rots + r) * COMPS + i) * limbs + l) * N + Gr::base(0, j);
#pragma unroll
      for (int k = 0; k < 16; k++) {
        W v = acc[i][k];
        if (!A::kInvCanonical) v = P.ar.canon_inv(v);
        st_stream<true>(cp + Gr::off(0, k), (IO)v);
      }
    }
  });
}

// 4096 < n <= 65536: the row pass in front of k_rnsmp_cols_inv over units COMPS polynomials.
// Grid (units << L1, limbs) for one sub-batch of `units` output units; output unit u0 + v of the
// call is (p, r) = ((u0 + v) / rots, (u0 + v) mod rots).  Row `row` of limb l: per term the 4096
// words of a_hat[p][t] whose slots are src_k of the row's slots (over all logn bits: one other
// row, permuted), from caller memory; per component the row of b_hat[r][i][t] from caller memory,
// as k_rnsmp_mac reads it; COMPS rows to the output scratch tc ([units COMPS][limbs][n], the
// layout of the sub-batch's c, which k_rnsmp_cols_inv then writes in place of it).  tab:
// make_params (F is in k_rnsmp_cols_inv).
template <class A, class IO, int L1, int COMPS>
__global__ __launch_bounds__(256) void k_rnsmp_hoist(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const IO *__restrict__ ah, const IO *__restrict__ bh, typename A::word *__restrict__ tc,
    GaloisKs ks, uint32_t rots, size_t u0, size_t rows, uint32_t terms, uint32_t limbs) {
  using W = typename A::word;
  using Gr = Groups<kMpLogs>;
  constexpr int N = Gr::N, TP = N / 16, G = Gr::G, NP = Gr::NP, LOGN = kMpLogs + L1;
  static_assert(TP == 256 && COMPS >= 1 && COMPS <= 2, "one row of 4096 per workgroup");
  __shared__ W lds[NP];
  const uint32_t l = blockIdx.y;
  const KParams<A> P = mp_limb_params<A>(tab, tw, l, LOGN);
  const int j = threadIdx.x;
  const size_t v = blockIdx.x;
  if (v >= rows) return;  // (grid = rows exactly; block-uniform)
  const int row = (int)(v & ((1u << L1) - 1));
  const size_t ul = v >> L1, ug = u0 + ul, p = ug / rots;
  const uint32_t r = (uint32_t)(ug - p * rots), kr = ks.k[r];
  const size_t step = (size_t)limbs << LOGN, cstep = step * terms;
  static_assert(NP >= 17 * TP, "a 17-word slot per lane in the LDS row");
  uint32_t blk;
  const uint64_t perm =
      hoist_sources<Gr>(((uint32_t)row << kMpLogs) + (uint32_t)Gr::base(G - 1, j), kr, 32 - LOGN,
                        (2u << LOGN) - 1, &blk);
  const IO *ap = ah + ((p * terms * limbs + l) << LOGN) + blk;
  const IO *bp = bh + mp_row_word<L1>((size_t)r * COMPS * terms, row, limbs, l) +
                 Gr::base(G - 1, j);
  W *slot = lds + 17 * j;
  W acc[COMPS][16], y[16];
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
#pragma unroll
    for (int k = 0; k < 16; k++) acc[i][k] = 0;
  });
  for (uint32_t t = 0; t < terms; t++, ap += step, bp += step) {
    W x[16];
    hoist_load<Gr>(x, ap, slot, perm, kr == 1);
    each_comp<COMPS>([&](auto ci) {
      constexpr int i = decltype(ci)::value;
      W bv[16];
#pragma unroll
      for (int k = 0; k < 16; k++) bv[k] = to_word<W>(bp[i * cstep + Gr::off(G - 1, k)]);
#pragma unroll
      for (int k = 0; k < 16; k++) acc[i][k] = mac_add(P.ar, acc[i][k], P.ar.mont(x[k], bv[k]));
    });
  }
  __syncthreads();  // (every wave's last slot read, before the exchanges write the row)
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
    inv_all<A, kMpLogs, G - 1, false, 0>(P, acc[i], y, lds, P.iw, j, row, L1);
    W *cp = tc + mp_row_word<L1>(ul * COMPS + i, row, limbs, l) + Gr::base(0, j);
#pragma unroll
    for (int k = 0; k < 16; k++) cp[Gr::off(0, k)] = acc[i][k];
  });
}

}  // namespace nttmul
