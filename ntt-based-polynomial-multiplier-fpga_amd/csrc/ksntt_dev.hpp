// ksntt_dev.hpp — the kernels of include/nttmul_ksntt.h (lib/libnttmul_ksntt.so only): the first
// two steps of a hybrid key switch on NTT-domain limbs.  Device code; its launchers are in
// ksntt.hip.  It reuses md_sum (mdntt_dev.hpp), fwd_all and the stream loads and stores of
// kernels_dev.hpp, limb_params (rns_dev.hpp), mp_limb_params / mp_row_word (rnsmp_dev.hpp),
// BconvArith<W> (bconv_dev.hpp), mac_add (mac_dev.hpp), each_comp (macn_dev.hpp) and galois_slot
// (galois_dev.hpp) unchanged and adds no function to them.
//
// modup   x_hat [batch][L][n] -> up_hat [batch][dnum][M][n], M = L + K, every limb a transform
//   y_i             = INTT_{q_i}(x_hat[p][i]) (Dh_i^-1 mod q_i)              canonical, in the scratch
//   up_hat[p][d][m] = canon(NTT_m((sum_{i in D_d} y_i (Dh_i R mod m)) R^-1 mod m))   m not in D_d
//   up_hat[p][d][m] = x_hat[p][m]                                                   m in D_d
// The inverse is mdntt_dev.hpp's own kernel with (L, K) := (0, L) and a table whose scale carries
// n^-1 Dh_i^-1 (k_mdntt_inv, or k_mdntt_inv_rows and the library's k_rnsmp_cols_inv above
// n = 4096), launched through mdntt.hip: no second copy of it here.  The forward half is new:
// k_ksntt_fwd at n <= 4096; above, the 2^L1 x 4096 split, k_ksntt_cols_fwd and k_ksntt_rows.
//
// Grid order of the three: one-dimensional with the target (d, m) fastest, dm = blockIdx.x mod
// (dnum M), d = dm / M, m = dm mod M (ks_target below; md_limb's order).  Every y word of digit d
// is read by the M - |D_d| workgroups of its targets; with the target fastest those are adjacent
// in dispatch order and the re-reads meet in L2.  d and m are blockIdx expressions, wave-uniform:
// the limb's KParams, its BconvTo entry and the weights stay scalar loads, and the own-limb branch
// is block-uniform and taken before any barrier.  The batch never goes to gridDim.y.
//
// Above n = 4096 the column-passed sums are as many words as the output.  They pass through
// up_hat itself: k_ksntt_cols_fwd stores the lazy words of (p, d, m) to up_hat[p][d][m], and
// k_ksntt_rows reads each row of 4096 whole into registers, transforms it and stores the
// canonical words to the same row (k_rnsmp_xform allows out == in for the same reason: a
// workgroup owns its row).  The own limbs are skipped by the column kernel and copied by the row
// kernel, once.  Every word of up_hat is final when the row kernel has run, and no other caller
// memory is written.
//
// Loads of y and x_hat and stores of up_hat are plain, not non-temporal: in layout G - 1 a lane
// holds 16 consecutive words, and non-temporal accesses of that shape go out as partial lines
// (mdntt_dev.hpp md_epilogue records the measurement).
//
// Range contract of modup, per arithmetic class: mdntt_dev.hpp's without the epilogue (y = a word
// of the scratch, w = a weight, r = the reduced sum, t = fwd_all's output, C = the target modulus):
//   Arith32P  y <= q_i - 1, w <= C - 1, both < 2^31: bconv_dev.hpp's 64-bit accumulator, a fold
//             after every 2 products, for any alpha <= 63 (the last group may hold 1 product and
//             is folded as well); r = reduce(folded) in [0, C).  fwd_all reads canonical words
//             and leaves t in [0, 2C); canon(t) in [0, C) is stored.
//   Arith64   y <= q_i - 1, w <= C - 1, both < 2^62: the four 31-bit limb sums, a fold after every
//             4 products, for any alpha <= 63 (a last group of 1 .. 3 is folded as well); r in
//             [0, C).  fwd_all (Harvey CT) reads [0, 4C) and leaves t in [0, 4C); canon(t) in
//             [0, C) is stored.
// The multi-pass pair splits the chain at the column pass: k_ksntt_cols_fwd forms canonical r and
// runs k_rnsmp_cols_fwd's butterflies on it (lazy words, [0, 2C) / [0, 4C)), k_ksntt_rows reads
// them as k_rnsmp_xform<.., 0> does and stores canon(t).
//
// mac     c_hat[p][r][i][l][j] = (sum_t a_hat[p][t][l][src_{k_r}(j)] b_hat[r][i][t][l][j]) mod m_l
//   k_ksntt_mac: element-wise, one launch at every n, no transform and no twiddle.  The gather
//   form with one slot per lane, k_galois_ntt's: a workgroup of 256 threads takes kKsMacSlices
//   slices of 256 consecutive slots, thread t slot t of each, so every load of b_hat and every
//   store of c_hat is one word per lane, contiguous over the wave; src_k maps an aligned block of
//   64 slots onto an aligned block of 64 (galois_dev.hpp), so a wave's load of a_hat touches the
//   cache lines a contiguous load would touch, permuted.  src_k is computed per lane with
//   galois_slot, once per slice, before the term loop; there is no index table, no LDS and no
//   barrier.  The first form built took hoist_dev.hpp's shape instead (16 consecutive slots per
//   lane, the source block loaded whole and permuted through a 17-word LDS slot): there a wave's
//   access touches one word of each of 64 lines for b_hat and c_hat as well, which nothing forces
//   on an element-wise kernel, and it ran at 1.6 to 4.0 times its bound where this form's figures
//   are DESIGN.md section 4's.  The scatter form would read a_hat once and hold rots comps
//   accumulators per slot: 32 per lane and slice at 16 rotations of 2 components, 128 to 256
//   registers at four slices, or a read-modify-write of c_hat per term; the gather form re-reads
//   a_hat per rotation through the caches (the rotation is the fastest grid index, as k_rns_hoist
//   has it).
//
//   The limb's constants are its BconvTo entry, a scalar load by blockIdx.y.
//   Range contract, per accumulator (mac_dev.hpp's, mac_add per term and component):
//   Arith32P  a, b canonical; m = mont(a, b) in [0, q); acc stays canonical (acc + m < 2q < 2^32).
//             acc = S R^-1; the one step per output word is mulc(acc, R mod q) (Plantard, any
//             32-bit input), canonical S.
//   Arith64   a, b canonical; m in [0, 2q); acc stays in [0, 2q) (acc + m < 4q < 2^64);
//             mulc(acc, R mod q) (Shoup takes any 64-bit word, one conditional subtraction):
//             canonical S.
//   src_k(j) < n by construction, so every gathered word lies in the limb polynomial its base
//   addresses.  Polynomial offsets are 64-bit, slots 32-bit.
#pragma once
#include "galois_dev.hpp"
#include "macn_dev.hpp"
#include "mdntt_dev.hpp"

namespace nttmul {

// The target (d, m) of a forward kernel's workgroup and its index bx among the target's
// workgroups, from the one-dimensional grid of dnum M (workgroups per target); the target is the
// fastest index.  [i0, i1): the digit's own limbs.  All blockIdx expressions.
struct KsTarget {
  uint32_t d, m, i0, i1;
  size_t bx;
  bool own;
};
__device__ __forceinline__ KsTarget ks_target(uint32_t L, uint32_t M, uint32_t dnum,
                                              uint32_t alpha) {
  KsTarget t;
  const uint32_t per = dnum * M, dm = blockIdx.x % per;
  t.bx = blockIdx.x / per;
  t.d = dm / M;
  t.m = dm - t.d * M;
  t.i0 = t.d * alpha;
  t.i1 = t.i0 + alpha < L ? t.i0 + alpha : L;
  t.own = t.m >= t.i0 && t.m < t.i1;
  return t;
}

// One thread group per output limb polynomial (p, d, m), Groups<LOGS> layout 0, PB = 256 / (n / 16)
// polynomials of one target per workgroup.  m in D_d: the copy of x_hat[p][m].  Otherwise the
// conversion sum of the thread's 16 coefficients over the digit's limbs, fwd_all under modulus m,
// canon, at the addresses k_rns_xform<.., 0> stores to (layout G - 1).  tab: make_params per limb
// of Q u P; tw: the twiddles of limb 0; to / wt: padded to bconv_pad(M).  y [batch][L][n].
// Thread groups past the batch end read polynomial 0 and never store.
template <class A, class IO, int LOGS>
__global__ __launch_bounds__(256) void k_ksntt_fwd(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const BconvTo<typename A::word> *__restrict__ to, const typename A::word *__restrict__ wt,
    const typename A::word *__restrict__ y, const IO *__restrict__ xh, IO *__restrict__ up,
    size_t batch, uint32_t L, uint32_t K, uint32_t dnum, uint32_t alpha) {
  using W = typename A::word;
  using Gr = Groups<LOGS>;
  constexpr int N = Gr::N, TP = N / 16, PB = 256 / TP, G = Gr::G, NP = Gr::NP;
  constexpr int KG = md_group<W>();
  __shared__ W lds[PB][NP];
  const uint32_t M = L + K;
  const KsTarget t = ks_target(L, M, dnum, alpha);
  const int pb = threadIdx.x / TP, j = threadIdx.x % TP;
  const size_t p = t.bx * PB + pb;
  const bool live = p < batch;
  const size_t pl = live ? p : 0;
  IO *op = up + ((p * dnum + t.d) * M + t.m) * N + Gr::base(G - 1, j);
  if (t.own) {  // (block-uniform, before any barrier)
    if (live) {
      const IO *xp = xh + (p * L + t.m) * N + Gr::base(G - 1, j);
#pragma unroll
      for (int k = 0; k < 16; k++) op[Gr::off(G - 1, k)] = xp[Gr::off(G - 1, k)];
    }
    return;
  }
  const KParams<A> P = limb_params<A, N>(tab, tw, t.m);
  const BconvTo<W> C = to[t.m];
  const uint32_t mpad = bconv_pad(M);
  const W *yp = y + (pl * L + t.i0) * N + Gr::base(0, j);
  W x[16], unused[16];
#pragma unroll
  for (int g0 = 0; g0 < 16; g0 += KG) {
    W r[KG];
    md_sum<W, KG>(r, yp, N, t.i1 - t.i0, wt + (size_t)t.i0 * mpad + t.m, mpad, C,
                  [&](int k) { return Gr::off(0, g0 + k); });
#pragma unroll
    for (int k = 0; k < KG; k++) x[g0 + k] = r[k];
  }
  TwPair<W> zw[16];
  fwd_all<A, LOGS, 0, 1>(P.ar, x, unused, lds[pb], P.fw, j, 0, 0, zw);
  if (live) {
#pragma unroll
    for (int k = 0; k < 16; k++) op[Gr::off(G - 1, k)] = (IO)P.ar.canon(x[k]);
  }
}

// k_mdntt_cols_fwd's body over the targets (d, m): thread = one column of one (polynomial, d, m)
// with m not in D_d; its 2^L1 elements are sums over the digit's limbs of y ([cnt][L][n],
// canonical), then the L1 column stages under modulus m, lazy words to up_hat[p][d][m].  A
// workgroup whose m is one of the digit's own limbs leaves at once (k_ksntt_rows copies them).
// Grid one-dimensional: (units 4096 / 256) workgroups per target, the target fastest.
template <class A, class IO, int L1>
__global__ __launch_bounds__(256) void k_ksntt_cols_fwd(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const BconvTo<typename A::word> *__restrict__ to, const typename A::word *__restrict__ wt,
    const typename A::word *__restrict__ y, IO *__restrict__ up, size_t units, uint32_t L,
    uint32_t K, uint32_t dnum, uint32_t alpha) {
  using W = typename A::word;
  static_assert(sizeof(IO) == sizeof(W), "the lazy words pass through up_hat");
  constexpr int M1 = 1 << L1, logn = kMpLogs + L1;
  constexpr int KG = M1 < md_group<W>() ? M1 : md_group<W>();
  const uint32_t M = L + K;
  const KsTarget t = ks_target(L, M, dnum, alpha);
  if (t.own) return;  // (block-uniform)
  const KParams<A> P = mp_limb_params<A>(tab, tw, t.m, (uint32_t)logn);
  const BconvTo<W> C = to[t.m];
  const uint32_t mpad = bconv_pad(M);
  const size_t gid = t.bx * blockDim.x + threadIdx.x;
  if (gid >= (units << kMpLogs)) return;
  const size_t u = gid >> kMpLogs, col = gid & (((size_t)1 << kMpLogs) - 1);
  const W *yp = y + ((u * L + t.i0) << logn) + col;
  W x[M1];
#pragma clang loop unroll(full)
  for (int g0 = 0; g0 < M1; g0 += KG) {
    W r[KG];
    md_sum<W, KG>(r, yp, (size_t)1 << logn, t.i1 - t.i0, wt + (size_t)t.i0 * mpad + t.m, mpad, C,
                  [&](int k) { return (size_t)(g0 + k) << kMpLogs; });
#pragma clang loop unroll(full)
    for (int k = 0; k < KG; k++) x[g0 + k] = r[k];
  }
#pragma clang loop unroll(full)
  for (int st = 0; st < L1; st++) {
    const int dist = M1 >> (st + 1);
#pragma clang loop unroll(full)
    for (int m = 0; m < M1; m++) {
      if (m & dist) continue;
      const TwPair<W> w = P.fw[(1 << st) + (m >> (L1 - st))];
      P.ar.ct(x[m], x[m + dist], w.w, w.ws);
    }
  }
  IO *tp = up + (((u * dnum + t.d) * M + t.m) << logn) + col;
#pragma clang loop unroll(full)
  for (int m = 0; m < M1; m++) tp[(size_t)m << kMpLogs] = (IO)x[m];
}

// k_rnsmp_xform<A, IO, L1, 0>'s body in place on up_hat: row `row` of (p, d, m), the lazy words
// k_ksntt_cols_fwd left there, fwd_all at (row, L1), canon, to the same row (a workgroup reads its
// row whole before fwd_all's first barrier and owns it).  m in D_d: the row of x_hat[p][m] is
// copied instead.  Grid one-dimensional: units = cnt << L1 rows per target, the target fastest.
// up carries no __restrict__: it is read and written.
template <class A, class IO, int L1>
__global__ __launch_bounds__(256) void k_ksntt_rows(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const IO *__restrict__ xh, IO *up, size_t units, uint32_t L, uint32_t K, uint32_t dnum,
    uint32_t alpha) {
  using W = typename A::word;
  using Gr = Groups<kMpLogs>;
  constexpr int N = Gr::N, TP = N / 16, G = Gr::G, NP = Gr::NP;
  static_assert(TP == 256 && sizeof(IO) == sizeof(W), "one row of 4096 per workgroup");
  __shared__ W lds[NP];
  const uint32_t M = L + K;
  const KsTarget t = ks_target(L, M, dnum, alpha);
  const size_t u = t.bx;
  if (u >= units) return;  // (grid = units dnum M exactly; block-uniform)
  const int j = threadIdx.x;
  const int row = (int)(u & ((1u << L1) - 1));
  const size_t p = u >> L1;
  const size_t word_o = mp_row_word<L1>(p * dnum + t.d, row, M, t.m);
  IO *op = up + word_o + Gr::base(G - 1, j);
  if (t.own) {  // (block-uniform, before any barrier)
    const IO *xp = xh + mp_row_word<L1>(p, row, L, t.m) + Gr::base(G - 1, j);
#pragma unroll
    for (int k = 0; k < 16; k++) op[Gr::off(G - 1, k)] = xp[Gr::off(G - 1, k)];
    return;
  }
  const KParams<A> P = mp_limb_params<A>(tab, tw, t.m, kMpLogs + L1);
  W x[16], unused[16];
#pragma unroll
  for (int k = 0; k < 16; k++) x[k] = to_word<W>(up[word_o + Gr::base(0, j) + Gr::off(0, k)]);
  TwPair<W> zw[16];
  fwd_all<A, kMpLogs, 0, 1>(P.ar, x, unused, lds, P.fw, j, row, L1, zw);
#pragma unroll
  for (int k = 0; k < 16; k++) op[Gr::off(G - 1, k)] = (IO)P.ar.canon(x[k]);
}

// The class's arithmetic object from a limb's BconvTo entry: what mont and mac_add read (the
// modulus and -q^-1 mod R)
template <class A>
__device__ __forceinline__ A ks_arith(const BconvTo<typename A::word> &C);
template <>
__device__ __forceinline__ Arith32P ks_arith<Arith32P>(const BconvTo<uint32_t> &C) {
  return Arith32P{C.c, C.qinv_neg, C.cr, 0};
}
template <>
__device__ __forceinline__ Arith64 ks_arith<Arith64>(const BconvTo<uint64_t> &C) {
  return Arith64{C.c, C.qinv_neg, 2 * C.c};
}

// slices of 256 slots a k_ksntt_mac workgroup takes: 4 (1 + comps) loads in flight per term
constexpr int kKsMacSlices = 4;

// Element-wise.  Grid (ceil(slices / kKsMacSlices) rots, M) with slices = batch n / 256: workgroup
// blockIdx.x takes rotation r = blockIdx.x mod rots of the kKsMacSlices slices from
// (blockIdx.x / rots) kKsMacSlices; slice s is slots [(s mod 2^lgs) 256, +256) of polynomial
// p = s >> lgs, lgs = logn - 8, limb l = blockIdx.y, thread t its slot t.  (p, t) of a_hat starts
// at word ((p terms + t) M + l) n, (r, i, t) of b_hat at (((r COMPS + i) terms + t) M + l) n,
// (p, r, i) of c_hat at (((p rots + r) COMPS + i) M + l) n, all in 64 bits.  to: BconvTo<W>[..]
// over Q u P whose (v, vs) is the pair of R mod m.  Slices past the end read slice 0 (always
// valid) instead of branching per load; their results are never stored.
template <class A, class IO, int COMPS>
__global__ __launch_bounds__(256) void k_ksntt_mac(
    const BconvTo<typename A::word> *__restrict__ to, const IO *__restrict__ ah,
    const IO *__restrict__ bh, IO *__restrict__ c, GaloisKs ks, uint32_t rots, size_t slices,
    uint32_t terms, uint32_t limbs, uint32_t logn) {
  using W = typename A::word;
  static_assert(COMPS >= 1 && COMPS <= 2, "NTTMUL_MACN_MAX_COMPS");
  constexpr int V = kKsMacSlices;
  const uint32_t l = blockIdx.y, r = blockIdx.x % rots, kr = ks.k[r];
  const BconvTo<W> C = to[l];
  const A ar = ks_arith<A>(C);
  const uint32_t lgs = logn - 8, sh = 32 - logn, mask2 = (2u << logn) - 1;
  const size_t step = (size_t)limbs << logn, cstep = step * terms;
  bool live[V];
  const IO *ap[V], *bp[V];
  IO *cp[V];
#pragma unroll
  for (int v = 0; v < V; v++) {
    const size_t s = (size_t)(blockIdx.x / rots) * V + v;
    live[v] = s < slices;
    const size_t sl = live[v] ? s : 0, p = sl >> lgs;
    const uint32_t j = ((uint32_t)(sl & (((size_t)1 << lgs) - 1)) << 8) + threadIdx.x;
    ap[v] = ah + ((p * terms * limbs + l) << logn) + galois_slot(j, kr, sh, mask2);
    bp[v] = bh + (((size_t)r * COMPS * terms * limbs + l) << logn) + j;
    cp[v] = c + ((((p * rots + r) * COMPS) * limbs + l) << logn) + j;
  }
  W acc[COMPS][V];
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
#pragma unroll
    for (int v = 0; v < V; v++) acc[i][v] = 0;
  });
  for (uint32_t t = 0; t < terms; t++) {
    const size_t o = (size_t)t * step;
    W x[V], bv[COMPS][V];
#pragma unroll
    for (int v = 0; v < V; v++) x[v] = to_word<W>(ap[v][o]);
    each_comp<COMPS>([&](auto ci) {
      constexpr int i = decltype(ci)::value;
#pragma unroll
      for (int v = 0; v < V; v++) bv[i][v] = to_word<W>(bp[v][i * cstep + o]);
    });
    each_comp<COMPS>([&](auto ci) {
      constexpr int i = decltype(ci)::value;
#pragma unroll
      for (int v = 0; v < V; v++) acc[i][v] = mac_add(ar, acc[i][v], ar.mont(x[v], bv[i][v]));
    });
  }
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
#pragma unroll
    for (int v = 0; v < V; v++)
      if (live[v])
        cp[v][i * step] = (IO)BconvArith<W>::mulc(acc[i][v], C.v, C.vs, C.c);  // acc R mod m
  });
}

}  // namespace nttmul
