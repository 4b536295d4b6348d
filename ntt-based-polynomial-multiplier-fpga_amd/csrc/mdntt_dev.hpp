// mdntt_dev.hpp — the kernels of include/nttmul_mdntt.h (lib/libnttmul_mdntt.so only): ModDown on
// NTT-domain limbs, x_hat [batch][L + K][n] -> out [batch][L][n], every limb a transform.  Device
// code; its launchers are in mdntt.hip.  It reuses fwd_all / inv_all and the stream loads and
// stores of kernels_dev.hpp, limb_params (rns_dev.hpp), mp_limb_params / mp_row_word
// (rnsmp_dev.hpp) and BconvArith<W> (bconv_dev.hpp: mulc, mac, fold, reduce and the fold cadences)
// unchanged and adds no function to them.
//
//   y_j       = INTT_{p_j}(x_hat[p][L + j]) (Ph_j^-1 mod p_j)              canonical, in the scratch
//   r_l[k]    = (sum_j y_j[k] (Ph_j R mod q_l)) R^-1 mod q_l               canonical
//   out[p][l] = (x_hat[p][l] - canon(NTT_{q_l}(r_l)) + q_l) (P^-1 mod q_l) mod q_l
//
// n <= 4096, two launches: k_mdntt_inv (grid (blocks, K)) and k_mdntt_fwd.  Above, the 2^L1 x 4096
// split of rnsmp_dev.hpp, four launches: k_mdntt_inv_rows (grid (rows, K)), the library's own
// k_rnsmp_cols_inv on a view of the P limbs' tables, k_mdntt_cols_fwd and k_mdntt_rows.
//
// The factor Ph_j^-1 costs nothing: the inverse's table entry (mdntt.cpp) carries
// n^-1 Ph_j^-1 and iw[1] n^-1 Ph_j^-1 where the standalone inverse carries n^-1 and iw[1] n^-1,
// and the last inverse stage (gs_scaled) multiplies by them either way.
//
// Grid order of the two kernels that read y (k_mdntt_fwd, k_mdntt_cols_fwd) and of k_mdntt_rows:
// one-dimensional with the target limb fastest, l = blockIdx.x % L.  Every y word is read by L
// workgroups, one per target limb; with the limb fastest those are adjacent in dispatch order, so
// the re-reads meet in L2 instead of lying a whole sub-batch apart.  l is still a blockIdx
// expression, wave-uniform: the limb's KParams, its BconvTo entry and the weights stay scalar
// loads.  The batch never goes to gridDim.y (limited to 65535).
//
// Range contract, per arithmetic class (y = a word of the scratch, w = a weight, r = the reduced
// sum, t = fwd_all's output, x = a word of x_hat, C = q_l):
//   Arith32P  y <= p_j - 1, w <= C - 1, both < 2^31: bconv_dev.hpp's 64-bit accumulator, a fold
//             after every 2 products, for any K <= 63; r = reduce(folded) in [0, C).  fwd_all reads
//             canonical words (what k_rns_xform<.., 0> feeds it) and leaves t in [0, 2C);
//             canon(t) in [0, C); x - canon(t) + C in (0, 2C) < 2^32, which mulc takes (any 32-bit
//             word) and returns canonical.
//   Arith64   y <= p_j - 1, w <= C - 1, both < 2^62: the four 31-bit limb sums, a fold after every
//             4 products, for any K <= 63; r in [0, C).  fwd_all (Harvey CT) reads [0, 4C), so
//             canonical r is inside, and leaves t in [0, 4C); canon(t) in [0, C);
//             x - canon(t) + C in (0, 2C) < 2^63, which mulc (Shoup, then one conditional
//             subtraction) takes and returns canonical.
// The multi-pass pair splits the same chain at the column pass: k_mdntt_cols_fwd forms canonical
// r and runs k_rnsmp_cols_fwd's butterflies on it (lazy words to the scratch, [0, 2C) / [0, 4C)),
// k_mdntt_rows reads them as k_rnsmp_xform<.., 0> does and ends in the same epilogue.
#pragma once
#include "bconv_dev.hpp"
#include "rns_dev.hpp"
#include "rnsmp_dev.hpp"

namespace nttmul {

// coefficients converted together: 16 accumulators of 64 bits on 32-bit words, 4 of BconvArith's
// six-word accumulators on 64-bit words
template <class W>
constexpr int md_group() { return sizeof(W) == 4 ? 16 : 4; }

// r[k] = (sum over j < K of y_j[off(k)] w_j) R^-1 mod c for KG coefficients.  yp: this thread's
// word 0 of y_0, `step` words between limbs; wl: the weight of (limb 0 of P, this target limb),
// lpad words between source limbs.  j is a loop counter and wl, C are wave-uniform: scalar loads.
template <class W, int KG, class Off>
__device__ __forceinline__ void md_sum(W (&r)[KG], const W *__restrict__ yp, size_t step,
                                       uint32_t K, const W *__restrict__ wl, uint32_t lpad,
                                       const BconvTo<W> &C, Off off) {
  using Ar = BconvArith<W>;
  constexpr int CAD = Ar::kCadence;
  typename Ar::Acc acc[KG];
#pragma unroll
  for (int k = 0; k < KG; k++) acc[k] = Ar::zero();
  const auto term = [&](uint32_t j) {
    const W w = wl[(size_t)j * lpad];
    const W *yj = yp + (size_t)j * step;
#pragma unroll
    for (int k = 0; k < KG; k++) Ar::mac(acc[k], yj[off(k)], w);
  };
  const auto fold = [&] {
#pragma unroll
    for (int k = 0; k < KG; k++) Ar::fold(acc[k], C.cr);
  };
  // CAD products, a fold; the last group may be shorter and is folded as well, so reduce always
  // reads a folded accumulator (k_bconv's loop)
  uint32_t j = 0;
  for (; j + CAD <= K; j += CAD) {
#pragma unroll
    for (int c = 0; c < CAD; c++) term(j + c);
    fold();
  }
  if (j < K) {
    for (; j < K; j++) term(j);
    fold();
  }
#pragma unroll
  for (int k = 0; k < KG; k++) r[k] = Ar::reduce(acc[k], C);
}

// k_rns_xform<A, IO, LOGS, 1>'s body with separate input and output strides: limb L + j of
// x_hat ([batch][L + K][n], j = blockIdx.y) -> y [batch][K][n], compact, canonical, scaled by
// n^-1 Ph_j^-1.  tab: K entries with the folded scale; tw: the twiddles of limb L (P's first).
// 32-bit words take two polynomials per thread group, as k_rns_xform.
template <class A, class IO, int LOGS>
__global__ __launch_bounds__(256) void k_mdntt_inv(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const IO *__restrict__ xh, typename A::word *__restrict__ y, size_t batch, uint32_t L,
    uint32_t K) {
  using W = typename A::word;
  using Gr = Groups<LOGS>;
  constexpr int N = Gr::N, TP = N / 16, PB = 256 / TP, G = Gr::G, NP = Gr::NP;
  constexpr int UPG = xform_upg<A, 0, 1>();
  __shared__ W lds[PB][UPG][NP];
  const uint32_t jl = blockIdx.y;
  const KParams<A> P = limb_params<A, N>(tab, tw, jl);
  const int pb = threadIdx.x / TP, j = threadIdx.x % TP;
  const size_t p = ((size_t)blockIdx.x * PB + pb) * UPG;
  const bool live = p < batch, live2 = UPG == 2 && p + 1 < batch;
  const auto in0 = [&](size_t v) { return (v * (L + K) + L + jl) * N; };
  const size_t base_in = in0(live ? p : 0) + Gr::base(G - 1, j);
  const size_t base_in2 = in0(live2 ? p + 1 : live ? p : 0) + Gr::base(G - 1, j);
  W x[16], x2[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    x[k] = to_word<W>(xh[base_in + Gr::off(G - 1, k)]);
    if (UPG == 2) x2[k] = to_word<W>(xh[base_in2 + Gr::off(G - 1, k)]);
  }
  inv_all<A, LOGS, G - 1, true, 0, 0, UPG>(P, x, x2, lds[pb][0], P.iw, j, 0, 0);
  if (live) {
    W *yo = y + (p * K + jl) * N + Gr::base(0, j);
#pragma unroll
    for (int k = 0; k < 16; k++)
      yo[Gr::off(0, k)] = A::kInvCanonical ? x[k] : P.ar.canon_inv(x[k]);
  }
  if (live2) {
    W *yo = y + ((p + 1) * K + jl) * N + Gr::base(0, j);
#pragma unroll
    for (int k = 0; k < 16; k++)
      yo[Gr::off(0, k)] = A::kInvCanonical ? x2[k] : P.ar.canon_inv(x2[k]);
  }
}

// The target limb l of a forward kernel's workgroup and its index bx among the limb's
// workgroups, from the one-dimensional grid of L * (workgroups per limb).  The limb is the fastest
// index.  NTTMUL_MDNTT_LIMB_SLOW (make ab-mdntt, measured by tools/bench_mdntt.py --lib) builds the
// other order, the limb slowest as a second grid dimension would have it, for the A/B of
// DESIGN.md section 4; both are blockIdx expressions and wave-uniform.
__device__ __forceinline__ void md_limb(uint32_t L, uint32_t &l, size_t &bx) {
#ifdef NTTMUL_MDNTT_LIMB_SLOW
  const uint32_t per = gridDim.x / L;
  l = blockIdx.x / per;
  bx = blockIdx.x % per;
#else
  l = blockIdx.x % L;
  bx = blockIdx.x / L;
#endif
}

// The epilogue of both forward kernels: out = (x - canon(t) + c) (P^-1 mod c) mod c.  Its loads of
// x_hat and stores of out are plain, as k_rns_xform's and k_rnsmp_xform's stores: in layout G - 1 a
// thread holds 16 consecutive words, so one 128-bit access of a wave touches a quarter (32-bit
// words) or an eighth (64-bit) of each of 64 cache lines, and the lines fill over the next
// accesses.  Plain accesses meet in L2; non-temporal ones (the first form built) go out as partial
// lines, and the forward kernels took three times their twins' time (profiles/mdntt/INDEX.md).
template <class A>
__device__ __forceinline__ typename A::word md_epilogue(const A &ar, typename A::word t,
                                                        typename A::word x,
                                                        const BconvTo<typename A::word> &C) {
  using W = typename A::word;
  return BconvArith<W>::mulc(x - ar.canon(t) + C.c, C.v, C.vs, C.c);  // x - t + c in (0, 2c)
}

// One thread group per output polynomial (p, l), Groups<LOGS> layout 0, PB = 256 / (n / 16)
// polynomials of one target limb per workgroup; grid one-dimensional, the limb fastest (md_limb).  The
// conversion sum of the thread's 16 coefficients, fwd_all under q_l, then the epilogue on the 16
// words of x_hat[p][l] at the addresses k_rns_xform<.., 0> stores to (layout G - 1).  tab: make_params per limb of Q (the
// first L entries of the extended basis' table); tw: the twiddles of limb 0.  to / wt:
// bconv.hpp's tables for from = P, to = Q, padded to bconv_pad(L).  Thread groups past the batch
// end read polynomial 0 and never store.
template <class A, class IO, int LOGS>
__global__ __launch_bounds__(256) void k_mdntt_fwd(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const BconvTo<typename A::word> *__restrict__ to, const typename A::word *__restrict__ wt,
    const typename A::word *__restrict__ y, const IO *__restrict__ xh, IO *__restrict__ out,
    size_t batch, uint32_t L, uint32_t K) {
  using W = typename A::word;
  using Gr = Groups<LOGS>;
  constexpr int N = Gr::N, TP = N / 16, PB = 256 / TP, G = Gr::G, NP = Gr::NP;
  constexpr int KG = md_group<W>();
  __shared__ W lds[PB][NP];
  uint32_t l;
  size_t bx;
  md_limb(L, l, bx);
  const KParams<A> P = limb_params<A, N>(tab, tw, l);
  const BconvTo<W> C = to[l];
  const int pb = threadIdx.x / TP, j = threadIdx.x % TP;
  const size_t p = bx * PB + pb;
  const bool live = p < batch;
  const size_t pl = live ? p : 0;
  const IO *xp = xh + (pl * (L + K) + l) * N + Gr::base(G - 1, j);
  // (k_mac's placement of its second operand: requested before the sums on 32-bit words, so that
  // the latency passes under them; after the transform on 64-bit words, where 16 more live words
  // cost a wave per SIMD)
  constexpr bool kEarlyX = sizeof(W) == 4;
  W xv[16];
  if constexpr (kEarlyX) {
#pragma unroll
    for (int k = 0; k < 16; k++) xv[k] = to_word<W>(xp[Gr::off(G - 1, k)]);
  }
  const W *yp = y + pl * K * N + Gr::base(0, j);
  W x[16], unused[16];
#pragma unroll
  for (int g0 = 0; g0 < 16; g0 += KG) {
    W r[KG];
    md_sum<W, KG>(r, yp, N, K, wt + l, bconv_pad(L), C, [&](int k) { return Gr::off(0, g0 + k); });
#pragma unroll
    for (int k = 0; k < KG; k++) x[g0 + k] = r[k];
  }
  TwPair<W> zw[16];
  fwd_all<A, LOGS, 0, 1>(P.ar, x, unused, lds[pb], P.fw, j, 0, 0, zw);
  if constexpr (!kEarlyX) {
#pragma unroll
    for (int k = 0; k < 16; k++) xv[k] = to_word<W>(xp[Gr::off(G - 1, k)]);
  }
  if (live) {
    IO *op = out + (p * L + l) * N + Gr::base(G - 1, j);
#pragma unroll
    for (int k = 0; k < 16; k++)
      op[Gr::off(G - 1, k)] = (IO)md_epilogue<A>(P.ar, x[k], xv[k], C);
  }
}

// k_rnsmp_xform<A, IO, L1, 1>'s body with the strided input: row `row` of limb L + j of x_hat
// (j = blockIdx.y) -> the same row of yl [cnt][K][n], lazy words, for k_rnsmp_cols_inv.  Grid
// (cnt << L1, K).  tab: K entries with the folded scale (read by the column pass); tw: the
// twiddles of limb L.
template <class A, class IO, int L1>
__global__ __launch_bounds__(256) void k_mdntt_inv_rows(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const IO *__restrict__ xh, typename A::word *__restrict__ yl, size_t units, uint32_t L,
    uint32_t K) {
  using W = typename A::word;
  using Gr = Groups<kMpLogs>;
  constexpr int N = Gr::N, TP = N / 16, G = Gr::G, NP = Gr::NP;
  static_assert(TP == 256 && sizeof(IO) == sizeof(W), "one row of 4096 per workgroup");
  __shared__ W lds[NP];
  const uint32_t jl = blockIdx.y;
  const KParams<A> P = mp_limb_params<A>(tab, tw, jl, kMpLogs + L1);
  const int j = threadIdx.x;
  const size_t u = blockIdx.x;
  if (u >= units) return;  // (grid = units exactly; block-uniform)
  const int row = (int)(u & ((1u << L1) - 1));
  const size_t base_in = mp_row_word<L1>(u >> L1, row, L + K, L + jl) + Gr::base(G - 1, j);
  const size_t base_out = mp_row_word<L1>(u >> L1, row, K, jl) + Gr::base(0, j);
  W x[16], unused[16];
#pragma unroll
  for (int k = 0; k < 16; k++)
    x[k] = to_word<W>(xh[base_in + Gr::off(G - 1, k)]);
  inv_all<A, kMpLogs, G - 1, false, 0, 0, 1>(P, x, unused, lds, P.iw, j, row, L1);
#pragma unroll
  for (int k = 0; k < 16; k++) yl[base_out + Gr::off(0, k)] = x[k];
}

// k_rnsmp_cols_fwd<A, IO, L1, 1>'s body with the conversion sum at its head: thread = one column
// of one (polynomial, target limb); its 2^L1 elements are sums over the K limbs of y
// ([cnt][K][n], canonical), then the L1 column stages under q_l, lazy words to t [cnt][L][n].
// Grid one-dimensional: (units 4096 / 256) workgroups per limb, the limb fastest (md_limb).  tab,
// tw, to, wt as k_mdntt_fwd's.
template <class A, class IO, int L1>
__global__ __launch_bounds__(256) void k_mdntt_cols_fwd(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const BconvTo<typename A::word> *__restrict__ to, const typename A::word *__restrict__ wt,
    const typename A::word *__restrict__ y, typename A::word *__restrict__ t, size_t units,
    uint32_t L, uint32_t K) {
  using W = typename A::word;
  constexpr int M = 1 << L1, logn = kMpLogs + L1;
  constexpr int KG = M < md_group<W>() ? M : md_group<W>();
  uint32_t l;
  size_t bx;
  md_limb(L, l, bx);
  const KParams<A> P = mp_limb_params<A>(tab, tw, l, (uint32_t)logn);
  const BconvTo<W> C = to[l];
  const size_t gid = bx * blockDim.x + threadIdx.x;
  if (gid >= (units << kMpLogs)) return;
  const size_t u = gid >> kMpLogs, col = gid & (((size_t)1 << kMpLogs) - 1);
  const W *yp = y + ((u * K) << logn) + col;
  W x[M];
#pragma clang loop unroll(full)
  for (int g0 = 0; g0 < M; g0 += KG) {
    W r[KG];
    md_sum<W, KG>(r, yp, (size_t)1 << logn, K, wt + l, bconv_pad(L), C,
                  [&](int k) { return (size_t)(g0 + k) << kMpLogs; });
#pragma clang loop unroll(full)
    for (int k = 0; k < KG; k++) x[g0 + k] = r[k];
  }
#pragma clang loop unroll(full)
  for (int st = 0; st < L1; st++) {
    const int dist = M >> (st + 1);
#pragma clang loop unroll(full)
    for (int m = 0; m < M; m++) {
      if (m & dist) continue;
      const TwPair<W> w = P.fw[(1 << st) + (m >> (L1 - st))];
      P.ar.ct(x[m], x[m + dist], w.w, w.ws);
    }
  }
  W *tp = t + ((u * L + l) << logn) + col;
#pragma clang loop unroll(full)
  for (int m = 0; m < M; m++) st_stream<false>(tp + ((size_t)m << kMpLogs), x[m]);
}

// k_rnsmp_xform<A, IO, L1, 0>'s body with the epilogue: row `row` of (p, l) from t
// ([cnt][L][n], after k_mdntt_cols_fwd), fwd_all at (row, L1), then the epilogue on the row of
// x_hat[p][l] at the output's addresses.  Grid one-dimensional: units = cnt << L1 rows per limb,
// the limb fastest (md_limb).
template <class A, class IO, int L1>
__global__ __launch_bounds__(256) void k_mdntt_rows(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const BconvTo<typename A::word> *__restrict__ to, const typename A::word *__restrict__ t,
    const IO *__restrict__ xh, IO *__restrict__ out, size_t units, uint32_t L, uint32_t K) {
  using W = typename A::word;
  using Gr = Groups<kMpLogs>;
  constexpr int N = Gr::N, TP = N / 16, G = Gr::G, NP = Gr::NP;
  static_assert(TP == 256 && sizeof(IO) == sizeof(W), "one row of 4096 per workgroup");
  __shared__ W lds[NP];
  uint32_t l;
  size_t u;
  md_limb(L, l, u);
  const KParams<A> P = mp_limb_params<A>(tab, tw, l, kMpLogs + L1);
  const BconvTo<W> C = to[l];
  const int j = threadIdx.x;
  if (u >= units) return;  // (grid = units L exactly; block-uniform)
  const int row = (int)(u & ((1u << L1) - 1));
  const size_t p = u >> L1;
  const size_t word_q = mp_row_word<L1>(p, row, L, l);
  const IO *xp = xh + mp_row_word<L1>(p, row, L + K, l) + Gr::base(G - 1, j);
  constexpr bool kEarlyX = sizeof(W) == 4;  // (k_mdntt_fwd)
  W x[16], xv[16], unused[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    x[k] = ld_stream<false>(t + word_q + Gr::base(0, j) + Gr::off(0, k));
    if (kEarlyX) xv[k] = to_word<W>(xp[Gr::off(G - 1, k)]);
  }
  TwPair<W> zw[16];
  fwd_all<A, kMpLogs, 0, 1>(P.ar, x, unused, lds, P.fw, j, row, L1, zw);
  if constexpr (!kEarlyX) {
#pragma unroll
    for (int k = 0; k < 16; k++) xv[k] = to_word<W>(xp[Gr::off(G - 1, k)]);
  }
  IO *op = out + word_q + Gr::base(G - 1, j);
#pragma unroll
  for (int k = 0; k < 16; k++)
    op[Gr::off(G - 1, k)] = (IO)md_epilogue<A>(P.ar, x[k], xv[k], C);
}

}  // namespace nttmul
