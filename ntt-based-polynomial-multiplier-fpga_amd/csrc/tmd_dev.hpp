// tmd_dev.hpp — the kernels of include/nttmul_tmd.h (lib/libnttmul_tmd.so only): the
// plaintext-preserving ModDown x_hat [batch][L + K][n] -> out [batch][L][n], every limb a
// transform.  Device code; its launchers are in tmd.hip.  It reuses md_group, md_limb and
// md_epilogue (mdntt_dev.hpp), fwd_all and the stream loads and stores of kernels_dev.hpp,
// limb_params (rns_dev.hpp), mp_limb_params (rnsmp_dev.hpp) and BconvArith<W> (bconv_dev.hpp:
// mac, fold, reduce and the fold cadences) unchanged and adds no function to them.
//
//   y_j       = INTT_{p_j}(x_hat[p][L + j]) (Ph_j^-1 mod p_j)              canonical, in the scratch
//   v[k]      = (sum_j y_j[k] (g_j T mod t)) T^-1 mod t                    canonical, g_j = -p_j^-1 mod t
//   u[k]      = v[k] if v[k] <= (t - 1) / 2 else v[k] - t                  |u| <= (t - 1) / 2
//   r_l[k]    = (sum_j y_j[k] (Ph_j R mod q_l) + |u[k]| (+-P R mod q_l)) R^-1 mod q_l      canonical
//   out[p][l] = (x_hat[p][l] - canon(NTT_{q_l}(r_l)) + q_l) (P^-1 mod q_l) mod q_l
//
// (R = T = 2^32 or 2^64, the word's.)  S = sum_j y_j Ph_j is an exact integer congruent to X
// modulo P, v = -S P^-1 mod t, and d = S + u P is congruent to X modulo P and to 0 modulo t:
// (X - d) / P keeps X's residue modulo t up to the factor P^-1 (include/nttmul_tmd.h).
//
// The inverse half is mdntt_dev.hpp's own (k_mdntt_inv, or k_mdntt_inv_rows and the library's
// k_rnsmp_cols_inv above n = 4096) and so is the row pass above n = 4096 (k_mdntt_rows, which
// reads P^-1 from the table), launched through mdntt.hip.  The forward half is new: k_tmd_fwd at
// n <= 4096, k_tmd_cols_fwd above.
//
// The mod-t sum is a second BconvArith accumulator per coefficient, folded with T mod t and
// reduced with t's own BconvTo entry: the same mac, fold and reduce as the conversion sum, under
// the same stated contract, which asks of the target modulus only that it is odd and inside its
// class (bconv_dev.hpp: "small moduli only make every bound smaller"), and of y only y <= p_j - 1:
// y >= t is inside it.  reduce leaves v canonical in [0, t), so the centring is one comparison.
//
// Sign of u.  The (K + 1)-th multiplier is |u| <= (t - 1) / 2, and its weight is chosen per lane
// between two wave-uniform rows of the table, P R mod q_l (u >= 0) and -P R mod q_l (u < 0): a
// multiplier t - |u| or u + q_l would leave mac's operand range.
//
// Grid order: md_limb's, one-dimensional with the target limb fastest, with plain loads and stores
// (mdntt_dev.hpp md_epilogue records why).  The weights, g_j and t's entry stay a scalar load per j.
//
// Range contract, per arithmetic class (y = a word of the scratch, w = a weight, g = g_j T mod t,
// r = the reduced sum, s = fwd_all's output, x = a word of x_hat, C = q_l):
//   Arith32P  y <= p_j - 1, w <= C - 1, g <= t - 1, |u| <= (t - 1) / 2, p_j, C, t <= 2^31 - 1:
//             two of bconv_dev.hpp's 64-bit accumulators, a fold of each after every 2 products,
//             for any K + 1 <= 64 (a last group of 1 product is folded as well).  The mod-t one
//             ends there: v = reduce(folded) in [0, t).  The correction |u| w_K is a group of its
//             own on the folded conversion accumulator (F + P < 2^64 as F + 2 P is) and is folded;
//             r = reduce(folded) in [0, C).  fwd_all reads canonical words and leaves s in
//             [0, 2C); canon(s) in [0, C); x - canon(s) + C in (0, 2C) < 2^32, which mulc takes
//             and returns canonical.
//   Arith64   the same with p_j, C, t <= 2^62 - 1: two of the four-limb-sum accumulators, a fold
//             of each after every 4 products, for any K + 1 <= 64 (a last group of 1 .. 3 is
//             folded as well); v in [0, t); the correction is a group of its own (one product in
//             empty limb sums) and is folded; r in [0, C).  fwd_all (Harvey CT) reads [0, 4C) and
//             leaves s in [0, 4C); canon(s) in [0, C); x - canon(s) + C in (0, 2C) < 2^63 for mulc.
// t >= 3 and odd: -t^-1 mod T exists, T mod t is well defined, and (t - 1) / 2 >= 1.  Nothing
// asks more of a small t; the lower bound is the interface's, not the arithmetic's.
// The multi-pass pair splits the same chain at the column pass, as mdntt_dev.hpp's does.
#pragma once
#include "mdntt_dev.hpp"

namespace nttmul {

// coefficients converted together, two accumulators each.  32-bit words: md_group's 16 (groups of 8
// change no instantiation's waves per SIMD).  64-bit words: half of md_group's 4, so that the two
// six-word accumulators per coefficient take the registers md_sum's one takes (with 4 k_tmd_fwd
// took 216 to 222 VGPRs, two waves per SIMD; with 2, 166 to 168, three as k_mdntt_fwd).
// k_tmd_cols_fwd keeps its 2^L1 results live beside the accumulators: at L1 = 4 it takes 248
// VGPRs with 4, 190 with 2 and 165 with 1 (three waves, as k_mdntt_cols_fwd's 130), and one
// coefficient at a time is what it converts there; below, 2 keeps the waves and measured 2 to 7 %
// ahead of 1, which in turn is 1 to 8 % ahead of 2 at L1 = 4 (profiles/tmd/cols_group.json)
template <class W>
constexpr int tm_group() { return sizeof(W) == 4 ? 16 : 2; }
template <class W, int L1>
constexpr int tm_cols_group() { return sizeof(W) == 4 ? 16 : L1 == 4 ? 1 : 2; }

// md_sum with the mod-t accumulator beside the conversion sum and the correction as the
// (K + 1)-th product.  yp, step, lpad, C, off as md_sum's; wl has K + 2 rows (row K: P, row
// K + 1: -P); gt: g_j T mod t at gt[j gpad]; T: t's entry (c = t, qinv_neg, cr).  j is a loop
// counter and wl, gt, C, T are wave-uniform: scalar loads.
template <class W, int KG, class Off>
__device__ __forceinline__ void tm_sum(W (&r)[KG], const W *__restrict__ yp, size_t step,
                                       uint32_t K, const W *__restrict__ wl, uint32_t lpad,
                                       const W *__restrict__ gt, uint32_t gpad,
                                       const BconvTo<W> &C, const BconvTo<W> &T, Off off) {
  using Ar = BconvArith<W>;
  constexpr int CAD = Ar::kCadence;
  typename Ar::Acc acc[KG], tac[KG];
#pragma unroll
  for (int k = 0; k < KG; k++) {
    acc[k] = Ar::zero();
    tac[k] = Ar::zero();
  }
  const auto term = [&](uint32_t j) {
    const W w = wl[(size_t)j * lpad];
    const W g = gt[(size_t)j * gpad];
    const W *yj = yp + (size_t)j * step;
#pragma unroll
    for (int k = 0; k < KG; k++) {
      const W y = yj[off(k)];
      Ar::mac(acc[k], y, w);
      Ar::mac(tac[k], y, g);
    }
  };
  const auto fold = [&] {
#pragma unroll
    for (int k = 0; k < KG; k++) {
      Ar::fold(acc[k], C.cr);
      Ar::fold(tac[k], T.cr);
    }
  };
  // CAD products, a fold; the last group may be shorter and is folded as well (md_sum's loop);
  // then the correction, one product, and its fold: reduce always reads a folded accumulator
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
  const W wp = wl[(size_t)K * lpad], wn = wl[(size_t)(K + 1) * lpad];
  const W half = T.c >> 1;  // (t - 1) / 2
#pragma unroll
  for (int k = 0; k < KG; k++) {
    const W v = Ar::reduce(tac[k], T);
    const bool neg = v > half;
    Ar::mac(acc[k], neg ? T.c - v : v, neg ? wn : wp);
    Ar::fold(acc[k], C.cr);
    r[k] = Ar::reduce(acc[k], C);
  }
}

// k_mdntt_fwd's body with the corrected sum.  tab, tw, to, y, xh, out, batch, L, K as
// k_mdntt_fwd's; wt has K + 2 rows padded to bconv_pad(L); tt: t's entry; gt: [K] rows of
// bconv_pad(1) words.  Thread groups past the batch end read polynomial 0 and never store.
template <class A, class IO, int LOGS>
__global__ __launch_bounds__(256) void k_tmd_fwd(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const BconvTo<typename A::word> *__restrict__ to, const typename A::word *__restrict__ wt,
    const BconvTo<typename A::word> *__restrict__ tt, const typename A::word *__restrict__ gt,
    const typename A::word *__restrict__ y, const IO *__restrict__ xh, IO *__restrict__ out,
    size_t batch, uint32_t L, uint32_t K) {
  using W = typename A::word;
  using Gr = Groups<LOGS>;
  constexpr int N = Gr::N, TP = N / 16, PB = 256 / TP, G = Gr::G, NP = Gr::NP;
  constexpr int KG = tm_group<W>();
  __shared__ W lds[PB][NP];
  uint32_t l;
  size_t bx;
  md_limb(L, l, bx);
  const KParams<A> P = limb_params<A, N>(tab, tw, l);
  const BconvTo<W> C = to[l], T = tt[0];
  const int pb = threadIdx.x / TP, j = threadIdx.x % TP;
  const size_t p = bx * PB + pb;
  const bool live = p < batch;
  const size_t pl = live ? p : 0;
  const W *yp = y + pl * K * N + Gr::base(0, j);
  W x[16], unused[16];
#pragma unroll
  for (int g0 = 0; g0 < 16; g0 += KG) {
    W r[KG];
    tm_sum<W, KG>(r, yp, N, K, wt + l, bconv_pad(L), gt, bconv_pad(1), C, T,
                  [&](int k) { return Gr::off(0, g0 + k); });
#pragma unroll
    for (int k = 0; k < KG; k++) x[g0 + k] = r[k];
  }
  TwPair<W> zw[16];
  fwd_all<A, LOGS, 0, 1>(P.ar, x, unused, lds[pb], P.fw, j, 0, 0, zw);
  // (after the transform in both classes: the sums hold an accumulator per coefficient more
  // than k_mdntt_fwd's, and 16 more live words under them cost registers)
  const IO *xp = xh + (pl * (L + K) + l) * N + Gr::base(G - 1, j);
  W xv[16];
#pragma unroll
  for (int k = 0; k < 16; k++) xv[k] = to_word<W>(xp[Gr::off(G - 1, k)]);
  if (live) {
    IO *op = out + (p * L + l) * N + Gr::base(G - 1, j);
#pragma unroll
    for (int k = 0; k < 16; k++)
      op[Gr::off(G - 1, k)] = (IO)md_epilogue<A>(P.ar, x[k], xv[k], C);
  }
}

// k_mdntt_cols_fwd's body with the corrected sum: thread = one column of one (polynomial, target
// limb); lazy words to t [cnt][L][n] for k_mdntt_rows.  Grid one-dimensional: (units 4096 / 256)
// workgroups per limb, the limb fastest (md_limb).
template <class A, class IO, int L1>
__global__ __launch_bounds__(256) void k_tmd_cols_fwd(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const BconvTo<typename A::word> *__restrict__ to, const typename A::word *__restrict__ wt,
    const BconvTo<typename A::word> *__restrict__ tt, const typename A::word *__restrict__ gt,
    const typename A::word *__restrict__ y, typename A::word *__restrict__ t, size_t units,
    uint32_t L, uint32_t K) {
  using W = typename A::word;
  constexpr int M = 1 << L1, logn = kMpLogs + L1;
  constexpr int KG = M < tm_cols_group<W, L1>() ? M : tm_cols_group<W, L1>();
  uint32_t l;
  size_t bx;
  md_limb(L, l, bx);
  const KParams<A> P = mp_limb_params<A>(tab, tw, l, (uint32_t)logn);
  const BconvTo<W> C = to[l], T = tt[0];
  const size_t gid = bx * blockDim.x + threadIdx.x;
  if (gid >= (units << kMpLogs)) return;
  const size_t u = gid >> kMpLogs, col = gid & (((size_t)1 << kMpLogs) - 1);
  const W *yp = y + ((u * K) << logn) + col;
  W x[M];
#pragma clang loop unroll(full)
  for (int g0 = 0; g0 < M; g0 += KG) {
    W r[KG];
    tm_sum<W, KG>(r, yp, (size_t)1 << logn, K, wt + l, bconv_pad(L), gt, bconv_pad(1), C, T,
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

}  // namespace nttmul
