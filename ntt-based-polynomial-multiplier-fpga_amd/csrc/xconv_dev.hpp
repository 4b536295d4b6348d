// xconv_dev.hpp — the kernels of include/nttmul_xconv.h (lib/libnttmul_xconv.so only): the exact
// base extension p_hat [batch][K][n] -> out [batch][L][n] and the rounded ModDown
// x_hat [batch][L + K][n] -> out [batch][L][n], every limb a transform.  Device code; its launchers
// are in xconv.hip.  It reuses md_group's idea, md_limb and md_epilogue (mdntt_dev.hpp), fwd_all
// and the stream loads and stores of kernels_dev.hpp, limb_params (rns_dev.hpp), mp_limb_params /
// mp_row_word (rnsmp_dev.hpp) and BconvArith<W> (bconv_dev.hpp: mulc, mac, fold, reduce and the
// fold cadences) unchanged and adds no function to them.
//
//   y_j       = INTT_{p_j}(in[p][.. + j]) (t Ph_j^-1 mod p_j)             canonical, in the scratch
//   phi[k]    = sum_j y_j[k] / p_j                                       double, fixed order
//   a[k]      = floor(phi[k] + 1/2)                                      0 .. K
//   r_l[k]    = (sum_j y_j[k] (w_j R mod q_l) + a[k] (w_K R mod q_l)) R^-1 mod q_l     canonical
//   extend    w_j = Ph_j, w_K = -P:            out[p][l] = canon(NTT_{q_l}(r_l))
//   moddown   w_j = Ph_j t^-1, w_K = -P t^-1:  out[p][l] = (x_hat[p][l] - canon(NTT_{q_l}(r_l)) + q_l)
//                                                          (t P^-1 mod q_l) mod q_l
//
// The inverse half is mdntt_dev.hpp's own (k_mdntt_inv, or k_mdntt_inv_rows and the library's
// k_rnsmp_cols_inv above n = 4096), launched through mdntt.hip with a table whose scale carries
// n^-1 Ph_j^-1 t; extend launches it with (L, K) := (0, K), as ksntt.cpp does.  The forward half
// is new: k_xconv_fwd<.., OP> at n <= 4096; above, k_xconv_cols_fwd, then k_xconv_rows (extend) or
// mdntt_dev.hpp's k_mdntt_rows, whose epilogue reads v = t P^-1 from the table (moddown).
//
// Grid order: md_limb's, one-dimensional with the target limb fastest, with plain loads and stores
// (mdntt_dev.hpp md_epilogue records why).  The weights and 1 / p_j stay a scalar load per j.
//
// The guard band of a.  u = 2^-53.  Per term: (double)y_j = y_j (1 + d1), |d1| <= u (exact on
// 32-bit words); the table's 1 / p_j = (1 / p_j)(1 + d2), |d2| <= u; so the product the fused
// multiply-add forms exactly errs by less than y_j / p_j (2u + u^2) < 2^-51.  The fma rounds the
// running sum once; every partial sum is below K <= 63 < 64, so that rounding is at most half an
// ulp of [32, 64) = 2^-48.  After K terms |phi_computed - phi| < K (2^-48 + 2^-51), and phi + 0.5
// (below 64 as well) rounds once more, by at most 2^-48.  In all the computed phi + 1/2 is within
// (K + 1)(2^-48 + 2^-51) <= K 2^-46 of the true one, so its floor is the true a whenever the true
// phi + 1/2 is farther than eps = K 2^-46 from an integer: kXcBandLog2 = 46 (xconv_plan.hpp), well
// inside the K 2^-40 the interface allows.  Inside the band the floor is the true a or a neighbour,
// so c is off by one P at most.  The sum is written with __builtin_fma in the loop's order and
// contraction is off in xc_sum: every workgroup of a call computes the same a from the same y.
//
// Range contract, per arithmetic class: mdntt_dev.hpp's with K + 1 for K, the (K + 1)-th product
// being a (w_K R mod q_l) with a <= K <= 63, inside every y range.
//   Arith32P  y <= p_j - 1, a <= 63, w <= C - 1, all < 2^31: bconv_dev.hpp's 64-bit accumulator,
//             a fold after every 2 products, for any K + 1 <= 64 (a last group of 1 product is
//             folded as well, and the correction is a group of its own); r = reduce(folded) in
//             [0, C).  fwd_all reads canonical words and leaves t in [0, 2C); canon(t) in [0, C);
//             moddown: x - canon(t) + C in (0, 2C) < 2^32, which mulc takes and returns canonical.
//   Arith64   y <= p_j - 1, a <= 63, w <= C - 1, all < 2^62: the four 31-bit limb sums, a fold after
//             every 4 products, for any K + 1 <= 64 (a last group of 1 .. 3 is folded as well, and
//             the correction is a group of its own); r in [0, C).  fwd_all (Harvey CT) reads [0, 4C) and leaves t in
//             [0, 4C); canon(t) in [0, C); moddown: x - canon(t) + C in (0, 2C) < 2^63 for mulc.
// The multi-pass pair splits the same chain at the column pass, as mdntt_dev.hpp's does.
#pragma once
#include "mdntt_dev.hpp"
#include "xconv_plan.hpp"

namespace nttmul {

// coefficients converted together: the accumulators of md_group and a double each.  Half of
// md_group's 16 on 32-bit words, so that the accumulators and the phi together take the registers
// md_sum's accumulators take
template <class W>
constexpr int xc_group() { return sizeof(W) == 4 ? 8 : 4; }

// md_sum with phi accumulated beside it and the correction as the (K + 1)-th product.  yp, step,
// wl, lpad, C, off as md_sum's; wl has K + 1 rows; ip: 1 / p_j as doubles, [K].  j is a loop
// counter and wl, ip, C are wave-uniform: scalar loads.
template <class W, int KG, class Off>
__device__ __forceinline__ void xc_sum(W (&r)[KG], const W *__restrict__ yp, size_t step,
                                       uint32_t K, const W *__restrict__ wl, uint32_t lpad,
                                       const double *__restrict__ ip, const BconvTo<W> &C,
                                       Off off) {
#pragma clang fp contract(off)
  using Ar = BconvArith<W>;
  constexpr int CAD = Ar::kCadence;
  typename Ar::Acc acc[KG];
  double phi[KG];
#pragma unroll
  for (int k = 0; k < KG; k++) {
    acc[k] = Ar::zero();
    phi[k] = 0.0;
  }
  const auto term = [&](uint32_t j) {
    const W w = wl[(size_t)j * lpad];
    const double ipj = ip[j];
    const W *yj = yp + (size_t)j * step;
#pragma unroll
    for (int k = 0; k < KG; k++) {
      const W y = yj[off(k)];
      Ar::mac(acc[k], y, w);
      phi[k] = __builtin_fma((double)y, ipj, phi[k]);
    }
  };
  const auto fold = [&] {
#pragma unroll
    for (int k = 0; k < KG; k++) Ar::fold(acc[k], C.cr);
  };
  // CAD products, a fold; the last group may be shorter and is folded as well (md_sum's loop);
  // then the correction, one product, and its fold: reduce always reads a folded accumulator.
  // (The correction in the last group's fold saves a fold where K is no multiple of CAD, and
  // cost the 64-bit k_xconv_fwd a wave per SIMD in the listing: 252 to 262 VGPRs for 159 to 167,
  // DESIGN.md section 4.)
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
  const W wa = wl[(size_t)K * lpad];
#pragma unroll
  for (int k = 0; k < KG; k++) Ar::mac(acc[k], (W)(uint32_t)(phi[k] + 0.5), wa);
  fold();
#pragma unroll
  for (int k = 0; k < KG; k++) r[k] = Ar::reduce(acc[k], C);
}

// k_mdntt_fwd's body with the corrected sum.  OP kXcModdown: x_hat [batch][L + K][n], the
// epilogue on the 16 words of x_hat[p][l].  OP kXcExtend: no x_hat (xh is not read), canon(t) is
// stored, as k_ksntt_fwd stores it.  tab, tw, to, y, out, batch, L, K as k_mdntt_fwd's; wt has
// K + 1 rows padded to bconv_pad(L); ip [K].  Thread groups past the batch end read polynomial 0
// and never store.
template <class A, class IO, int LOGS, int OP>
__global__ __launch_bounds__(256) void k_xconv_fwd(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const BconvTo<typename A::word> *__restrict__ to, const typename A::word *__restrict__ wt,
    const double *__restrict__ ip, const typename A::word *__restrict__ y,
    const IO *__restrict__ xh, IO *__restrict__ out, size_t batch, uint32_t L, uint32_t K) {
  using W = typename A::word;
  using Gr = Groups<LOGS>;
  constexpr int N = Gr::N, TP = N / 16, PB = 256 / TP, G = Gr::G, NP = Gr::NP;
  constexpr int KG = xc_group<W>();
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
  const W *yp = y + pl * K * N + Gr::base(0, j);
  W x[16], unused[16];
#pragma unroll
  for (int g0 = 0; g0 < 16; g0 += KG) {
    W r[KG];
    xc_sum<W, KG>(r, yp, N, K, wt + l, bconv_pad(L), ip, C,
                  [&](int k) { return Gr::off(0, g0 + k); });
#pragma unroll
    for (int k = 0; k < KG; k++) x[g0 + k] = r[k];
  }
  TwPair<W> zw[16];
  fwd_all<A, LOGS, 0, 1>(P.ar, x, unused, lds[pb], P.fw, j, 0, 0, zw);
  IO *op = out + (pl * L + l) * N + Gr::base(G - 1, j);
  if constexpr (OP == kXcModdown) {
    // (after the transform in both classes: the sums hold a double per coefficient more than
    // k_mdntt_fwd's, and 16 more live words under them cost registers)
    const IO *xp = xh + (pl * (L + K) + l) * N + Gr::base(G - 1, j);
    W xv[16];
#pragma unroll
    for (int k = 0; k < 16; k++) xv[k] = to_word<W>(xp[Gr::off(G - 1, k)]);
    if (live) {
#pragma unroll
      for (int k = 0; k < 16; k++)
        op[Gr::off(G - 1, k)] = (IO)md_epilogue<A>(P.ar, x[k], xv[k], C);
    }
  } else {
    if (live) {
#pragma unroll
      for (int k = 0; k < 16; k++) op[Gr::off(G - 1, k)] = (IO)P.ar.canon(x[k]);
    }
  }
}

// k_mdntt_cols_fwd's body with the corrected sum; both operations (their weights differ, not the
// kernel).  Grid one-dimensional: (units 4096 / 256) workgroups per limb, the limb fastest.
template <class A, class IO, int L1>
__global__ __launch_bounds__(256) void k_xconv_cols_fwd(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const BconvTo<typename A::word> *__restrict__ to, const typename A::word *__restrict__ wt,
    const double *__restrict__ ip, const typename A::word *__restrict__ y,
    typename A::word *__restrict__ t, size_t units, uint32_t L, uint32_t K) {
  using W = typename A::word;
  constexpr int M = 1 << L1, logn = kMpLogs + L1;
  constexpr int KG = M < xc_group<W>() ? M : xc_group<W>();
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
    xc_sum<W, KG>(r, yp, (size_t)1 << logn, K, wt + l, bconv_pad(L), ip, C,
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

// extend's row pass: k_mdntt_rows without x_hat and with canon(t) stored.  (k_rnsmp_xform<.., 0>
// would do the same work, but its launcher takes one table over the limbs of both operands, and
// k_ksntt_rows runs in place on a [dnum][L + K] layout: neither fits as it stands.)  Row `row`
// of (p, l) from t ([cnt][L][n], after k_xconv_cols_fwd), fwd_all at (row, L1).  Grid
// one-dimensional: units = cnt << L1 rows per limb, the limb fastest (md_limb).
template <class A, class IO, int L1>
__global__ __launch_bounds__(256) void k_xconv_rows(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const typename A::word *__restrict__ t, IO *__restrict__ out, size_t units, uint32_t L) {
  using W = typename A::word;
  using Gr = Groups<kMpLogs>;
  constexpr int N = Gr::N, TP = N / 16, G = Gr::G, NP = Gr::NP;
  static_assert(TP == 256 && sizeof(IO) == sizeof(W), "one row of 4096 per workgroup");
  __shared__ W lds[NP];
  uint32_t l;
  size_t u;
  md_limb(L, l, u);
  const KParams<A> P = mp_limb_params<A>(tab, tw, l, kMpLogs + L1);
  const int j = threadIdx.x;
  if (u >= units) return;  // (grid = units L exactly; block-uniform)
  const int row = (int)(u & ((1u << L1) - 1));
  const size_t word_q = mp_row_word<L1>(u >> L1, row, L, l);
  W x[16], unused[16];
#pragma unroll
  for (int k = 0; k < 16; k++)
    x[k] = ld_stream<false>(t + word_q + Gr::base(0, j) + Gr::off(0, k));
  TwPair<W> zw[16];
  fwd_all<A, kMpLogs, 0, 1>(P.ar, x, unused, lds, P.fw, j, row, L1, zw);
  IO *op = out + word_q + Gr::base(G - 1, j);
#pragma unroll
  for (int k = 0; k < 16; k++) op[Gr::off(G - 1, k)] = (IO)P.ar.canon(x[k]);
}

}  // namespace nttmul
