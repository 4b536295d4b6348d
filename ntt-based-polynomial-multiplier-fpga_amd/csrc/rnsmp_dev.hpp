// rnsmp_dev.hpp — the limb-aware multi-pass kernels of include/nttmul_rnsmp.h
// (lib/libnttmul_rnsmp.so only): three launches per operation over all limbs of an RNS basis,
// operands [batch][limbs][n] with 4096 < n <= 65536.  Device code; its launchers are in rnsmp.hip.
// It reuses the transform stages, exchanges, base multiplication and load / store helpers of
// kernels_dev.hpp and mac_add of mac_dev.hpp unchanged and adds no function to them.
//
// The split is 2^L1 x 4096 (L1 = logn - 12 in 1 .. 4) for both word classes: a column pass over
// the L1 outer stages (k_cols_fwd / k_cols_inv's bodies) and a row pass over rows of 4096
// (k_rows / k_xform's bodies at LOGS = 12).  The intermediates live in the context's scratch with
// the operands' own layout, so one index algebra serves caller memory and scratch:
//
//   polynomial u of limb l starts at word (u L + l) << logn                     (L = limbs)
//   its row r (r < 2^L1) at word          (((u L + l) << L1) | r) * 4096
//   its column c (c < 4096), element m at ((u L + l) << logn) + c + (m << 12)
//
// u is a polynomial of the batch, or a (polynomial, term) pair p terms + t of the mac's a.
//
// The limb is blockIdx.y, as in rns_dev.hpp: the limb's KParams<A> is entry blockIdx.y of a
// per-family table, read by scalar loads, and its twiddle pointers are formed from the kernel
// argument tw (mp_limb_params), never read from the table, so the twiddle loads stay global.
#pragma once
#include "mac_dev.hpp"

namespace nttmul {

constexpr int kMpLogs = 12;  // rows of 4096

// rns_dev.hpp limb_params with n = 2^logn at run time: fw of limb l at pair 2 l n, iw at (2 l + 1) n
template <class A>
__device__ __forceinline__ KParams<A> mp_limb_params(const KParams<A> *__restrict__ tab,
                                                     const TwPair<typename A::word> *__restrict__ tw,
                                                     uint32_t l, uint32_t logn) {
  KParams<A> P = tab[l];
  P.fw = tw + (((size_t)l * 2) << logn);
  P.iw = P.fw + ((size_t)1 << logn);
  return P;
}

// Column pass, forward: k_cols_fwd's body on a grid (ceil(units 4096 / 256), limbs).  Thread = one
// column of one unit of limb blockIdx.y; 4096 is a multiple of 256, so a workgroup's columns stay
// inside one polynomial of one limb.  NPOLY 2: a and b of a product; 1: the forward transform and
// the mac's a (units = batch terms).  Non-temporal loads and stores, as k_cols_fwd's.
template <class A, class IO, int L1, int NPOLY>
__global__ __launch_bounds__(256) void k_rnsmp_cols_fwd(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const IO *__restrict__ a, const IO *__restrict__ b, typename A::word *__restrict__ ta,
    typename A::word *__restrict__ tb, size_t units, uint32_t limbs, int logs) {
  using W = typename A::word;
  constexpr int M = 1 << L1;
  const uint32_t l = blockIdx.y;
  const KParams<A> P = mp_limb_params<A>(tab, tw, l, (uint32_t)(logs + L1));
  const size_t ncol = (size_t)1 << logs;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= units * ncol) return;
  const size_t u = gid >> logs, col = gid & (ncol - 1);
  const size_t base = ((u * limbs + l) << (logs + L1)) + col;
  W x[M], y[M];
#pragma clang loop unroll(full)
  for (int m = 0; m < M; m++) {
    x[m] = (W)ld_stream<true>(a + base + ((size_t)m << logs));
    y[m] = NPOLY == 2 ? (W)ld_stream<true>(b + base + ((size_t)m << logs)) : W(0);
  }
#pragma clang loop unroll(full)
  for (int st = 0; st < L1; st++) {
    const int dist = M >> (st + 1);
#pragma clang loop unroll(full)
    for (int m = 0; m < M; m++) {
      if (m & dist) continue;
      const TwPair<W> t = P.fw[(1 << st) + (m >> (L1 - st))];
      P.ar.ct(x[m], x[m + dist], t.w, t.ws);
      if (NPOLY == 2) P.ar.ct(y[m], y[m + dist], t.w, t.ws);
    }
  }
#pragma clang loop unroll(full)
  for (int m = 0; m < M; m++) {
    st_stream<true>(ta + base + ((size_t)m << logs), x[m]);
    if (NPOLY == 2) st_stream<true>(tb + base + ((size_t)m << logs), y[m]);
  }
}

// Column pass, inverse: k_cols_inv's body with the same addressing.  The scale of the table's
// family (F 2^D after the product rows, F after the mac, n^-1 after the inverse transform's rows)
// is folded into stage 0; canonical words to the caller's c / out.
template <class A, class IO, int L1>
__global__ __launch_bounds__(256) void k_rnsmp_cols_inv(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const typename A::word *__restrict__ tc, IO *__restrict__ c, size_t units, uint32_t limbs,
    int logs) {
  using W = typename A::word;
  constexpr int M = 1 << L1;
  const uint32_t l = blockIdx.y;
  const KParams<A> P = mp_limb_params<A>(tab, tw, l, (uint32_t)(logs + L1));
  const size_t ncol = (size_t)1 << logs;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= units * ncol) return;
  const size_t u = gid >> logs, col = gid & (ncol - 1);
  const size_t base = ((u * limbs + l) << (logs + L1)) + col;
  W x[M];
#pragma clang loop unroll(full)
  for (int m = 0; m < M; m++) x[m] = ld_stream<true>(tc + base + ((size_t)m << logs));
#pragma clang loop unroll(full)
  for (int st = L1 - 1; st >= 0; st--) {
    const int dist = M >> (st + 1);
#pragma clang loop unroll(full)
    for (int m = 0; m < M; m++) {
      if (m & dist) continue;
      if (st == 0) {
        P.ar.gs_scaled(x[m], x[m + dist], P.f, P.fs, P.wf, P.wfs);
      } else {
        const TwPair<W> t = P.iw[(1 << st) + (m >> (L1 - st))];
        P.ar.gs(x[m], x[m + dist], t.w, t.ws);
      }
    }
  }
#pragma clang loop unroll(full)
  for (int m = 0; m < M; m++)
    st_stream<true>(c + base + ((size_t)m << logs),
                    (IO)(A::kInvCanonical ? x[m] : P.ar.canon_inv(x[m])));
}

// The row of unit v = (p << L1 | row) of limb l, in words from the start of a [..][limbs][n] array
template <int L1>
__device__ __forceinline__ size_t mp_row_word(size_t p, int row, uint32_t limbs, uint32_t l) {
  return ((((p * limbs + l) << L1) | (size_t)row) << kMpLogs);
}

// Row pass of the product: the body of k_rows<A, W, W, 12, L1> (one row of 4096 per workgroup,
// fwd_all / base_mult / inv_all with D = A::kBaseD, temporal loads and stores of the
// intermediates, lazy output) without the hooks, the clock stamps, the priority variant and the
// descriptor path.  Grid (batch << L1, limbs).  tab: product_params per limb (scale F 2^D, read
// by k_rnsmp_cols_inv).
template <class A, int L1>
__global__ __launch_bounds__(rows_threads(kMpLogs)) void k_rnsmp_rows(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const typename A::word *__restrict__ a, const typename A::word *__restrict__ b,
    typename A::word *__restrict__ c, size_t units, uint32_t limbs) {
  using W = typename A::word;
  using Gr = Groups<kMpLogs>;
  constexpr int N = Gr::N, TP = N / 16, G = Gr::G, NP = Gr::NP;
  static_assert(rows_threads(kMpLogs) == TP && L1 >= 1 && L1 <= 4, "one row of 4096 per workgroup");
  __shared__ W lds[NP];
  const uint32_t l = blockIdx.y;
  const KParams<A> P = mp_limb_params<A>(tab, tw, l, kMpLogs + L1);
  const int j = threadIdx.x;
  const size_t u = blockIdx.x;
  if (u >= units) return;  // (grid = units exactly; block-uniform)
  const int row = (int)(u & ((1u << L1) - 1));
  const size_t base = mp_row_word<L1>(u >> L1, row, limbs, l) + Gr::base(0, j);
  W x[16], y[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    x[k] = ld_stream<false>(a + base + Gr::off(0, k));
    y[k] = ld_stream<false>(b + base + Gr::off(0, k));
  }
  constexpr int D = A::kBaseD;
  TwPair<W> zw[16];
  fwd_all<A, kMpLogs, 0, 2, D>(P.ar, x, y, lds, P.fw, j, row, L1, zw);
  base_mult<A, kMpLogs, D>(P.ar, x, y, zw);
  inv_all<A, kMpLogs, G - 1, false, D>(P, x, y, lds, P.iw, j, row, L1);
#pragma unroll
  for (int k = 0; k < 16; k++) st_stream<false>(c + base + Gr::off(0, k), x[k]);
}

// Row pass of the standalone transforms: k_xform<A, .., 12, L1, DIR>, one polynomial row per
// thread group.  DIR 0 (tab: make_params): reads the scratch after k_rnsmp_cols_fwd, writes
// bit-reversed canonical words to the caller's out.  DIR 1 (tab: the fi / wfi scale, read by
// k_rnsmp_cols_inv): reads the caller's in, writes lazy words to the scratch.  in and out are
// never the same buffer here (one of them is the scratch), which is why out == in needs nothing
// special from the caller's side.
template <class A, class IO, int L1, int DIR>
__global__ __launch_bounds__(256) void k_rnsmp_xform(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const IO *__restrict__ in, IO *__restrict__ out, size_t units, uint32_t limbs) {
  using W = typename A::word;
  using Gr = Groups<kMpLogs>;
  constexpr int N = Gr::N, TP = N / 16, G = Gr::G, NP = Gr::NP;
  constexpr int GIN = DIR == 0 ? 0 : G - 1, GOUT = DIR == 0 ? G - 1 : 0;
  static_assert(TP == 256 && sizeof(IO) == sizeof(W) && xform_upg<A, L1, DIR>() == 1,
                "one row of 4096 per workgroup, scratch words = operand words");
  __shared__ W lds[NP];
  const uint32_t l = blockIdx.y;
  const KParams<A> P = mp_limb_params<A>(tab, tw, l, kMpLogs + L1);
  const int j = threadIdx.x;
  const size_t u = blockIdx.x;
  if (u >= units) return;  // (grid = units exactly; block-uniform)
  const int row = (int)(u & ((1u << L1) - 1));
  const size_t word0 = mp_row_word<L1>(u >> L1, row, limbs, l);
  const size_t base_in = word0 + Gr::base(GIN, j), base_out = word0 + Gr::base(GOUT, j);
  W x[16], y[16];
#pragma unroll
  for (int k = 0; k < 16; k++) x[k] = to_word<W>(in[base_in + Gr::off(GIN, k)]);
  TwPair<W> zw[16];
  if (DIR == 0)
    fwd_all<A, kMpLogs, 0, 1>(P.ar, x, y, lds, P.fw, j, row, L1, zw);
  else
    inv_all<A, kMpLogs, G - 1, false, 0, 0, 1>(P, x, y, lds, P.iw, j, row, L1);
#pragma unroll
  for (int k = 0; k < 16; k++) {
    W v = x[k];
    if (DIR == 0) v = P.ar.canon(v);
    out[base_out + Gr::off(GOUT, k)] = (IO)v;
  }
}

// Row pass of the mac, all terms in one launch.  Row (p, row) of limb l, for each t < terms:
// the column-passed row of a[p][t] from the scratch ta ([batch terms][limbs][n]), fwd_all with
// SKIP = 0 at (row, L1), the 16 words of b_hat[p or 0][t]'s row at the addresses
// k_rnsmp_xform<.., 0> stores to, one mont each, mac_add into 16 accumulators; then inv_all
// (unscaled: F is in k_rnsmp_cols_inv, tab: make_params) and the row to the output scratch tc
// ([batch][limbs][n]).  Range contract per class: k_mac's (mac_dev.hpp), except that the forward
// rows read the column pass's lazy words, as k_xform<.., L1 > 0, 0> does.  b_hat loads stay
// temporal (a shared operand is re-read by every polynomial), placed as in k_mac: before the
// transform on 32-bit words, after it on 64-bit words.
template <class A, class IO, int L1>
__global__ __launch_bounds__(256) void k_rnsmp_mac(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const typename A::word *__restrict__ ta, const IO *__restrict__ bh,
    typename A::word *__restrict__ tc, size_t units, uint32_t terms, uint32_t bpolys,
    uint32_t limbs) {
  using W = typename A::word;
  using Gr = Groups<kMpLogs>;
  constexpr int N = Gr::N, TP = N / 16, G = Gr::G, NP = Gr::NP;
  static_assert(TP == 256, "one row of 4096 per workgroup");
  __shared__ W lds[NP];
  const uint32_t l = blockIdx.y;
  const KParams<A> P = mp_limb_params<A>(tab, tw, l, kMpLogs + L1);
  const int j = threadIdx.x;
  const size_t u = blockIdx.x;
  if (u >= units) return;  // (grid = units exactly; block-uniform)
  const int row = (int)(u & ((1u << L1) - 1));
  const size_t p = u >> L1, step = (size_t)limbs << (kMpLogs + L1);
  const W *ap = ta + mp_row_word<L1>(p * terms, row, limbs, l) + Gr::base(0, j);
  const IO *bp = bh + mp_row_word<L1>(p * bpolys, row, limbs, l) + Gr::base(G - 1, j);
  W acc[16], y[16];
#pragma unroll
  for (int k = 0; k < 16; k++) acc[k] = 0;
  for (uint32_t t = 0; t < terms; t++, ap += step, bp += step) {
    W x[16], bv[16];
#pragma unroll
    for (int k = 0; k < 16; k++) x[k] = ap[Gr::off(0, k)];
    constexpr bool kEarlyB = sizeof(W) == 4;
    if constexpr (kEarlyB) {
#pragma unroll
      for (int k = 0; k < 16; k++) bv[k] = to_word<W>(bp[Gr::off(G - 1, k)]);
    }
    TwPair<W> zw[16];
    fwd_all<A, kMpLogs, 0, 1, 0>(P.ar, x, y, lds, P.fw, j, row, L1, zw);
    if constexpr (!kEarlyB) {
#pragma unroll
      for (int k = 0; k < 16; k++) bv[k] = to_word<W>(bp[Gr::off(G - 1, k)]);
    }
#pragma unroll
    for (int k = 0; k < 16; k++) acc[k] = mac_add(P.ar, acc[k], P.ar.mont(x[k], bv[k]));
  }
  inv_all<A, kMpLogs, G - 1, false, 0>(P, acc, y, lds, P.iw, j, row, L1);
  W *cp = tc + mp_row_word<L1>(p, row, limbs, l) + Gr::base(0, j);
#pragma unroll
  for (int k = 0; k < 16; k++) cp[Gr::off(0, k)] = acc[k];
}

}  // namespace nttmul
