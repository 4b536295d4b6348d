// rns_dev.hpp — the limb-aware kernels of include/nttmul_rns.h (lib/libnttmul_rns.so only): one
// launch over all limbs of an RNS basis, operands [batch][limbs][n] with n <= 4096.  Device code;
// its launchers are in rns.hip.  It reuses the transform stages, exchanges, base multiplication
// and load / store helpers of kernels_dev.hpp (and mac_add of mac_dev.hpp) unchanged and adds no
// function to them.
//
// The limb is a grid dimension: blockIdx.y = limb, blockIdx.x over ceil(batch / PB).  The PB
// polynomials of a workgroup share their limb, and its constants -- modulus, Plantard / Shoup
// constants, folded scale: one KParams<A> -- are entry blockIdx.y of a table in device memory
// (the twiddle pointers come from a kernel argument, limb_params below).  The index is a blockIdx
// expression, so the compiler knows it wave-uniform and reads the entry with scalar loads into
// SGPRs, where k_rows keeps its kernel argument; a per-lane limb would put q and every constant
// into VGPRs.  Polynomial p of limb l starts at word (p L + l) n.
#pragma once
#include "mac_dev.hpp"

namespace nttmul {

// A limb's table entry, with its twiddle pointers formed from the kernel argument tw.  The limbs'
// twiddle tables are one allocation (rns.cpp setup_device): fw of limb l at pair 2 l n, iw at
// (2 l + 1) n, which is also what the entry's own fw / iw hold.  A pointer that arrives as a
// kernel argument is known to be global memory; one loaded from a table is generic to the
// compiler, which then reads every twiddle with flat loads (counted against the LDS exchanges'
// lgkmcnt as well as vmcnt).
template <class A, int N>
__device__ __forceinline__ KParams<A> limb_params(const KParams<A> *__restrict__ tab,
                                                  const TwPair<typename A::word> *__restrict__ tw,
                                                  uint32_t l) {
  KParams<A> P = tab[l];
  P.fw = tw + (size_t)l * (2 * N);
  P.iw = P.fw + N;
  return P;
}

// Fused products: the body of k_rows<A, IO, IO, LOGS, 0> (same block shape, same load and store
// forms, fwd_all / base_mult / inv_all with D = A::kBaseD) without the hooks, the clock stamps and
// the issue-priority variant.  tab: product_params per limb (scale F 2^D).
template <class A, class IO, int LOGS>
__global__ __launch_bounds__(rows_threads(LOGS)) void k_rns_rows(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const IO *__restrict__ a, const IO *__restrict__ b, IO *__restrict__ c, size_t batch,
    uint32_t limbs) {
  using W = typename A::word;
  using Gr = Groups<LOGS>;
  constexpr int N = Gr::N, TP = N / 16, PB = rows_threads(LOGS) / TP, G = Gr::G, NP = Gr::NP;
  __shared__ W lds[PB][NP];
  const uint32_t l = blockIdx.y;
  const KParams<A> P = limb_params<A, N>(tab, tw, l);
  const int pb = threadIdx.x / TP, j = threadIdx.x % TP;
  const size_t p = (size_t)blockIdx.x * PB + pb;
  const bool live = p < batch;
  // threads past the batch end read polynomial 0 of the limb (always valid) instead of branching
  // per load; their results are never stored
  const size_t base_g = (p * limbs + l) * N + Gr::base(0, j);
  const size_t base_r = live ? base_g : (size_t)l * N + Gr::base(0, j);
  W x[16], y[16];
  // one product per block on 32-bit words: buffer loads / stores on a block-uniform descriptor
  // with nt cache policy, each register's constant offset in the scalar offset (k_rows kCpol)
  constexpr bool kCpol = PB == 1 && sizeof(W) == 4 && sizeof(IO) == 4;
  if constexpr (kCpol) {
    const size_t ub = ((live ? (size_t)blockIdx.x : 0) * limbs + l) * N;
    const auto ra = span_rsrc(a + ub, N), rb = span_rsrc(b + ub, N);
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int vo = Gr::base(0, j) * 4, so = Gr::off(0, k) * 4;
      x[k] = (W)buf_ld32<kAuxNt>(ra, vo, so);
      y[k] = (W)buf_ld32<kAuxNt>(rb, vo, so);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++) {
      x[k] = to_word<W>(ld_stream<true>(a + base_r + Gr::off(0, k)));
      y[k] = to_word<W>(ld_stream<true>(b + base_r + Gr::off(0, k)));
    }
  }
  W *lx = lds[pb];
  constexpr int D = A::kBaseD;
  TwPair<W> zw[16];
  fwd_all<A, LOGS, 0, 2, D>(P.ar, x, y, lx, P.fw, j, 0, 0, zw);
  base_mult<A, LOGS, D>(P.ar, x, y, zw);
  inv_all<A, LOGS, G - 1, true, D>(P, x, y, lx, P.iw, j, 0, 0);
  if constexpr (kCpol) {
    if (live) {
      const auto rc = span_rsrc(c + ((size_t)blockIdx.x * limbs + l) * N, N);
#pragma unroll
      for (int k = 0; k < 16; k++) {
        W v = x[k];
        if (!A::kInvCanonical) v = P.ar.canon_inv(v);
        buf_st32<kAuxNt>(rc, Gr::base(0, j) * 4, (uint32_t)v, Gr::off(0, k) * 4);
      }
    }
    return;
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < 16; k++) {
      W v = x[k];
      if (!A::kInvCanonical) v = P.ar.canon_inv(v);
      st_stream<true>(c + base_g + Gr::off(0, k), (IO)v);
    }
  }
}

// Standalone transforms: k_xform<A, IO, IO, LOGS, 0, DIR> per limb.  DIR 0 forward (standard
// order in, bit-reversed canonical out; tab: make_params), DIR 1 inverse (bit-reversed in, scaled
// by n^-1, standard canonical out; tab: the fi / wfi scale).  32-bit words take two polynomials
// per thread group, (p, p + 1) of the same limb; an odd batch leaves the last group half empty.
// in == out is allowed (no __restrict__ on the two): a thread group reads its polynomials whole
// before the first exchange barrier and writes them after the last.
template <class A, class IO, int LOGS, int DIR>
__global__ __launch_bounds__(256) void k_rns_xform(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const IO *in, IO *out, size_t batch, uint32_t limbs) {
  using W = typename A::word;
  using Gr = Groups<LOGS>;
  constexpr int N = Gr::N, TP = N / 16, PB = 256 / TP, G = Gr::G, NP = Gr::NP;
  constexpr int GIN = DIR == 0 ? 0 : G - 1, GOUT = DIR == 0 ? G - 1 : 0;
  constexpr int UPG = xform_upg<A, 0, DIR>();
  // (k_xform's size: UPG == 2 uses the first region only, and the second keeps the workgroups per
  // CU, and with them the transforms' memory streams, what k_xform's are)
  __shared__ W lds[PB][UPG][NP];
  const uint32_t l = blockIdx.y;
  const KParams<A> P = limb_params<A, N>(tab, tw, l);
  const int pb = threadIdx.x / TP, j = threadIdx.x % TP;
  const size_t p = ((size_t)blockIdx.x * PB + pb) * UPG;
  const bool live = p < batch, live2 = UPG == 2 && p + 1 < batch;
  const auto word0 = [&](size_t v) { return (v * limbs + l) * N; };
  const size_t base_in = word0(live ? p : 0) + Gr::base(GIN, j);
  const size_t base_in2 = word0(live2 ? p + 1 : live ? p : 0) + Gr::base(GIN, j);
  W x[16], y[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    x[k] = to_word<W>(in[base_in + Gr::off(GIN, k)]);
    if (UPG == 2) y[k] = to_word<W>(in[base_in2 + Gr::off(GIN, k)]);
  }
  TwPair<W> zw[16];
  if (DIR == 0)
    fwd_all<A, LOGS, 0, UPG>(P.ar, x, y, lds[pb][0], P.fw, j, 0, 0, zw);
  else
    inv_all<A, LOGS, G - 1, true, 0, 0, UPG>(P, x, y, lds[pb][0], P.iw, j, 0, 0);
  if (live) {
    const size_t base_out = word0(p) + Gr::base(GOUT, j);
#pragma unroll
    for (int k = 0; k < 16; k++) {
      W v = x[k];
      if (DIR == 0)
        v = P.ar.canon(v);
      else if (!A::kInvCanonical)
        v = P.ar.canon_inv(v);
      out[base_out + Gr::off(GOUT, k)] = (IO)v;
    }
  }
  if (live2) {
    const size_t base_out = word0(p + 1) + Gr::base(GOUT, j);
#pragma unroll
    for (int k = 0; k < 16; k++) {
      W v = y[k];
      if (DIR == 0)
        v = P.ar.canon(v);
      else if (!A::kInvCanonical)
        v = P.ar.canon_inv(v);
      out[base_out + Gr::off(GOUT, k)] = (IO)v;
    }
  }
}

// Fused multiply-accumulate against NTT-domain operands: k_mac per limb, with its range contract
// per class (mac_dev.hpp) and its temporal b_hat loads.  Polynomial (p, t) of a starts at word
// ((p terms + t) L + l) n, of b_hat at ((p bpolys + t) L + l) n with bpolys = terms, or 0 when one
// [terms][L][n] operand is shared by the batch.  tab: make_params (scale F).
template <class A, class IO, int LOGS>
__global__ __launch_bounds__(256) void k_rns_mac(
    const KParams<A> *__restrict__ tab, const TwPair<typename A::word> *__restrict__ tw,
    const IO *__restrict__ a, const IO *__restrict__ bh, IO *__restrict__ c, size_t batch,
    uint32_t terms, uint32_t bpolys, uint32_t limbs) {
  using W = typename A::word;
  using Gr = Groups<LOGS>;
  constexpr int N = Gr::N, TP = N / 16, PB = 256 / TP, G = Gr::G, NP = Gr::NP;
  __shared__ W lds[PB][NP];
  const uint32_t l = blockIdx.y;
  const KParams<A> P = limb_params<A, N>(tab, tw, l);
  const int pb = threadIdx.x / TP, j = threadIdx.x % TP;
  const size_t p = (size_t)blockIdx.x * PB + pb;
  const bool live = p < batch;
  const size_t pl = live ? p : 0, step = (size_t)limbs * N;
  const IO *ap = a + (pl * terms * limbs + l) * N + Gr::base(0, j);
  const IO *bp = bh + (pl * bpolys * limbs + l) * N + Gr::base(G - 1, j);
  W acc[16], y[16];
#pragma unroll
  for (int k = 0; k < 16; k++) acc[k] = 0;
  for (uint32_t t = 0; t < terms; t++, ap += step, bp += step) {
    W x[16], bv[16];
#pragma unroll
    for (int k = 0; k < 16; k++) x[k] = to_word<W>(ld_stream<true>(ap + Gr::off(0, k)));
    // (k_mac: 32-bit words load b_hat before the transform, 64-bit words after it)
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
    IO *cp = c + (p * limbs + l) * N + Gr::base(0, j);
#pragma unroll
    for (int k = 0; k < 16; k++) {
      W v = acc[k];
      if (!A::kInvCanonical) v = P.ar.canon_inv(v);
      st_stream<true>(cp + Gr::off(0, k), (IO)v);
    }
  }
}

// NTTMUL_FLAG_VALIDATE: word i of an operand belongs to limb (i / n) mod limbs
template <class T>
__global__ void k_rns_check_range(const T *__restrict__ a, const uint64_t *__restrict__ q,
                                  size_t total, uint32_t logn, uint32_t limbs, int *bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if ((uint64_t)a[i] >= q[(i >> logn) % limbs]) atomicOr(bad, 1);
}

}  // namespace nttmul
