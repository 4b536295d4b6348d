// level_dev.hpp — the kernels of include/nttmul_level.h (lib/libnttmul_level.so only): the three
// element-wise kernels that read a key, k_ksntt_mac (ksntt_dev.hpp), k_lintrans
// (lintrans_dev.hpp, the batch-sliced form the library builds) and k_ctmul_relin (ctmul_dev.hpp),
// with the key and the diagonals read through a level view.  Device code; the launchers are in
// level.hip.  It reuses mont (modarith.hpp), mac_add (mac_dev.hpp), BconvArith<W>::mulc
// (bconv_dev.hpp), galois_slot (galois_dev.hpp), each_comp (macn_dev.hpp) and ks_arith
// (ksntt_dev.hpp) unchanged, inside their stated domains, and adds no function to them.
//
// The bodies are the dense kernels' own, statement for statement: the same grids, the same
// slicing, the same V = 4 reuse of every key word, the same accumulators and the same final mulc.
// They are copies and not a shared template, so that the dense kernels' machine code is the
// parent's bit for bit (tests/test_level_ledger.py).  What differs is how the addresses of the
// viewed operands are formed.  A key is [outer][top_terms][top_limbs][n] and a diagonal set
// [outer][top_limbs][n], made for a chain of top_limbs - K primes of Q; the context has L <= that
// many, and reads limb l of term t at
//
//   kl = l < L ? l : l + (top_limbs - limbs)           (view_limb below)
//   word (o top_terms + t) top_limbs n + kl n + j      kstep = top_limbs n, kcstep = top_terms kstep
//
// l is blockIdx.y and every other quantity a kernel argument: kl, kstep and kcstep are
// wave-uniform and live in SGPRs; a lane adds its slot j once, before the term loop, as the dense
// kernels do.  Nothing of the view is per-lane and no lane reads a word the view does not select.
// The other operands (a_hat, up_hat, c0_hat, x_hat, y_hat, c_hat) are dense at the context's own
// level and addressed as in the dense kernels, with step = limbs n.
//
// Range contracts: the dense kernels', word for word; the arithmetic is not touched.
//
// k_level_check_range: k_rns_check_range (rns_dev.hpp) over exactly the words a view selects, one
// thread per selected word; its index is decomposed per lane (a check, not a hot path).
#pragma once
#include "ctmul_dev.hpp"
#include "level.hpp"
#include "lintrans_dev.hpp"

namespace nttmul {

// top(l) of include/nttmul_level.h: the operand's limb behind limb l of the context (block-uniform)
__device__ __forceinline__ uint32_t view_limb(uint32_t l, uint32_t L, uint32_t limbs,
                                              uint32_t top_limbs) {
  return l < L ? l : l + (top_limbs - limbs);
}

// k_ksntt_mac with b_hat viewed.  Grid and the addresses of a_hat and c_hat: k_ksntt_mac's.
// (r, i, t) of b_hat starts at word ((r COMPS + i) top_terms + t) top_limbs n + kl n.
template <class A, class IO, int COMPS>
__global__ __launch_bounds__(256) void k_level_mac(
    const BconvTo<typename A::word> *__restrict__ to, const IO *__restrict__ ah,
    const IO *__restrict__ bh, IO *__restrict__ c, GaloisKs ks, uint32_t rots, size_t slices,
    uint32_t terms, uint32_t L, uint32_t limbs, uint32_t top_limbs, uint32_t top_terms,
    uint32_t logn) {
  using W = typename A::word;
  static_assert(COMPS >= 1 && COMPS <= 2, "NTTMUL_MACN_MAX_COMPS");
  constexpr int V = kKsMacSlices;
  const uint32_t l = blockIdx.y, r = blockIdx.x % rots, kr = ks.k[r];
  const uint32_t kl = view_limb(l, L, limbs, top_limbs);
  const BconvTo<W> C = to[l];
  const A ar = ks_arith<A>(C);
  const uint32_t lgs = logn - 8, sh = 32 - logn, mask2 = (2u << logn) - 1;
  const size_t step = (size_t)limbs << logn;
  const size_t kstep = (size_t)top_limbs << logn, kcstep = kstep * top_terms;
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
    bp[v] = bh + ((size_t)r * COMPS * kcstep + ((size_t)kl << logn)) + j;
    cp[v] = c + ((((p * rots + r) * COMPS) * limbs + l) << logn) + j;
  }
  W acc[COMPS][V];
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
#pragma unroll
    for (int v = 0; v < V; v++) acc[i][v] = 0;
  });
  for (uint32_t t = 0; t < terms; t++) {
    const size_t o = (size_t)t * step, ko = (size_t)t * kstep;
    W x[V], bv[COMPS][V];
#pragma unroll
    for (int v = 0; v < V; v++) x[v] = to_word<W>(ap[v][o]);
    each_comp<COMPS>([&](auto ci) {
      constexpr int i = decltype(ci)::value;
#pragma unroll
      for (int v = 0; v < V; v++) bv[i][v] = to_word<W>(bp[v][i * kcstep + ko]);
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

// k_lintrans (batch-sliced, the range of 256 slots the faster index, V = kLtSlices) with b_hat
// and w_hat viewed.  Grid and the addresses of a_hat, c0_hat and c_hat: k_lintrans's.  (r, i, t)
// of b_hat starts at word ((r COMPS + i) top_terms + t) top_limbs n + kl n, r of w_hat at
// r top_limbs n + kl n.
template <class A, class IO, int COMPS, int WEIGHTED>
__global__ __launch_bounds__(256) void k_level_lintrans(
    const BconvTo<typename A::word> *__restrict__ to,
    const LtLimb<typename A::word> *__restrict__ lc, const IO *__restrict__ ah,
    const IO *__restrict__ bh, const IO *__restrict__ wh, const IO *__restrict__ c0,
    IO *__restrict__ c, GaloisKs ks, uint32_t rots, size_t units, uint32_t terms, uint32_t L,
    uint32_t limbs, uint32_t top_limbs, uint32_t top_terms, uint32_t logn) {
  using W = typename A::word;
  static_assert(COMPS >= 1 && COMPS <= 2, "NTTMUL_MACN_MAX_COMPS");
  static_assert(WEIGHTED == 0 || WEIGHTED == 1, "w_hat is given or not");
  constexpr int V = (int)kLtSlices;
  const uint32_t l = blockIdx.y;
  const uint32_t kl = view_limb(l, L, limbs, top_limbs);
  const BconvTo<W> C = to[l];
  const LtLimb<W> E = lc[l];
  const A ar = ks_arith<A>(C);
  const uint32_t lgs = logn - 8, sh = 32 - logn, mask2 = (2u << logn) - 1;
  const size_t step = (size_t)limbs << logn;
  const size_t kstep = (size_t)top_limbs << logn, kcstep = kstep * top_terms,
               krstep = kcstep * COMPS;
  const bool with_c0 = c0 != nullptr && l < L;  // (block-uniform)
  const uint32_t g = blockIdx.x >> lgs, s = blockIdx.x & ((1u << lgs) - 1);
  const uint32_t j = (s << 8) + threadIdx.x;
  const IO *bp = bh + ((size_t)kl << logn) + j;
  const IO *wp = WEIGHTED ? wh + ((size_t)kl << logn) + j : nullptr;
  bool live[V];
  const IO *ap[V], *zp[V];
  IO *cp[V];
#pragma unroll
  for (int v = 0; v < V; v++) {
    const size_t e = (size_t)g * V + v;
    live[v] = e < units;
    const size_t p = live[v] ? e : 0;
    ap[v] = ah + ((p * terms * limbs + l) << logn);
    zp[v] = with_c0 ? c0 + ((p * L + l) << logn) : nullptr;
    cp[v] = c + ((p * COMPS * limbs + l) << logn) + j;
  }
  W in[COMPS][V], out[COMPS][V];
  each_comp<COMPS>([&](auto ci) {
    constexpr int i = decltype(ci)::value;
#pragma unroll
    for (int v = 0; v < V; v++) in[i][v] = out[i][v] = 0;
  });
  for (uint32_t r = 0; r < rots; r++) {
    const uint32_t src = galois_slot(j, ks.k[r], sh, mask2);
    if constexpr (WEIGHTED) {
      each_comp<COMPS>([&](auto ci) {
        constexpr int i = decltype(ci)::value;
#pragma unroll
        for (int v = 0; v < V; v++) in[i][v] = 0;
      });
    }
    const size_t ro = (size_t)r * krstep;
    for (uint32_t t = 0; t < terms; t++) {
      const size_t o = (size_t)t * step, ko = (size_t)t * kstep;
      W x[V], bv[COMPS];
#pragma unroll
      for (int v = 0; v < V; v++) x[v] = to_word<W>(ap[v][o + src]);
      each_comp<COMPS>([&](auto ci) {
        constexpr int i = decltype(ci)::value;
        bv[i] = to_word<W>(bp[ro + i * kcstep + ko]);
      });
      each_comp<COMPS>([&](auto ci) {
        constexpr int i = decltype(ci)::value;
#pragma unroll
        for (int v = 0; v < V; v++) in[i][v] = mac_add(ar, in[i][v], ar.mont(x[v], bv[i]));
      });
    }
    if (with_c0) {
#pragma unroll
      for (int v = 0; v < V; v++)
        in[0][v] = mac_add(ar, in[0][v], ar.mont(to_word<W>(zp[v][src]), E.pq));
    }
    if constexpr (WEIGHTED) {
      const W w = to_word<W>(wp[(size_t)r * kstep]);
      each_comp<COMPS>([&](auto ci) {
        constexpr int i = decltype(ci)::value;
#pragma unroll
        for (int v = 0; v < V; v++) out[i][v] = mac_add(ar, out[i][v], ar.mont(in[i][v], w));
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

// k_ctmul_relin with key_hat viewed.  Grid and the addresses of up_hat, x_hat, y_hat and c_hat:
// k_ctmul_relin's.  (i, t) of key_hat starts at word (i top_terms + t) top_limbs n + kl n.
template <class A, class IO>
__global__ __launch_bounds__(256) void k_level_relin(
    const BconvTo<typename A::word> *__restrict__ to,
    const CtLimb<typename A::word> *__restrict__ lc, const IO *__restrict__ uh,
    const IO *__restrict__ kh, const IO *xh, const IO *yh, IO *__restrict__ c, size_t batch,
    uint32_t pairs, uint32_t terms, uint32_t L, uint32_t limbs, uint32_t top_limbs,
    uint32_t top_terms, uint32_t logn) {
  using W = typename A::word;
  constexpr int V = (int)kCtSlices;
  const uint32_t l = blockIdx.y;
  const uint32_t kl = view_limb(l, L, limbs, top_limbs);
  const BconvTo<W> C = to[l];
  const A ar = ks_arith<A>(C);
  const uint32_t lgs = logn - 8;
  const uint32_t g = blockIdx.x >> lgs, s = blockIdx.x & ((1u << lgs) - 1);
  const uint32_t j = (s << 8) + threadIdx.x;
  const size_t step = (size_t)limbs << logn;
  const size_t kstep = (size_t)top_limbs << logn, kcstep = kstep * top_terms;
  const bool tensor = l < L;  // (block-uniform)
  bool live[V];
  size_t p[V];
  const IO *up[V];
#pragma unroll
  for (int v = 0; v < V; v++) {
    const size_t e = (size_t)g * V + v;
    live[v] = e < batch;
    p[v] = live[v] ? e : 0;
    up[v] = uh + ((p[v] * terms * limbs + l) << logn) + j;
  }
  const IO *kp = kh + ((size_t)kl << logn) + j;
  W acc[2][V];
#pragma unroll
  for (int v = 0; v < V; v++) acc[0][v] = acc[1][v] = 0;
  for (uint32_t t = 0; t < terms; t++) {
    const size_t o = (size_t)t * step, ko = (size_t)t * kstep;
    W u[V];
#pragma unroll
    for (int v = 0; v < V; v++) u[v] = to_word<W>(up[v][o]);
    const W k0 = to_word<W>(kp[ko]), k1 = to_word<W>(kp[kcstep + ko]);
#pragma unroll
    for (int v = 0; v < V; v++) {
      acc[0][v] = mac_add(ar, acc[0][v], ar.mont(u[v], k0));
      acc[1][v] = mac_add(ar, acc[1][v], ar.mont(u[v], k1));
    }
  }
  if (tensor) {
    const W pr = lc[l].pr;
    const size_t half = (size_t)L << logn;  // a component of a pair
    W e0[V], e1[V];
    size_t xo[V];
#pragma unroll
    for (int v = 0; v < V; v++) {
      e0[v] = e1[v] = 0;
      xo[v] = ((p[v] * pairs * 2 * L + l) << logn) + j;
    }
    for (uint32_t q = 0; q < pairs; q++) {
      const size_t o = (size_t)q * 2 * half;
      W x0[V], x1[V], y0[V], y1[V];
#pragma unroll
      for (int v = 0; v < V; v++) {
        x0[v] = to_word<W>(xh[xo[v] + o]);
        x1[v] = to_word<W>(xh[xo[v] + o + half]);
        y0[v] = to_word<W>(yh[xo[v] + o]);
        y1[v] = to_word<W>(yh[xo[v] + o + half]);
      }
#pragma unroll
      for (int v = 0; v < V; v++) {
        e0[v] = mac_add(ar, e0[v], ar.mont(x0[v], y0[v]));
        e1[v] = mac_add(ar, e1[v], ar.mont(x0[v], y1[v]));
        e1[v] = mac_add(ar, e1[v], ar.mont(x1[v], y0[v]));
      }
    }
#pragma unroll
    for (int v = 0; v < V; v++) {
      acc[0][v] = mac_add(ar, acc[0][v], ar.mont(e0[v], pr));
      acc[1][v] = mac_add(ar, acc[1][v], ar.mont(e1[v], pr));
    }
  }
#pragma unroll
  for (int v = 0; v < V; v++) {
    if (!live[v]) continue;
    IO *cp = c + ((p[v] * 2 * limbs + l) << logn) + j;
    cp[0] = (IO)BconvArith<W>::mulc(acc[0][v], C.v, C.vs, C.c);  // acc R mod m
    cp[step] = (IO)BconvArith<W>::mulc(acc[1][v], C.v, C.vs, C.c);
  }
}

// NTTMUL_FLAG_VALIDATE on a viewed operand: selected word i is slot i mod n of limb
// m = (i / n) mod limbs of term (i / (limbs n)) mod terms of outer index i / (terms limbs n); it
// lies at o ostride + t kstep + top(m) n + j and is held to q[m].  A diagonal set: terms = 1 and
// ostride = kstep.  Threads past `total` return; no word outside the view is read.
template <class T>
__global__ void k_level_check_range(const T *__restrict__ a, const uint64_t *__restrict__ q,
                                    size_t total, uint32_t logn, uint32_t L, uint32_t limbs,
                                    uint32_t top_limbs, uint32_t terms, size_t ostride, int *bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint32_t j = (uint32_t)(i & (((size_t)1 << logn) - 1));
  size_t r = i >> logn;
  const uint32_t m = (uint32_t)(r % limbs);
  r /= limbs;
  const uint32_t t = (uint32_t)(r % terms);
  const size_t o = r / terms;
  const size_t kstep = (size_t)top_limbs << logn;
  const size_t w = o * ostride + t * kstep + ((size_t)view_limb(m, L, limbs, top_limbs) << logn) + j;
  if ((uint64_t)a[w] >= q[m]) atomicOr(bad, 1);
}

}  // namespace nttmul
