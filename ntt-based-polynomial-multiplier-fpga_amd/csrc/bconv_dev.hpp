// bconv_dev.hpp — the kernel of include/nttmul_bconv.h (lib/libnttmul_bconv.so only): RNS base
// conversion from B = (b_0 .. b_{L-1}) to C = (c_0 .. c_{K-1}), and ModDown with the subtraction
// and the product by B^-1 as its epilogue.  Device code; its launchers are in bconv.hip.  It uses
// Arith32P::pmul, Arith64::shoup / csub / mulhi64 (modarith.hpp) and the stream loads and stores
// of kernels_dev.hpp unchanged and adds no function to them.
//
// The kernel is element-wise in (polynomial, coefficient): no LDS, no twiddles.  A workgroup of
// 256 threads takes kV slices of 256 consecutive coefficients (a slice lies in one polynomial,
// n >= 256), thread t coefficient t of each, so every load and store is one word per lane,
// contiguous over the wave.  Per coefficient and tile of kBconvTile target limbs:
//
//   for i < L:   y_i = x_i (Bh_i^-1 mod b_i) mod b_i                      canonical
//                acc_t += y_i (Bh_i R mod c_{j0+t})    for t < tile       integer sum
//   out_{j0+t} = acc_t R^-1 mod c_{j0+t}                                  canonical
//   (moddown)    out_{j0+t} = (x_{j0+t} - out_{j0+t} + c) (B^-1 mod c) mod c
//
// The tiles are an outer loop of the thread, and y_i is recomputed per tile: neither L values of y
// nor K accumulators fit in registers for L, K up to 64.  The source words are re-read once per
// tile by the same workgroup (ordinary loads; the output and moddown's x_j are touched once and go
// non-temporal; x_j is requested at the tile's start, so its latency passes under the sums).
//
// Every constant index is a loop counter (i, j0 + t), so the compiler knows it wave-uniform and
// reads BconvFrom / BconvTo / the weights with scalar loads into SGPRs, as k_rns_* reads its
// KParams; a per-lane limb index would put every constant in VGPRs.
//
// The accumulator's range contract, per word class (P = one product y_i w, F = the accumulator
// after a fold hi (R mod c) + lo, A = before the next fold; c32 / c64 = R mod c <= c - 1):
//
//   32-bit  y <= b - 1, w <= c - 1, b, c <= 2^31 - 1:  P <= (2^31 - 2)^2 = 2^62 - 2^33 + 4.
//           64-bit accumulator.  F <= (2^32 - 1)(c - 1) + 2^32 - 1 = (2^32 - 1) c < 2^63 - 2^31.
//           A <= F + 2 P < 2^63 + 2^63 - 2^34 + 8 < 2^64: a fold after every 2 products.  (Four
//           products fit an empty accumulator, but a folded one is not empty: F can exceed two
//           products, so the steady cadence is 2.)
//           End: the accumulator is folded, m = lo(F) (-c^-1) mod 2^32, F + m c <= 2 (2^32 - 1) c
//           < 2^64 and (F + m c) / 2^32 < 2c: one Montgomery reduction, one conditional subtraction.
//   64-bit  y <= b - 1, w <= c - 1, b, c <= 2^62 - 1, both split into 31-bit limbs (Arith64::basemul's
//           form): y = yh 2^31 + yl, w = wh 2^31 + wl, every limb <= 2^31 - 1.  Four 64-bit sums
//           ll, lh, hl, hh of limb products <= (2^31 - 1)^2 < 2^62 take one v_mad_u64_u32 each per
//           product and hold 4 products (4 (2^31 - 1)^2 < 2^64): a fold after every 4 products.
//           The fold assembles S = ll + (lh + hl) 2^31 + hh 2^62 = the sum of the 4 products
//           < 4 2^124 = 2^126 in 128 bits, adds the running value F <= (2^64 - 1) c < 2^126
//           (F + S < 2^127) and folds: F' = hi64 (2^64 mod c) + lo64 <= (2^64 - 1) c again.
//           End: F + m c <= 2 (2^64 - 1) c < 2^127 and the quotient is below 2c, as above.
//           (The first form summed whole 128-bit products, about 14 instructions each; here a
//           product is 4 and the fold about 34 per four products: DESIGN.md section 4.)
//
// Small moduli only make every bound smaller; nothing above needs c or b near the top of its class.
#pragma once
#include "bconv.hpp"
#include "kernels_dev.hpp"

namespace nttmul {

template <class W>
struct BconvArith;

template <>
struct BconvArith<uint32_t> {
  using Acc = uint64_t;
  static constexpr int kV = 4;        // slices per workgroup
  static constexpr int kCadence = 2;  // products between folds
  // x k mod q in [0, q) for any 32-bit x; (v, vs) the Plantard pair of k
  __device__ __forceinline__ static uint32_t mulc(uint32_t x, uint32_t v, uint32_t vs, uint32_t q) {
    return Arith32P{q, 0, 0, 0}.pmul(x, v, vs);
  }
  __device__ __forceinline__ static Acc zero() { return 0; }
  __device__ __forceinline__ static void mac(Acc &acc, uint32_t y, uint32_t w) {
    acc += (uint64_t)y * w;
  }
  __device__ __forceinline__ static void fold(Acc &acc, uint32_t cr) {
    acc = (uint64_t)(uint32_t)(acc >> 32) * cr + (uint32_t)acc;
  }
  // folded accumulator -> acc 2^-32 mod c in [0, c)
  __device__ __forceinline__ static uint32_t reduce(Acc f, const BconvTo<uint32_t> &C) {
    const uint32_t m = (uint32_t)f * C.qinv_neg;
    return Arith32P::csub((uint32_t)((f + (uint64_t)m * C.c) >> 32), C.c);
  }
};

template <>
struct BconvArith<uint64_t> {
  struct Acc {
    uint64_t ll, lh, hl, hh;  // sums of 31-bit limb products since the last fold
    unsigned __int128 f;      // the folded value of everything before
  };
  static constexpr int kV = 1;
  static constexpr int kCadence = 4;
  // x k mod q in [0, q) for any 64-bit x; (v, vs) the Shoup pair of k
  __device__ __forceinline__ static uint64_t mulc(uint64_t x, uint64_t v, uint64_t vs, uint64_t q) {
    return Arith64::csub(Arith64{q, 0, 0}.shoup<false>(x, v, vs), q);
  }
  __device__ __forceinline__ static Acc zero() { return Acc{0, 0, 0, 0, 0}; }
  __device__ __forceinline__ static void mac(Acc &acc, uint64_t y, uint64_t w) {
    const uint32_t yl = (uint32_t)y & 0x7FFFFFFFu, yh = (uint32_t)(y >> 31);
    const uint32_t wl = (uint32_t)w & 0x7FFFFFFFu, wh = (uint32_t)(w >> 31);
    acc.ll += (uint64_t)yl * wl;
    acc.lh += (uint64_t)yl * wh;
    acc.hl += (uint64_t)yh * wl;
    acc.hh += (uint64_t)yh * wh;
  }
  __device__ __forceinline__ static void fold(Acc &acc, uint64_t cr) {
    const unsigned __int128 s = acc.f + acc.ll + (((unsigned __int128)acc.lh + acc.hl) << 31) +
                                ((unsigned __int128)acc.hh << 62);
    acc.f = (unsigned __int128)(uint64_t)(s >> 64) * cr + (uint64_t)s;
    acc.ll = acc.lh = acc.hl = acc.hh = 0;
  }
  // folded accumulator -> acc 2^-64 mod c in [0, c)
  __device__ __forceinline__ static uint64_t reduce(const Acc &acc, const BconvTo<uint64_t> &C) {
    const uint64_t lo = (uint64_t)acc.f, hi = (uint64_t)(acc.f >> 64);
    const uint64_t m = lo * C.qinv_neg;
    // lo + lo64(m c) = 0 mod 2^64: its carry is (lo != 0)
    return Arith64::csub(hi + Arith64::mulhi64(m, C.c) + (lo != 0 ? 1 : 0), C.c);
  }
};

// OP kBconvConvert: in [batch][L][n] -> out [batch][K][n].  OP kBconvModdown: in [batch][K + L][n]
// (limbs c_0 .. c_{K-1}, then b_0 .. b_{L-1}) -> out [batch][K][n].  slices = batch n / 256.
// to and wt are padded to bconv_pad(K) target limbs (bconv.hpp).  Slices past the end read slice 0
// (always valid) instead of branching per load; their results are never stored.
template <class W, int OP>
__global__ __launch_bounds__(256) void k_bconv(const BconvFrom<W> *__restrict__ from,
                                               const BconvTo<W> *__restrict__ to,
                                               const W *__restrict__ wt, const W *__restrict__ in,
                                               W *__restrict__ out, size_t slices, uint32_t logn,
                                               uint32_t L, uint32_t K) {
  using Ar = BconvArith<W>;
  using Acc = typename Ar::Acc;
  constexpr int V = Ar::kV, T = (int)kBconvTile, CAD = Ar::kCadence;
  const uint32_t kpad = bconv_pad(K);
  const uint32_t in_limbs = OP == kBconvModdown ? K + L : L, in_first = OP == kBconvModdown ? K : 0;
  const uint32_t lgs = logn - 8;  // slices per polynomial = 2^lgs
  bool live[V];
  const W *src[V];                // limb 0 of the slice's polynomial in `in`, this thread's word
  W *dst[V];
#pragma unroll
  for (int v = 0; v < V; v++) {
    const size_t s = (size_t)blockIdx.x * V + v;
    live[v] = s < slices;
    const size_t sl = live[v] ? s : 0;
    const size_t p = sl >> lgs, k = ((sl & (((size_t)1 << lgs) - 1)) << 8) + threadIdx.x;
    src[v] = in + ((p * in_limbs) << logn) + k;
    dst[v] = out + ((p * K) << logn) + k;
  }
  for (uint32_t j0 = 0; j0 < K; j0 += T) {
    Acc acc[V][T];
    W cr[T], xj[V][T];
#pragma unroll
    for (int t = 0; t < T; t++) {
      cr[t] = to[j0 + t].cr;
      // moddown's x_j, requested before the sums so that its latency passes under them (a padded
      // target limb reads the last real one)
      const uint32_t jx = j0 + t < K ? j0 + t : K - 1;
#pragma unroll
      for (int v = 0; v < V; v++) {
        acc[v][t] = Ar::zero();
        if (OP == kBconvModdown) xj[v][t] = ld_stream<true>(src[v] + ((size_t)jx << logn));
      }
    }
    const auto step = [&](uint32_t i) {
      const BconvFrom<W> F = from[i];
      W y[V];
#pragma unroll
      for (int v = 0; v < V; v++)
        y[v] = Ar::mulc(src[v][(size_t)(in_first + i) << logn], F.v, F.vs, F.b);
#pragma unroll
      for (int t = 0; t < T; t++) {
        const W w = wt[(size_t)i * kpad + j0 + t];
#pragma unroll
        for (int v = 0; v < V; v++) Ar::mac(acc[v][t], y[v], w);
      }
    };
    const auto fold = [&] {
#pragma unroll
      for (int t = 0; t < T; t++)
#pragma unroll
        for (int v = 0; v < V; v++) Ar::fold(acc[v][t], cr[t]);
    };
    // CAD products, a fold; the last group may be shorter and is folded as well, so reduce always
    // reads a folded accumulator
    uint32_t i = 0;
    for (; i + CAD <= L; i += CAD) {
#pragma unroll
      for (int c = 0; c < CAD; c++) step(i + c);
      fold();
    }
    if (i < L) {
      for (; i < L; i++) step(i);
      fold();
    }
#pragma unroll
    for (int t = 0; t < T; t++) {
      const uint32_t j = j0 + t;
      if (j >= K) break;
      const BconvTo<W> C = to[j];
#pragma unroll
      for (int v = 0; v < V; v++) {
        if (!live[v]) continue;
        W r = Ar::reduce(acc[v][t], C);
        if (OP == kBconvModdown)
          r = Ar::mulc(xj[v][t] - r + C.c, C.v, C.vs, C.c);  // x - r + c in (0, 2c)
        st_stream<true>(dst[v] + ((size_t)j << logn), r);
      }
    }
  }
}

}  // namespace nttmul
