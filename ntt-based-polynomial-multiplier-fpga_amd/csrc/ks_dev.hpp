// ks_dev.hpp — the kernel of include/nttmul_ks.h (lib/libnttmul_ks.so only): digit ModUp, the
// base conversion of every digit D_d of Q to all M = L + K limbs of Q u P in one launch, written
// in nttmul_*_mac_ntt's operand layout [batch][dnum][M][n].  Device code; its launcher is in
// ks.hip.  It uses BconvArith<W> (bconv_dev.hpp: mulc, mac, fold, reduce, the fold cadences and the
// accumulator's range contract, which a digit of at most 64 limbs meets as any `from` basis does)
// and the stream stores of kernels_dev.hpp unchanged and adds no function to them.
//
// Element-wise in (polynomial, digit, coefficient) like k_bconv.  The grid is (workgroups, dnum):
// a workgroup of 256 threads takes kV slices of 256 consecutive coefficients (a slice lies in one
// polynomial, n >= 256) for the digit d = blockIdx.y, thread t coefficient t of each.  Per
// coefficient and tile of kBconvTile target limbs of the extended basis:
//
//   for i in D_d:  y_i = x_i (Dh_i^-1 mod q_i) mod q_i                       canonical
//                  acc_t += y_i (Dh_i R mod m_{j0+t})     for t < tile       integer sum
//   out_{d, j0+t} = acc_t R^-1 mod m_{j0+t}                                   canonical
//
// The digit's own limbs are computed by the same formula: Dh_i = 0 mod q_m for every other limb m
// of the digit, so the sum is y_m Dh_m = x_m mod q_m, bit for bit for a canonical x_m.  No target
// limb is a special case and no branch depends on it.
//
// Only the digit's |D_d| source limbs are read, once per tile by the same workgroup (ordinary
// loads: the re-reads come from L2); the output is touched once and goes non-temporal.
//
// Every constant index is a loop counter or a block index (i, j0 + t, d), so the compiler knows
// it wave-uniform and reads BconvFrom / BconvTo / the weights with scalar loads into SGPRs; a
// per-lane limb or digit index would put every constant in VGPRs.
#pragma once
#include "bconv_dev.hpp"
#include "ks.hpp"

namespace nttmul {

// in [batch][L][n] -> out [batch][dnum][M][n], M = L + K, dnum = gridDim.y = ceil(L / alpha).
// slices = batch n / 256.  to and wt are padded to bconv_pad(M) target limbs (bconv.hpp).  Slices
// past the end read slice 0 (always valid) instead of branching per load; their results are never
// stored.  Polynomial and digit offsets are 64-bit: batch dnum M n may pass 2^32 words.
template <class W>
__global__ __launch_bounds__(256) void k_ks_modup(const BconvFrom<W> *__restrict__ from,
                                                  const BconvTo<W> *__restrict__ to,
                                                  const W *__restrict__ wt,
                                                  const W *__restrict__ in, W *__restrict__ out,
                                                  size_t slices, uint32_t logn, uint32_t L,
                                                  uint32_t M, uint32_t alpha) {
  using Ar = BconvArith<W>;
  using Acc = typename Ar::Acc;
  constexpr int V = Ar::kV, T = (int)kBconvTile, CAD = Ar::kCadence;
  const uint32_t mpad = bconv_pad(M);
  const uint32_t d = blockIdx.y, dnum = gridDim.y;
  const uint32_t i0 = d * alpha, i1 = i0 + alpha < L ? i0 + alpha : L;  // the digit's limbs
  const uint32_t lgs = logn - 8;  // slices per polynomial = 2^lgs
  bool live[V];
  const W *src[V];                // limb 0 of the slice's polynomial in `in`, this thread's word
  W *dst[V];                      // limb 0 of digit d of that polynomial in `out`
#pragma unroll
  for (int v = 0; v < V; v++) {
    const size_t s = (size_t)blockIdx.x * V + v;
    live[v] = s < slices;
    const size_t sl = live[v] ? s : 0;
    const size_t p = sl >> lgs, k = ((sl & (((size_t)1 << lgs) - 1)) << 8) + threadIdx.x;
    src[v] = in + ((p * L) << logn) + k;
    dst[v] = out + (((p * dnum + d) * M) << logn) + k;
  }
  for (uint32_t j0 = 0; j0 < M; j0 += T) {
    Acc acc[V][T];
    W cr[T];
#pragma unroll
    for (int t = 0; t < T; t++) {
      cr[t] = to[j0 + t].cr;
#pragma unroll
      for (int v = 0; v < V; v++) acc[v][t] = Ar::zero();
    }
    const auto step = [&](uint32_t i) {
      const BconvFrom<W> F = from[i];
      W y[V];
#pragma unroll
      for (int v = 0; v < V; v++) y[v] = Ar::mulc(src[v][(size_t)i << logn], F.v, F.vs, F.b);
#pragma unroll
      for (int t = 0; t < T; t++) {
        const W w = wt[(size_t)i * mpad + j0 + t];
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
    uint32_t i = i0;
    for (; i + CAD <= i1; i += CAD) {
#pragma unroll
      for (int c = 0; c < CAD; c++) step(i + c);
      fold();
    }
    if (i < i1) {
      for (; i < i1; i++) step(i);
      fold();
    }
#pragma unroll
    for (int t = 0; t < T; t++) {
      const uint32_t j = j0 + t;
      if (j >= M) break;
      const BconvTo<W> C = to[j];
#pragma unroll
      for (int v = 0; v < V; v++) {
        if (!live[v]) continue;
        st_stream<true>(dst[v] + ((size_t)j << logn), Ar::reduce(acc[v][t], C));
      }
    }
  }
}

}  // namespace nttmul
