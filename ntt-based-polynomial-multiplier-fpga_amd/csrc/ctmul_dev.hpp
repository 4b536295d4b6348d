// ctmul_dev.hpp — the kernels of include/nttmul_ctmul.h (lib/libnttmul_ctmul.so only): the tensor
// product of two ciphertexts and its relinearisation, formed in Q u P before ModDown.  Device code;
// the launchers are in ctmul.hip.  It reuses mont (modarith.hpp), mac_add (mac_dev.hpp),
// BconvArith<W>::mulc (bconv_dev.hpp) and ks_arith (ksntt_dev.hpp) unchanged, inside their stated
// domains, and adds no function to them.
//
//   high   d2_hat[p][l][j] = (sum_s x_hat[p][s][1][l][j] y_hat[p][s][1][l][j]) mod q_l
//   relin  c_hat[p][i][l][j] = (sum_t up_hat[p][t][l][j] key_hat[i][t][l][j]
//                               + [l < L] (P mod q_l) e_i[p][l][j]) mod m_l
//          e_0 = sum_s x[s][0] y[s][0],  e_1 = sum_s (x[s][0] y[s][1] + x[s][1] y[s][0])
//
// Both are element-wise, one launch at every n: no transform, no twiddle, no LDS, no barrier, no
// index table, no gather.  x_hat and y_hat may be the same memory (the square) and are only read.
//
// k_ctmul_relin: k_lintrans's batch-sliced form (lintrans_dev.hpp) without the rotation loop.  256
// threads, one slot per lane; the V = kCtSlices slices of a workgroup are the same 256 slots of V
// consecutive batch entries, so every word of key_hat is loaded once and used V times (V is
// ctmul_plan.hpp's ctmul_slices of the class: 4 for both in the library, 2 on 64-bit words in the
// A/B build of Makefile ab-ctmul, which DESIGN.md section 4 records and does not keep).  Grid
// (runs n / 256, M), blockIdx.x = g (n / 256) + s with s the range of 256 slots (the faster
// index) and g the run of V entries; every access of a wave is one word per lane and contiguous.
// A lane keeps 2 x V accumulators over the terms, acc = mac_add(acc, mont(up, key)).  On the limbs
// l < L (blockIdx.y, block-uniform) it then forms e_0 and e_1 for its V entries over the pairs
// (four loads, three mont and three mac_add per pair and entry) and adds
// acc_i = mac_add(acc_i, mont(e_i, P R mod q_l)): e_i carries R^-1, the product with P R carries
// R^-1 again, the power the key sum carries, so every addend of an output word has the same scale
// and one mulc by R mod m per output word takes it out, as in k_ksntt_mac.  The limbs of P skip
// the tensor terms.  Slices past the end read entry 0, always valid, instead of branching per
// load, and never store.
//
// k_ctmul_high: a pure stream, nothing shared and nothing gathered.  A lane takes one vector of
// 16 bytes (4 words of 32 bits, 2 of 64) of one limb's stream [batch][n] per operand and pair: one
// 128-bit access where the caller's address allows it, declared with the word's alignment only
// (CtVec), since that is all the contract gives.  Grid (ceil(batch n / vec / 256), L).  A
// workgroup takes 256 consecutive vectors, which at n <= 512 (32-bit) or n = 256 (64-bit) are
// several whole polynomials; lanes past the last vector return at once (no barrier follows).
// acc = mac_add(acc, mont(x, y)) over the pairs, then mulc by R mod q_l.
//
// Range contract, per arithmetic class (u = a word of up_hat, x_hat or y_hat, k = a word of
// key_hat or y_hat, all canonical by the call's contract; acc, e = accumulators):
//   Arith32P  m = mont(u, k) in [0, q) (mont reduces its first operand from [0, 2q), the second
//             may be any word below 2q); acc = mac_add(acc, m) stays canonical (acc + m < 2q <
//             2^32), and so does e.  mont(e, P R mod q): e canonical is inside mont's [0, 2q),
//             the constant is canonical; the product is in [0, q) and acc stays canonical.  The
//             one step per output word is mulc(acc, R mod m) (Plantard, any 32-bit input):
//             canonical.
//   Arith64   m in [0, 2q); acc and e stay in [0, 2q) (acc + m < 4q < 2^64, one conditional
//             subtraction of 2q).  mont(e, P R mod q): mont takes lazy words below 4q and
//             canonicalises both; the product is in [0, 2q) and acc stays in [0, 2q).  mulc
//             (Shoup takes any 64-bit word, one conditional subtraction): canonical.
//   The sums run over terms + 1 and over pairs or 2 pairs addends; no bound on terms or pairs is
//   needed, every addition is followed by its conditional subtraction.
// Polynomial offsets are 64-bit, slots 32-bit.
#pragma once
#include "ctmul.hpp"
#include "ksntt_dev.hpp"

namespace nttmul {

// Grid (ctmul_plan.hpp ctmul_relin_grid wgx, M); groups = ceil(batch / V).  (p, t) of up_hat
// starts at word ((p terms + t) M + l) n, (i, t) of key_hat at ((i terms + t) M + l) n, (p, s, i)
// of x_hat and y_hat at (((p pairs + s) 2 + i) L + l) n, (p, i) of c_hat at ((p 2 + i) M + l) n,
// all in 64 bits.  to: BconvTo<W>[..] over Q u P whose (v, vs) is the pair of R mod m;
// lc: CtLimb<W>[L].
template <class A, class IO>
__global__ __launch_bounds__(256) void k_ctmul_relin(
    const BconvTo<typename A::word> *__restrict__ to,
    const CtLimb<typename A::word> *__restrict__ lc, const IO *__restrict__ uh,
    const IO *__restrict__ kh, const IO *xh, const IO *yh, IO *__restrict__ c, size_t batch,
    uint32_t pairs, uint32_t terms, uint32_t L, uint32_t limbs, uint32_t logn) {
  using W = typename A::word;
  constexpr int V = (int)ctmul_slices(8 * (int)sizeof(W));
  const uint32_t l = blockIdx.y;
  const BconvTo<W> C = to[l];
  const A ar = ks_arith<A>(C);
  const uint32_t lgs = logn - 8;
  const uint32_t g = blockIdx.x >> lgs, s = blockIdx.x & ((1u << lgs) - 1);
  const uint32_t j = (s << 8) + threadIdx.x;
  const size_t step = (size_t)limbs << logn, cstep = step * terms;
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
  const IO *kp = kh + ((size_t)l << logn) + j;
  W acc[2][V];
#pragma unroll
  for (int v = 0; v < V; v++) acc[0][v] = acc[1][v] = 0;
  for (uint32_t t = 0; t < terms; t++) {
    const size_t o = (size_t)t * step;
    W u[V];
#pragma unroll
    for (int v = 0; v < V; v++) u[v] = to_word<W>(up[v][o]);
    const W k0 = to_word<W>(kp[o]), k1 = to_word<W>(kp[cstep + o]);
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

// 16 bytes of consecutive words with the alignment of one: the compiler may use one 128-bit access
// (the target allows unaligned global accesses) and must not assume more than the word's alignment
template <class IO>
struct alignas(sizeof(IO)) CtVec {
  IO w[16 / sizeof(IO)];
};

// Grid (ctmul_plan.hpp ctmul_high_grid wgx, L); vectors = batch n / VEC.  Vector g of limb l is
// words [j, j + VEC) of polynomial p = g / (n / VEC), j = (g mod (n / VEC)) VEC: (p, s, 1) of
// x_hat and y_hat starts at word (((p pairs + s) 2 + 1) L + l) n, p of d2_hat at (p L + l) n, all
// in 64 bits.  to: the first L entries of the context's BconvTo<W> table.
template <class A, class IO>
__global__ __launch_bounds__(256) void k_ctmul_high(
    const BconvTo<typename A::word> *__restrict__ to, const IO *xh, const IO *yh,
    IO *__restrict__ d2, size_t vectors, uint32_t pairs, uint32_t L, uint32_t logn) {
  using W = typename A::word;
  constexpr int VEC = 16 / sizeof(IO);
  constexpr uint32_t LGV = VEC == 4 ? 2 : 1;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= vectors) return;
  const uint32_t l = blockIdx.y;
  const BconvTo<W> C = to[l];
  const A ar = ks_arith<A>(C);
  const uint32_t lgp = logn - LGV;  // vectors of a polynomial
  const size_t p = g >> lgp;
  const uint32_t j = (uint32_t)(g & (((size_t)1 << lgp) - 1)) << LGV;
  const size_t half = (size_t)L << logn;
  const size_t xo = (((p * pairs * 2 + 1) * L + l) << logn) + j;
  W acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; k++) acc[k] = 0;
  for (uint32_t q = 0; q < pairs; q++) {
    const size_t o = xo + (size_t)q * 2 * half;
    const CtVec<IO> x = *(const CtVec<IO> *)(xh + o), y = *(const CtVec<IO> *)(yh + o);
#pragma unroll
    for (int k = 0; k < VEC; k++)
      acc[k] = mac_add(ar, acc[k], ar.mont(to_word<W>(x.w[k]), to_word<W>(y.w[k])));
  }
  CtVec<IO> out;
#pragma unroll
  for (int k = 0; k < VEC; k++) out.w[k] = (IO)BconvArith<W>::mulc(acc[k], C.v, C.vs, C.c);
  *(CtVec<IO> *)(d2 + ((p * L + l) << logn) + j) = out;
}

}  // namespace nttmul
