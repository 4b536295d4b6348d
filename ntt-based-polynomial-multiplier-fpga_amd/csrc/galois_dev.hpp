// galois_dev.hpp — the kernels of include/nttmul_galois.h (lib/libnttmul_galois.so only): the
// automorphism sigma_k : a(x) -> a(x^k) mod (x^n + 1) over [batch][limbs][n] operands, in
// coefficient order and in the bit-reversed order of the forward transforms.  Device code; its
// launchers are in galois.hip.  It uses the stream loads and stores of kernels_dev.hpp unchanged
// and adds no function to them.
//
// Pure data movement: no twiddles, no index table (a table would double the traffic), one word per
// lane and access, so an operand needs the alignment of its word only.  The limb is blockIdx.y; a
// polynomial's base offset is 64-bit, every index inside it 32-bit: 2n is a power of two, so
// k (2 r + 1) and j k^-1 may wrap 32 bits before the mask without changing the result.
//
//   NTT order      slot j holds a(psi^(2 brv(j) + 1)).  sigma_k(a) at that point is a at the
//                  exponent k (2 brv(j) + 1) mod 2n, so  out[j] = in[src_k(j)],
//                  src_k(j) = brv(((k (2 brv(j) + 1)) mod 2n - 1) / 2).
//                  In natural order this is r -> (k r + (k - 1) / 2) mod n, whose low t bits
//                  depend on the low t bits of r alone.  Bit-reversed, the high bits of j decide
//                  the high bits of src_k(j): an aligned block of 2^m consecutive slots maps onto
//                  one aligned block of 2^m slots.  A wave that stores 64
//                  consecutive slots therefore loads from one aligned 64-word segment (256 or 512
//                  bytes: the cache lines a contiguous load would touch); k_galois_ntt_many
//                  loads 64 consecutive slots once and stores them into one aligned segment per
//                  automorphism (the scatter form: out_c[src_{k_c^-1}(j)] = in[j]).
//   coefficients   out[j] = +-in[i0 mod n], i0 = j k^-1 mod 2n, negated when i0 >= n: a gather at
//                  the odd stride k^-1, with no locality for a general k.  k_galois_coeff stages
//                  the source words in LDS: contiguous loads, LDS reads at an odd word stride (no
//                  bank conflict), contiguous stores.  While a limb polynomial fits the stage
//                  (kGaloisLdsBytes) a workgroup takes it whole (for n < 1024: 1024 / n of them).
//                  Above that it is split in M = 2^LGM residue classes: k^-1 is odd, so the
//                  outputs j = c mod M come from the sources i = c k^-1 mod M, and a workgroup
//                  stages one class, n / M words at stride M, and stores one class at stride M.
//                  A wave's load then spans M times the cache lines of a contiguous one, each
//                  shared with the M - 1 sibling workgroups (M <= 2 on 32-bit words, <= 4 on
//                  64-bit words: 8 and 32 bytes between the words of neighbouring lanes).
//
// The moduli come from the context's table q[limbs], indexed by blockIdx.y: wave-uniform, a scalar
// load into SGPRs, as k_rns_* reads its KParams.
#pragma once
#include "galois.hpp"
#include "kernels_dev.hpp"

namespace nttmul {

// src_k(j) of the header: sh = 32 - logn, mask2 = 2n - 1
__device__ __forceinline__ uint32_t galois_slot(uint32_t j, uint32_t k, uint32_t sh,
                                                uint32_t mask2) {
  const uint32_t r = __brev(j) >> sh;
  const uint32_t e = (k * (2u * r + 1u)) & mask2;  // odd
  return __brev(e >> 1) >> sh;
}

// Slices of 256 consecutive words of one limb polynomial (n >= 256): slice s of limb l is words
// [(s mod 2^lgs) 256, +256) of polynomial s >> lgs, lgs = logn - 8.  A workgroup takes
// kGaloisSlices of them (at n = 256: that many polynomials).
__device__ __forceinline__ size_t galois_base(size_t s, uint32_t lgs, uint32_t logn,
                                              uint32_t limbs, uint32_t l, uint32_t *j0) {
  *j0 = (uint32_t)(s & (((size_t)1 << lgs) - 1)) << 8;
  return (((s >> lgs) * limbs + l) << logn);
}

// Slices this workgroup holds: kGaloisSlices, fewer in the last workgroup of a launch
__device__ __forceinline__ int galois_live(size_t slices) {
  const size_t left = slices - (size_t)blockIdx.x * kGaloisSlices;
  return left >= (size_t)kGaloisSlices ? kGaloisSlices : (int)left;
}

// body(u, s): slice u of the workgroup, slice s of the launch.  A full workgroup runs `load` for
// all its slices and then `store` for all of them, so that a wave has kGaloisSlices loads in
// flight; the partial last workgroup takes its slices one after the other.  The branch is
// workgroup-uniform.
template <class Load, class Store>
__device__ __forceinline__ void galois_slices(size_t slices, Load load, Store store) {
  const size_t s0 = (size_t)blockIdx.x * kGaloisSlices;
  if (galois_live(slices) == kGaloisSlices) {
#pragma unroll
    for (int u = 0; u < kGaloisSlices; u++) load(u, s0 + u);
#pragma unroll
    for (int u = 0; u < kGaloisSlices; u++) store(u);
  } else {
#pragma unroll
    for (int u = 0; u < kGaloisSlices - 1; u++) {
      if (s0 + u >= slices) break;
      load(u, s0 + u);
      store(u);
    }
  }
}

// out[p][l][j] = in[p][l][src_k(j)]
template <class W>
__global__ __launch_bounds__(256) void k_galois_ntt(const W *__restrict__ in, W *__restrict__ out,
                                                    uint32_t k, uint32_t logn, size_t slices,
                                                    uint32_t limbs) {
  const uint32_t sh = 32 - logn, mask2 = (2u << logn) - 1, l = blockIdx.y;
  W v[kGaloisSlices];
  size_t dst[kGaloisSlices];
  galois_slices(
      slices,
      [&](int u, size_t s) {
        uint32_t j0;
        const size_t base = galois_base(s, logn - 8, logn, limbs, l, &j0);
        const uint32_t j = j0 + threadIdx.x;
        dst[u] = base + j;
        v[u] = ld_stream<true>(in + base + galois_slot(j, k, sh, mask2));
      },
      [&](int u) { st_stream<true>(out + dst[u], v[u]); });
}

// out[c][p][l][src_{kinv_c}(j)] = in[p][l][j] for c < count: kinv.k[c] = k_c^-1 mod 2n, so that
// out[c] is sigma_{k_c}.  plane = batch limbs n, the words of one out[c].
template <class W>
__global__ __launch_bounds__(256) void k_galois_ntt_many(const W *__restrict__ in,
                                                         W *__restrict__ out, GaloisKs kinv,
                                                         uint32_t count, uint32_t logn,
                                                         size_t slices, uint32_t limbs,
                                                         size_t plane) {
  const uint32_t sh = 32 - logn, mask2 = (2u << logn) - 1, l = blockIdx.y;
  W v[kGaloisSlices];
  size_t base[kGaloisSlices];
  uint32_t j[kGaloisSlices];
  galois_slices(
      slices,
      [&](int u, size_t s) {
        uint32_t j0;
        base[u] = galois_base(s, logn - 8, logn, limbs, l, &j0);
        j[u] = j0 + threadIdx.x;
        v[u] = ld_stream<true>(in + base[u] + j[u]);
      },
      [&](int u) {
        for (uint32_t c = 0; c < count; c++)  // kinv.k[c]: wave-uniform, the kernel argument
          st_stream<true>(out + (size_t)c * plane + base[u] + galois_slot(j[u], kinv.k[c], sh, mask2),
                          v[u]);
      });
}

// -x mod q for canonical x: q - x, and 0 for 0
template <class W>
__device__ __forceinline__ W galois_neg(W x, W q) {
  return x ? q - x : x;
}

// out[p][l][j] = +-in[p][l][(j kinv) mod n], negated when (j kinv) mod 2n >= n; kinv = k^-1 mod 2n.
// units = polynomials per limb.  M = 2^LGM residue classes per polynomial, n / M words each; the
// block size is a power of two from 256 that divides the words a workgroup stages.
//   LGM = 0   a workgroup stages max(n, kGaloisStage) words: max(1, kGaloisStage / n) whole
//             polynomials of limb l, fewer in the last workgroup.
//   LGM > 0   a workgroup stages class c of one polynomial: the words c' + M t, c' = c kinv mod M,
//             and stores the words c + M t.  Eight polynomials x M classes make a group of 8 M
//             consecutive workgroups, the M classes of a polynomial 8 apart: workgroups are dealt
//             round-robin over the 8 XCDs, so the M workgroups that share every cache line of a
//             polynomial, read and written, run on one L2 at about the same time.  Polynomials
//             past the end (units no multiple of 8) leave at once.
// Both phases move four words per thread at a time, so a wave has four loads in flight.
template <class W, int LGM>
__global__ __launch_bounds__(1024) void k_galois_coeff(
    const uint64_t *__restrict__ q, const W *__restrict__ in, W *__restrict__ out, uint32_t kinv,
    uint32_t logn, size_t units, uint32_t limbs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char galois_lds[];
  W *lds = (W *)galois_lds;
  constexpr uint32_t M = 1u << LGM;
  // a whole polynomial streams; the classes of a split one share every cache line, read and
  // written, with their sibling workgroups, so their accesses stay temporal
  constexpr bool kNT = LGM == 0;
  const uint32_t n = 1u << logn, mask2 = 2 * n - 1, l = blockIdx.y, bd = blockDim.x;
  const W ql = (W)q[l];
  size_t p0;
  uint32_t live, c = 0;  // words this workgroup stages; its class
  if constexpr (LGM == 0) {
    const uint32_t ppw = n >= kGaloisStage ? 1u : kGaloisStage >> logn;
    p0 = (size_t)blockIdx.x * ppw;
    const size_t left = units - p0;
    live = (left >= ppw ? ppw : (uint32_t)left) << logn;
  } else {
    c = (blockIdx.x >> 3) & (M - 1);
    p0 = (((size_t)blockIdx.x >> (3 + LGM)) << 3) + (blockIdx.x & 7);
    if (p0 >= units) return;
    live = n >> LGM;
  }
  const uint32_t cs = (c * kinv) & (M - 1);
  // word i of the stage: polynomial p0 + (i / (n / M)), word cs + M (i mod (n / M)) of it
  const auto src = [&](uint32_t i) {
    const uint32_t t = i & ((n >> LGM) - 1);
    return in + (((p0 + ((i - t) >> (logn - LGM))) * limbs + l) << logn) + cs + (t << LGM);
  };
  uint32_t i = threadIdx.x;
  for (; i + 3 * bd < live; i += 4 * bd) {
    W v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = ld_stream<kNT>(src(i + u * bd));
#pragma unroll
    for (int u = 0; u < 4; u++) lds[i + u * bd] = v[u];
  }
  for (; i < live; i += bd) lds[i] = ld_stream<kNT>(src(i));
  __syncthreads();
  // word i of the output: the same polynomial, word j = c + M (i mod (n / M)); its source is word
  // i0 mod n of the polynomial, which is in this class: word (i0 mod n) / M of the stage
  const auto move = [&](uint32_t i, W *x, W **dst) {
    const uint32_t t = i & ((n >> LGM) - 1), j = c + (t << LGM), i0 = (j * kinv) & mask2;
    const W v = lds[(i - t) + ((i0 & (n - 1)) >> LGM)];
    *x = i0 >= n ? galois_neg(v, ql) : v;
    *dst = out + (((p0 + ((i - t) >> (logn - LGM))) * limbs + l) << logn) + j;
  };
  i = threadIdx.x;
  for (; i + 3 * bd < live; i += 4 * bd) {
    W v[4], *dst[4];
#pragma unroll
    for (int u = 0; u < 4; u++) move(i + u * bd, &v[u], &dst[u]);
#pragma unroll
    for (int u = 0; u < 4; u++) st_stream<kNT>(dst[u], v[u]);
  }
  for (; i < live; i += bd) {
    W v, *dst;
    move(i, &v, &dst);
    st_stream<kNT>(dst, v);
  }
}

}  // namespace nttmul
