// bconv.hpp — internal interface between the host entry points of include/nttmul_bconv.h
// (bconv.cpp) and the launchers of bconv.hip.  lib/libnttmul_bconv.so only.
#pragma once
#include <vector>

#include "launch.hpp"

namespace nttmul {

enum BconvOp { kBconvConvert = 0, kBconvModdown = 1 };

// Target limbs per thread and pass of k_bconv (bconv_dev.hpp).  The device tables indexed by a
// target limb are padded to a multiple of it, so the kernel computes whole tiles and guards only
// its stores.
constexpr uint32_t kBconvTile = 4;
constexpr uint32_t bconv_pad(uint32_t to_limbs) {
  return (to_limbs + kBconvTile - 1) / kBconvTile * kBconvTile;
}

// Constants of one `from` limb: the modulus b_i and Bh_i^-1 mod b_i as the (value, companion)
// pair the word class multiplies by (32-bit words: the Plantard pair, low and high word; 64-bit
// words: Shoup).
template <class W>
struct BconvFrom {
  W b, v, vs;
};
// Constants of one `to` limb: the modulus c_j, -c_j^-1 mod R and R mod c_j (R = 2^32 or 2^64: the
// accumulator's fold and its Montgomery reduction), and B^-1 mod c_j as a (value, companion) pair.
template <class W>
struct BconvTo {
  W c, qinv_neg, cr, v, vs;
};

// The host side of the table format (bconv.cpp; ks.cpp builds its ModUp and ModDown tables with
// the same functions).
// (value, companion) pair the device multiplies by k with (bconv_dev.hpp mulc): the Plantard pair
// of Arith32P::pmul, BR = B q^-1 mod 2^64 with B = -k 2^64 mod q as (low, high) word, or Shoup
template <class W>
void mul_pair(uint64_t k, uint64_t q, W *v, W *vs);
// -q^-1 mod 2^64 (the low word serves 32-bit words)
uint64_t neg_inv(uint64_t q);
// The three device tables of a conversion for words of word_bits, in host memory: `from` limbs b
// with the factors inv [|b|], `to` limbs c with the epilogue factors binv [|c|] and the weights
// w [|b|][|c|]
void build_tables(int word_bits, const std::vector<uint64_t> &b, const std::vector<uint64_t> &inv,
                  const std::vector<uint64_t> &c, const std::vector<uint64_t> &binv,
                  const std::vector<uint64_t> &w, std::vector<uint8_t> *from,
                  std::vector<uint8_t> *to, std::vector<uint8_t> *wt);

// Per-device view of a converter: what a launch needs (pointers are device memory).
struct BconvTables {
  uint32_t logn = 0, from_limbs = 0, to_limbs = 0;
  int word_bits = 0;
  const void *from = nullptr;        // BconvFrom<W>[from_limbs]
  const void *to = nullptr;          // BconvTo<W>[bconv_pad(to_limbs)], the padding repeats the last
  const void *w = nullptr;           // W[from_limbs][bconv_pad(to_limbs)]: Bh_i R mod c_j, padding 0
  const uint64_t *q = nullptr;       // c_0 .. c_{K-1}, b_0 .. b_{L-1} (range check)
};

// One launch on stream s.  op kBconvConvert: in [batch][L][n] -> out [batch][K][n];
// kBconvModdown: in [batch][K + L][n] -> out [batch][K][n].
hipError_t launch_bconv(const BconvTables &T, int op, void *out, const void *in, size_t batch,
                        hipStream_t s);
// The kernel launch_bconv launches for (T, op), as "k_bconv<u32,0>": the dry run of the launching
// statement itself (kernels_dev.hpp Emit)
hipError_t describe_bconv(const BconvTables &T, int op, std::string *out);

}  // namespace nttmul
