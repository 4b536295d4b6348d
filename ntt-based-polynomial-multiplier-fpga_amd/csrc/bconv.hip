// bconv.hip — launchers of the base-conversion kernel (bconv_dev.hpp).  The translation unit of
// the kernels lib/libnttmul_bconv.so holds beyond libnttmul_rns.so's.
#include "bconv_dev.hpp"

namespace nttmul {

template <class W, int OP>
static hipError_t convert(const BconvTables &T, void *out, const void *in, size_t batch,
                          const Emit &E) {
  constexpr int V = BconvArith<W>::kV;
  const size_t slices = batch << (T.logn - 8), blocks = (slices + V - 1) / V;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  return emit(E, [] { return std::string("k_bconv<") + word_name<W>() + "," + std::to_string(OP) + ">"; },
              k_bconv<W, OP>, blocks, 256, (const BconvFrom<W> *)T.from, (const BconvTo<W> *)T.to,
              (const W *)T.w, (const W *)in, (W *)out, slices, T.logn, T.from_limbs, T.to_limbs);
}

template <class W>
static hipError_t dispatch(const BconvTables &T, int op, void *out, const void *in, size_t batch,
                           const Emit &E) {
  switch (op) {
    case kBconvConvert: return convert<W, kBconvConvert>(T, out, in, batch, E);
    case kBconvModdown: return convert<W, kBconvModdown>(T, out, in, batch, E);
    default: return hipErrorInvalidValue;
  }
}

static hipError_t dispatch_words(const BconvTables &T, int op, void *out, const void *in,
                                 size_t batch, const Emit &E) {
  // (nttmul_bconv_create stops at n = 4096 in bconv.cpp's validate; lib/libnttmul_ks.so's ModDown
  // launches the same kernel up to n = 65536: k_bconv takes logn and 64-bit offsets)
  if (T.logn < 8 || T.logn > 16 || !T.from_limbs || !T.to_limbs) return hipErrorInvalidValue;
  return T.word_bits == 32 ? dispatch<uint32_t>(T, op, out, in, batch, E)
                           : dispatch<uint64_t>(T, op, out, in, batch, E);
}

hipError_t launch_bconv(const BconvTables &T, int op, void *out, const void *in, size_t batch,
                        hipStream_t s) {
  return dispatch_words(T, op, out, in, batch, Emit{s, nullptr});
}

hipError_t describe_bconv(const BconvTables &T, int op, std::string *out) {
  out->clear();
  return dispatch_words(T, op, nullptr, nullptr, 1, Emit{nullptr, out});
}

}  // namespace nttmul
