// ks.hip — launcher of the digit ModUp kernel (ks_dev.hpp).  The translation unit of the kernels
// lib/libnttmul_ks.so holds beyond libnttmul_galois.so's: k_ks_modup only (ModDown launches
// bconv.hip's k_bconv through launch_bconv; k_bconv is not instantiated here).
#include "ks_dev.hpp"

namespace nttmul {

// emit (kernels_dev.hpp) on a two-dimensional grid: bx workgroups of `threads`, one row of them
// per digit
template <class Name, class... KArgs>
static hipError_t emit_digits(const Emit &E, Name name, void (*kernel)(KArgs...), size_t bx,
                              uint32_t digits, int threads,
                              typename NoDeduce<KArgs>::type... args) {
  if (E.describe) {
    if (!E.describe->empty()) *E.describe += " + ";
    *E.describe += name();
    return hipSuccess;
  }
  if (bx == 0 || digits == 0) return hipSuccess;
  if (bx > 0x7FFFFFFFull || digits > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)bx, digits), dim3(threads), 0, E.s, args...);
  return hipGetLastError();
}

template <class W>
static hipError_t modup(const KsTables &T, void *out, const void *in, size_t batch,
                        const Emit &E) {
  constexpr int V = BconvArith<W>::kV;
  const size_t slices = batch << (T.logn - 8), blocks = (slices + V - 1) / V;
  return emit_digits(E, [] { return std::string("k_ks_modup<") + word_name<W>() + ">"; },
                     k_ks_modup<W>, blocks, T.digits, 256, (const BconvFrom<W> *)T.from,
                     (const BconvTo<W> *)T.to, (const W *)T.w, (const W *)in, (W *)out, slices,
                     T.logn, T.q_limbs, T.q_limbs + T.p_limbs, T.digit_limbs);
}

static hipError_t dispatch_words(const KsTables &T, void *out, const void *in, size_t batch,
                                 const Emit &E) {
  if (T.logn < 8 || T.logn > 16 || !T.q_limbs || !T.p_limbs || !T.digit_limbs ||
      T.digit_limbs > T.q_limbs ||
      T.digits != (T.q_limbs + T.digit_limbs - 1) / T.digit_limbs)
    return hipErrorInvalidValue;
  return T.word_bits == 32 ? modup<uint32_t>(T, out, in, batch, E)
                           : modup<uint64_t>(T, out, in, batch, E);
}

hipError_t launch_ks_modup(const KsTables &T, void *out, const void *in, size_t batch,
                           hipStream_t s) {
  return dispatch_words(T, out, in, batch, Emit{s, nullptr});
}

hipError_t describe_ks_modup(const KsTables &T, std::string *out) {
  out->clear();
  return dispatch_words(T, nullptr, nullptr, 1, Emit{nullptr, out});
}

}  // namespace nttmul
