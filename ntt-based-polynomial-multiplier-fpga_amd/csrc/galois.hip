// galois.hip — launchers of the automorphism kernels (galois_dev.hpp).  The translation unit of
// the kernels lib/libnttmul_galois.so holds beyond libnttmul_rnsmp.so's.
#include "galois.hpp"
#include "galois_dev.hpp"

namespace nttmul {

// emit (kernels_dev.hpp) on a two-dimensional grid: bx workgroups of `threads` with `lds` bytes of
// dynamic LDS, one row of them per limb
template <class Name, class... KArgs>
static hipError_t emit_limbs(const Emit &E, Name name, void (*kernel)(KArgs...), size_t bx,
                             uint32_t limbs, int threads, size_t lds,
                             typename NoDeduce<KArgs>::type... args) {
  if (E.describe) {
    if (!E.describe->empty()) *E.describe += " + ";
    *E.describe += name();
    return hipSuccess;
  }
  if (bx == 0 || limbs == 0) return hipSuccess;
  if (bx > 0x7FFFFFFFull || limbs > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)bx, limbs), dim3(threads), lds, E.s, args...);
  return hipGetLastError();
}

// "k_galois_coeff<u32,0>": the kernel's own template arguments, all of them
template <class W>
static std::string galois_name(const char *kernel, int form = -1) {
  return std::string(kernel) + "<" + word_name<W>() +
         (form < 0 ? "" : "," + std::to_string(form)) + ">";
}

// The coefficient-order split, by n and the word: log2 of the residue classes a limb polynomial is
// staged in, the fewest whose n / M words fit kGaloisLdsBytes (0 up to n = 32768 on 32-bit words
// and 16384 on 64-bit words; at n = 65536: 1 and 2)
template <class W>
static int coeff_lgm(uint32_t logn) {
  int lgm = 0;
  while (((sizeof(W) << logn) >> lgm) > kGaloisLdsBytes) lgm++;
  return lgm;
}

template <class W, int LGM>
static hipError_t coeff(const GaloisTables &T, void *out, const void *in, uint32_t kinv,
                        size_t batch, const Emit &E) {
  // max(n / M, kGaloisStage) words per workgroup, a thread per 4 words up to 1024 threads
  const uint32_t span = std::max((1u << T.logn) >> LGM, kGaloisStage);
  // LGM = 0: span / n polynomials per workgroup; above: 8 M workgroups per 8 polynomials
  const size_t ppw = span >> (T.logn - LGM);
  const size_t bx = LGM ? ((batch + 7) / 8 * 8) << LGM : (batch + ppw - 1) / ppw;
  // (more dynamic LDS than a launch gets by default)
  if (!E.describe && span * sizeof(W) > (64u << 10)) {
    const hipError_t e = hipFuncSetAttribute((const void *)k_galois_coeff<W, LGM>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(span * sizeof(W)));
    if (e != hipSuccess) return e;
  }
  return emit_limbs(E, [] { return galois_name<W>("k_galois_coeff", LGM); },
                    k_galois_coeff<W, LGM>, bx, T.limbs, (int)std::min(1024u, span / 4),
                    span * sizeof(W), T.q, (const W *)in, (W *)out, kinv, T.logn, batch, T.limbs);
}

template <class W>
static hipError_t dispatch(const GaloisTables &T, int op, void *out, const void *in,
                           const GaloisKs &kv, uint32_t count, size_t batch, const Emit &E) {
  const uint32_t logn = T.logn;
  const size_t slices = batch << (logn - 8);
  const size_t bx = (slices + kGaloisSlices - 1) / kGaloisSlices;
  switch (op) {
    case kGaloisCoeff:
      switch (coeff_lgm<W>(logn)) {
        case 0: return coeff<W, 0>(T, out, in, kv.k[0], batch, E);
        case 1: return coeff<W, 1>(T, out, in, kv.k[0], batch, E);
        case 2:
          if constexpr (sizeof(W) == 8) return coeff<W, 2>(T, out, in, kv.k[0], batch, E);
          [[fallthrough]];
        default: return hipErrorNotSupported;
      }
    case kGaloisNtt:
      return emit_limbs(E, [] { return galois_name<W>("k_galois_ntt"); }, k_galois_ntt<W>, bx,
                        T.limbs, 256, 0, (const W *)in, (W *)out, kv.k[0], logn, slices, T.limbs);
    case kGaloisNttMany:
      return emit_limbs(E, [] { return galois_name<W>("k_galois_ntt_many"); },
                        k_galois_ntt_many<W>, bx, T.limbs, 256, 0, (const W *)in, (W *)out, kv,
                        count, logn, slices, T.limbs, (batch * T.limbs) << logn);
    default: return hipErrorInvalidValue;
  }
}

static hipError_t dispatch_words(const GaloisTables &T, int op, void *out, const void *in,
                                 const GaloisKs &kv, uint32_t count, size_t batch, const Emit &E) {
  if (T.logn < 8 || T.logn > 16) return hipErrorNotSupported;
  return T.word_bits == 32 ? dispatch<uint32_t>(T, op, out, in, kv, count, batch, E)
                           : dispatch<uint64_t>(T, op, out, in, kv, count, batch, E);
}

hipError_t launch_galois(const GaloisTables &T, int op, void *out, const void *in,
                         const GaloisKs &kv, uint32_t count, size_t batch, hipStream_t s) {
  return dispatch_words(T, op, out, in, kv, count, batch, Emit{s, nullptr});
}

hipError_t describe_galois(const GaloisTables &T, int op, std::string *out) {
  out->clear();
  return dispatch_words(T, op, nullptr, nullptr, GaloisKs{}, 1, 1, Emit{nullptr, out});
}

}  // namespace nttmul
