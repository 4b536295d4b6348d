// ctlin.hip — launchers of the kernels of ctlin_dev.hpp.  The translation unit of the kernels
// lib/libnttmul_ctlin.so holds beyond libnttmul_level.so's.
#include "ctlin.hpp"
#include "ctlin_dev.hpp"

namespace nttmul {

// "k_ctlin_combine<Arith32P,u32,2>": the kernel's own template arguments, all of them
template <class A, class IO>
static std::string cl_name(const char *kernel, int comps) {
  return std::string(kernel) + "<" + AName<A>::v + "," + word_name<IO>() +
         (comps ? "," + std::to_string(comps) : std::string()) + ">";
}

static bool describe(const Emit &E, const std::string &name) {
  if (!E.describe) return false;
  if (!E.describe->empty()) *E.describe += " + ";
  *E.describe += name;
  return true;
}

// grid (ctlin_grid's workgroups, L)
template <class A, class IO, int COMPS>
static hipError_t combine(const ClTables &T, void *out, const ClTerms &terms, size_t batch,
                          const Emit &E) {
  using W = typename A::word;
  if (describe(E, cl_name<A, IO>("k_ctlin_combine", COMPS))) return hipSuccess;
  const CtHighGrid G = ctlin_grid(batch, T.logn, T.word_bits);
  if (G.wgx == 0) return hipSuccess;
  if (!terms.nterms || terms.nterms > NTTMUL_CTLIN_MAX_TERMS || !G.ok ||
      G.vec * sizeof(IO) != 16)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_ctlin_combine<A, IO, COMPS>), dim3((unsigned)G.wgx, T.L), dim3(256), 0,
                     E.s, (const BconvTo<W> *)T.to, (const ClLimb<W> *)T.limb, terms, (IO *)out,
                     G.vectors, T.L, T.logn);
  return hipGetLastError();
}

template <class A, class IO>
static hipError_t combine_comps(const ClTables &T, void *out, const ClTerms &terms, size_t batch,
                                uint32_t comps, const Emit &E) {
  switch (comps) {
    case 1: return combine<A, IO, 1>(T, out, terms, batch, E);
    case 2: return combine<A, IO, 2>(T, out, terms, batch, E);
    case 3: return combine<A, IO, 3>(T, out, terms, batch, E);
  }
  return hipErrorInvalidValue;
}

template <class A, class IO>
static hipError_t tensor(const ClTables &T, void *d, const void *x, const void *y, size_t batch,
                         uint32_t pairs, const Emit &E) {
  using W = typename A::word;
  if (describe(E, cl_name<A, IO>("k_ctlin_tensor", 0))) return hipSuccess;
  const CtHighGrid G = ctlin_grid(batch, T.logn, T.word_bits);
  if (G.wgx == 0) return hipSuccess;
  if (!pairs || !G.ok || G.vec * sizeof(IO) != 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_ctlin_tensor<A, IO>), dim3((unsigned)G.wgx, T.L), dim3(256), 0, E.s,
                     (const BconvTo<W> *)T.to, (const IO *)x, (const IO *)y, (IO *)d, G.vectors,
                     pairs, T.L, T.logn);
  return hipGetLastError();
}

static bool shape_ok(const ClTables &T) {
  return T.L && T.L <= 65535u && T.logn >= 8 && T.logn <= 16 &&
         (T.word_bits == 32 || T.word_bits == 64);
}

hipError_t launch_ctlin_combine(const ClTables &T, void *out, const ClTerms &terms, size_t batch,
                                uint32_t comps, hipStream_t s) {
  if (!shape_ok(T)) return hipErrorInvalidValue;
  const Emit E{s, nullptr};
  return T.word_bits == 32 ? combine_comps<Arith32P, uint32_t>(T, out, terms, batch, comps, E)
                           : combine_comps<Arith64, uint64_t>(T, out, terms, batch, comps, E);
}

hipError_t launch_ctlin_tensor(const ClTables &T, void *d_hat, const void *x_hat,
                               const void *y_hat, size_t batch, uint32_t pairs, hipStream_t s) {
  if (!shape_ok(T)) return hipErrorInvalidValue;
  const Emit E{s, nullptr};
  return T.word_bits == 32 ? tensor<Arith32P, uint32_t>(T, d_hat, x_hat, y_hat, batch, pairs, E)
                           : tensor<Arith64, uint64_t>(T, d_hat, x_hat, y_hat, batch, pairs, E);
}

hipError_t describe_ctlin(const ClTables &T, int op, uint32_t comps, std::string *out) {
  out->clear();
  if (!shape_ok(T) || (op != kClCombine && op != kClTensor)) return hipErrorInvalidValue;
  const Emit E{nullptr, out};
  if (op == kClCombine) {
    const ClTerms none = {};
    return T.word_bits == 32 ? combine_comps<Arith32P, uint32_t>(T, nullptr, none, 1, comps, E)
                             : combine_comps<Arith64, uint64_t>(T, nullptr, none, 1, comps, E);
  }
  return T.word_bits == 32 ? tensor<Arith32P, uint32_t>(T, nullptr, nullptr, nullptr, 1, 1, E)
                           : tensor<Arith64, uint64_t>(T, nullptr, nullptr, nullptr, 1, 1, E);
}

}  // namespace nttmul
