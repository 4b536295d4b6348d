// ctmul.hip — launchers of the kernels of ctmul_dev.hpp.  The translation unit of the kernels
// lib/libnttmul_ctmul.so holds beyond libnttmul_lintrans.so's.
#include "ctmul.hpp"
#include "ctmul_dev.hpp"

namespace nttmul {

// "k_ctmul_relin<Arith32P,u32>": the kernel's own template arguments, all of them
template <class A, class IO>
static std::string ct_name(const char *kernel) {
  return std::string(kernel) + "<" + AName<A>::v + "," + word_name<IO>() + ">";
}

static bool describe(const Emit &E, const std::string &name) {
  if (!E.describe) return false;
  if (!E.describe->empty()) *E.describe += " + ";
  *E.describe += name;
  return true;
}

// grid (ctmul_high_grid's workgroups, L)
template <class A, class IO>
static hipError_t high(const CtTables &T, void *d2, const void *x, const void *y, size_t batch,
                       uint32_t pairs, const Emit &E) {
  using W = typename A::word;
  if (describe(E, ct_name<A, IO>("k_ctmul_high"))) return hipSuccess;
  const CtHighGrid G = ctmul_high_grid(batch, T.logn, T.word_bits);
  if (G.wgx == 0) return hipSuccess;
  if (!pairs || !G.ok || G.vec * sizeof(IO) != 16) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_ctmul_high<A, IO>), dim3((unsigned)G.wgx, T.L), dim3(256), 0, E.s,
                     (const BconvTo<W> *)T.to, (const IO *)x, (const IO *)y, (IO *)d2, G.vectors,
                     pairs, T.L, T.logn);
  return hipGetLastError();
}

// grid (ctmul_relin_grid's workgroups, limbs)
template <class A, class IO>
static hipError_t relin(const CtTables &T, void *c, const void *up, const void *key, const void *x,
                        const void *y, size_t batch, uint32_t pairs, uint32_t terms,
                        const Emit &E) {
  using W = typename A::word;
  if (describe(E, ct_name<A, IO>("k_ctmul_relin"))) return hipSuccess;
  const uint32_t limbs = T.L + T.K;
  const LtGrid G = ctmul_relin_grid(batch, T.logn, ctmul_slices(T.word_bits));
  if (G.wgx == 0) return hipSuccess;
  if (!pairs || !terms || !G.ok) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_ctmul_relin<A, IO>), dim3((unsigned)G.wgx, limbs), dim3(256), 0, E.s,
                     (const BconvTo<W> *)T.to, (const CtLimb<W> *)T.limb, (const IO *)up,
                     (const IO *)key, (const IO *)x, (const IO *)y, (IO *)c, batch, pairs, terms,
                     T.L, limbs, T.logn);
  return hipGetLastError();
}

static bool shape_ok(const CtTables &T) {
  return T.L && T.K && T.L + T.K <= 65535u && T.logn >= 8 && T.logn <= 16 &&
         (T.word_bits == 32 || T.word_bits == 64);
}

hipError_t launch_ctmul_high(const CtTables &T, void *d2_hat, const void *x_hat, const void *y_hat,
                             size_t batch, uint32_t pairs, hipStream_t s) {
  if (!shape_ok(T)) return hipErrorInvalidValue;
  const Emit E{s, nullptr};
  return T.word_bits == 32 ? high<Arith32P, uint32_t>(T, d2_hat, x_hat, y_hat, batch, pairs, E)
                           : high<Arith64, uint64_t>(T, d2_hat, x_hat, y_hat, batch, pairs, E);
}

hipError_t launch_ctmul_relin(const CtTables &T, void *c_hat, const void *up_hat,
                              const void *key_hat, const void *x_hat, const void *y_hat,
                              size_t batch, uint32_t pairs, uint32_t terms, hipStream_t s) {
  if (!shape_ok(T)) return hipErrorInvalidValue;
  const Emit E{s, nullptr};
  return T.word_bits == 32
             ? relin<Arith32P, uint32_t>(T, c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs,
                                         terms, E)
             : relin<Arith64, uint64_t>(T, c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs,
                                        terms, E);
}

hipError_t describe_ctmul(const CtTables &T, int op, std::string *out) {
  out->clear();
  if (!shape_ok(T) || (op != kCtHigh && op != kCtRelin)) return hipErrorInvalidValue;
  const Emit E{nullptr, out};
  if (op == kCtHigh)
    return T.word_bits == 32 ? high<Arith32P, uint32_t>(T, nullptr, nullptr, nullptr, 1, 1, E)
                             : high<Arith64, uint64_t>(T, nullptr, nullptr, nullptr, 1, 1, E);
  return T.word_bits == 32
             ? relin<Arith32P, uint32_t>(T, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, 1, E)
             : relin<Arith64, uint64_t>(T, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, 1, E);
}

}  // namespace nttmul
