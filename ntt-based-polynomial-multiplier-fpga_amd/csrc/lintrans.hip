// lintrans.hip — launcher of the kernel of lintrans_dev.hpp.  The translation unit of the kernels
// lib/libnttmul_lintrans.so holds beyond libnttmul_ksntt.so's.
#include "lintrans.hpp"
#include "lintrans_dev.hpp"

namespace nttmul {

// "k_lintrans<Arith32P,u32,2,1>": the kernel's own template arguments, all of them
template <class A, class IO, int COMPS, int WEIGHTED>
static std::string lt_name() {
  return std::string("k_lintrans<") + AName<A>::v + "," + word_name<IO>() + "," +
         std::to_string(COMPS) + "," + std::to_string(WEIGHTED) + ">";
}

// grid (lintrans_grid's workgroups, limbs)
template <class A, class IO, int COMPS, int WEIGHTED>
static hipError_t apply(const LtTables &T, void *c, const void *a, const void *b, const void *w,
                        const void *c0, const HoistArgs &H, size_t batch, uint32_t terms,
                        const Emit &E) {
  using W = typename A::word;
  if (E.describe) {
    if (!E.describe->empty()) *E.describe += " + ";
    *E.describe += lt_name<A, IO, COMPS, WEIGHTED>();
    return hipSuccess;
  }
  const uint32_t limbs = T.L + T.K;
  const LtGrid G = lintrans_grid(batch, T.logn, kLtSlotSliced, kLtV);
  if (G.wgx == 0) return hipSuccess;
  if (!H.rots || H.rots > kGaloisMaxCount || !G.ok || limbs > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_lintrans<A, IO, COMPS, WEIGHTED>), dim3((unsigned)G.wgx, limbs), dim3(256),
                     0, E.s, (const BconvTo<W> *)T.to, (const LtLimb<W> *)T.limb, (const IO *)a,
                     (const IO *)b, (const IO *)w, (const IO *)c0, (IO *)c, H.ks, H.rots, G.units,
                     (uint32_t)G.groups, terms, T.L, limbs, T.logn);
  return hipGetLastError();
}

template <class A, class IO>
static hipError_t apply_comps(const LtTables &T, void *c, const void *a, const void *b,
                              const void *w, const void *c0, const HoistArgs &H, size_t batch,
                              uint32_t terms, bool weighted, const Emit &E) {
  switch (H.comps * 2 + (weighted ? 1 : 0)) {
    case 2: return apply<A, IO, 1, 0>(T, c, a, b, w, c0, H, batch, terms, E);
    case 3: return apply<A, IO, 1, 1>(T, c, a, b, w, c0, H, batch, terms, E);
    case 4: return apply<A, IO, 2, 0>(T, c, a, b, w, c0, H, batch, terms, E);
    case 5: return apply<A, IO, 2, 1>(T, c, a, b, w, c0, H, batch, terms, E);
    default: return hipErrorInvalidValue;
  }
}

static bool shape_ok(const LtTables &T) {
  return T.L && T.K && T.logn >= 8 && T.logn <= 16 && (T.word_bits == 32 || T.word_bits == 64);
}

hipError_t launch_lintrans(const LtTables &T, void *c_hat, const void *a_hat, const void *b_hat,
                           const void *w_hat, const void *c0_hat, const HoistArgs &H, size_t batch,
                           uint32_t terms, hipStream_t s) {
  if (!shape_ok(T)) return hipErrorInvalidValue;
  const Emit E{s, nullptr};
  const bool weighted = w_hat != nullptr;
  return T.word_bits == 32 ? apply_comps<Arith32P, uint32_t>(T, c_hat, a_hat, b_hat, w_hat, c0_hat,
                                                             H, batch, terms, weighted, E)
                           : apply_comps<Arith64, uint64_t>(T, c_hat, a_hat, b_hat, w_hat, c0_hat,
                                                            H, batch, terms, weighted, E);
}

hipError_t describe_lintrans(const LtTables &T, uint32_t comps, bool weighted, std::string *out) {
  out->clear();
  if (!shape_ok(T)) return hipErrorInvalidValue;
  const Emit E{nullptr, out};
  HoistArgs H = {};
  H.rots = 1;
  H.comps = comps;
  return T.word_bits == 32 ? apply_comps<Arith32P, uint32_t>(T, nullptr, nullptr, nullptr, nullptr,
                                                             nullptr, H, 1, 1, weighted, E)
                           : apply_comps<Arith64, uint64_t>(T, nullptr, nullptr, nullptr, nullptr,
                                                            nullptr, H, 1, 1, weighted, E);
}

}  // namespace nttmul
