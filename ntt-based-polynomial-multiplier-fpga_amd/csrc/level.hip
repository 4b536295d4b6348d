// level.hip — launchers of the kernels of level_dev.hpp.  The translation unit of the kernels
// lib/libnttmul_level.so holds beyond libnttmul_xconv.so's.
#include "level.hpp"
#include "level_dev.hpp"

namespace nttmul {

// level_plan.hpp's grids are the kernels' slicing
static_assert(kLevelMacSlices == (uint32_t)kKsMacSlices, "level_mac_grid is k_level_mac's grid");

static bool describe(const Emit &E, const std::string &name) {
  if (!E.describe) return false;
  if (!E.describe->empty()) *E.describe += " + ";
  *E.describe += name;
  return true;
}

// "k_level_mac<Arith64,u64,2>", "k_level_lintrans<Arith64,u64,2,1>", "k_level_relin<Arith64,u64>":
// the kernel's own template arguments, all of them
template <class A, class IO>
static std::string lv_name(const char *kernel, std::initializer_list<int> sizes) {
  std::string s = std::string(kernel) + "<" + AName<A>::v + "," + word_name<IO>();
  for (int v : sizes) s += "," + std::to_string(v);
  return s + ">";
}

// what every launch requires of the view beyond the entry points' status: the addresses below
// stay inside the operand only then
static bool addr_ok(const LevelAddr &A, uint32_t L, uint32_t K, uint32_t logn, uint32_t terms) {
  return A.L == L && A.K == K && A.logn == logn && A.top_limbs >= L + K &&
         A.shift == A.top_limbs - (L + K) && A.top_terms >= terms &&
         A.kstep == (size_t)A.top_limbs << logn && A.kcstep == A.kstep * A.top_terms;
}

// grid (level_mac_grid's workgroups, limbs): k_ksntt_mac's
template <class A, class IO, int COMPS>
static hipError_t mac(const KsnttTables &T, void *c, const void *a, const void *b,
                      const HoistArgs &H, size_t batch, uint32_t terms, const LevelAddr &V,
                      const Emit &E) {
  using W = typename A::word;
  if (describe(E, lv_name<A, IO>("k_level_mac", {COMPS}))) return hipSuccess;
  const uint32_t limbs = T.L + T.K;
  const LevelMacGrid G = level_mac_grid(batch, T.logn, H.rots);
  if (G.bx == 0) return hipSuccess;
  if (!H.rots || !G.ok || limbs > 65535u || !addr_ok(V, T.L, T.K, T.logn, terms))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_level_mac<A, IO, COMPS>), dim3((unsigned)G.wgx, limbs), dim3(256), 0, E.s,
                     (const BconvTo<W> *)T.to, (const IO *)a, (const IO *)b, (IO *)c, H.ks, H.rots,
                     G.slices, terms, T.L, limbs, V.top_limbs, V.top_terms, T.logn);
  return hipGetLastError();
}

template <class A, class IO>
static hipError_t mac_comps(const KsnttTables &T, void *c, const void *a, const void *b,
                            const HoistArgs &H, size_t batch, uint32_t terms, const LevelAddr &V,
                            const Emit &E) {
  switch (H.comps) {
    case 1: return mac<A, IO, 1>(T, c, a, b, H, batch, terms, V, E);
    case 2: return mac<A, IO, 2>(T, c, a, b, H, batch, terms, V, E);
    default: return hipErrorInvalidValue;
  }
}

// grid (level_lintrans_grid's workgroups, limbs): k_lintrans's
template <class A, class IO, int COMPS, int WEIGHTED>
static hipError_t apply(const LtTables &T, void *c, const void *a, const void *b, const void *w,
                        const void *c0, const HoistArgs &H, size_t batch, uint32_t terms,
                        const LevelAddr &V, const Emit &E) {
  using W = typename A::word;
  if (describe(E, lv_name<A, IO>("k_level_lintrans", {COMPS, WEIGHTED}))) return hipSuccess;
  const uint32_t limbs = T.L + T.K;
  const LtGrid G = level_lintrans_grid(batch, T.logn);
  if (G.wgx == 0) return hipSuccess;
  if (!H.rots || H.rots > kGaloisMaxCount || !G.ok || limbs > 65535u ||
      !addr_ok(V, T.L, T.K, T.logn, terms))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_level_lintrans<A, IO, COMPS, WEIGHTED>), dim3((unsigned)G.wgx, limbs),
                     dim3(256), 0, E.s, (const BconvTo<W> *)T.to, (const LtLimb<W> *)T.limb,
                     (const IO *)a, (const IO *)b, (const IO *)w, (const IO *)c0, (IO *)c, H.ks,
                     H.rots, G.units, terms, T.L, limbs, V.top_limbs, V.top_terms, T.logn);
  return hipGetLastError();
}

template <class A, class IO>
static hipError_t apply_comps(const LtTables &T, void *c, const void *a, const void *b,
                              const void *w, const void *c0, const HoistArgs &H, size_t batch,
                              uint32_t terms, bool weighted, const LevelAddr &V, const Emit &E) {
  switch (H.comps * 2 + (weighted ? 1 : 0)) {
    case 2: return apply<A, IO, 1, 0>(T, c, a, b, w, c0, H, batch, terms, V, E);
    case 3: return apply<A, IO, 1, 1>(T, c, a, b, w, c0, H, batch, terms, V, E);
    case 4: return apply<A, IO, 2, 0>(T, c, a, b, w, c0, H, batch, terms, V, E);
    case 5: return apply<A, IO, 2, 1>(T, c, a, b, w, c0, H, batch, terms, V, E);
    default: return hipErrorInvalidValue;
  }
}

// grid (level_relin_grid's workgroups, limbs): k_ctmul_relin's
template <class A, class IO>
static hipError_t relin(const CtTables &T, void *c, const void *up, const void *key, const void *x,
                        const void *y, size_t batch, uint32_t pairs, uint32_t terms,
                        const LevelAddr &V, const Emit &E) {
  using W = typename A::word;
  if (describe(E, lv_name<A, IO>("k_level_relin", {}))) return hipSuccess;
  const uint32_t limbs = T.L + T.K;
  const LtGrid G = level_relin_grid(batch, T.logn);
  if (G.wgx == 0) return hipSuccess;
  if (!pairs || !terms || !G.ok || limbs > 65535u || !addr_ok(V, T.L, T.K, T.logn, terms))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_level_relin<A, IO>), dim3((unsigned)G.wgx, limbs), dim3(256), 0, E.s,
                     (const BconvTo<W> *)T.to, (const CtLimb<W> *)T.limb, (const IO *)up,
                     (const IO *)key, (const IO *)x, (const IO *)y, (IO *)c, batch, pairs, terms,
                     T.L, limbs, V.top_limbs, V.top_terms, T.logn);
  return hipGetLastError();
}

static bool shape_ok(uint32_t L, uint32_t K, uint32_t logn, int word_bits) {
  return L && K && logn >= 8 && logn <= 16 && (word_bits == 32 || word_bits == 64);
}

hipError_t launch_level_mac(const KsnttTables &T, void *c_hat, const void *a_hat,
                            const void *b_hat, const HoistArgs &H, size_t batch, uint32_t terms,
                            const LevelAddr &A, hipStream_t s) {
  if (!shape_ok(T.L, T.K, T.logn, T.word_bits)) return hipErrorInvalidValue;
  const Emit E{s, nullptr};
  return T.word_bits == 32
             ? mac_comps<Arith32P, uint32_t>(T, c_hat, a_hat, b_hat, H, batch, terms, A, E)
             : mac_comps<Arith64, uint64_t>(T, c_hat, a_hat, b_hat, H, batch, terms, A, E);
}

hipError_t launch_level_lintrans(const LtTables &T, void *c_hat, const void *a_hat,
                                 const void *b_hat, const void *w_hat, const void *c0_hat,
                                 const HoistArgs &H, size_t batch, uint32_t terms,
                                 const LevelAddr &A, hipStream_t s) {
  if (!shape_ok(T.L, T.K, T.logn, T.word_bits)) return hipErrorInvalidValue;
  const Emit E{s, nullptr};
  const bool weighted = w_hat != nullptr;
  return T.word_bits == 32
             ? apply_comps<Arith32P, uint32_t>(T, c_hat, a_hat, b_hat, w_hat, c0_hat, H, batch,
                                               terms, weighted, A, E)
             : apply_comps<Arith64, uint64_t>(T, c_hat, a_hat, b_hat, w_hat, c0_hat, H, batch,
                                              terms, weighted, A, E);
}

hipError_t launch_level_relin(const CtTables &T, void *c_hat, const void *up_hat,
                              const void *key_hat, const void *x_hat, const void *y_hat,
                              size_t batch, uint32_t pairs, uint32_t terms, const LevelAddr &A,
                              hipStream_t s) {
  if (!shape_ok(T.L, T.K, T.logn, T.word_bits)) return hipErrorInvalidValue;
  const Emit E{s, nullptr};
  return T.word_bits == 32
             ? relin<Arith32P, uint32_t>(T, c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs,
                                         terms, A, E)
             : relin<Arith64, uint64_t>(T, c_hat, up_hat, key_hat, x_hat, y_hat, batch, pairs,
                                        terms, A, E);
}

hipError_t launch_level_check(const void *op, const uint64_t *q, int word_bits, const LevelAddr &A,
                              size_t outer, uint32_t terms, bool has_terms, int *bad,
                              hipStream_t s) {
  if (!addr_ok(A, A.L, A.K, A.logn, has_terms ? terms : 0) || !terms || (!has_terms && terms != 1))
    return hipErrorInvalidValue;
  const LevelCheckGrid G = level_check_grid(A, outer, terms);
  if (G.wgx == 0) return hipSuccess;
  if (!G.ok) return hipErrorInvalidValue;
  const uint32_t limbs = A.L + A.K;
  const size_t ostride = has_terms ? A.kcstep : A.kstep;
  return word_bits == 32
             ? launch(k_level_check_range<uint32_t>, G.wgx, 256, s, (const uint32_t *)op, q,
                      G.total, A.logn, A.L, limbs, A.top_limbs, terms, ostride, bad)
             : launch(k_level_check_range<uint64_t>, G.wgx, 256, s, (const uint64_t *)op, q,
                      G.total, A.logn, A.L, limbs, A.top_limbs, terms, ostride, bad);
}

hipError_t describe_level(int op, uint32_t logn, int word_bits, uint32_t comps, bool weighted,
                          std::string *out) {
  out->clear();
  if (!shape_ok(1, 1, logn, word_bits)) return hipErrorInvalidValue;
  const Emit E{nullptr, out};
  const LevelAddr A;
  HoistArgs H = {};
  H.rots = 1;
  H.comps = comps;
  const bool w32 = word_bits == 32;
  switch (op) {
    case kLevelMac: {
      const KsnttTables T;
      return w32 ? mac_comps<Arith32P, uint32_t>(T, nullptr, nullptr, nullptr, H, 1, 1, A, E)
                 : mac_comps<Arith64, uint64_t>(T, nullptr, nullptr, nullptr, H, 1, 1, A, E);
    }
    case kLevelLintrans: {
      const LtTables T;
      return w32 ? apply_comps<Arith32P, uint32_t>(T, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                   H, 1, 1, weighted, A, E)
                 : apply_comps<Arith64, uint64_t>(T, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                  H, 1, 1, weighted, A, E);
    }
    case kLevelRelin: {
      const CtTables T;
      return w32 ? relin<Arith32P, uint32_t>(T, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1,
                                             1, A, E)
                 : relin<Arith64, uint64_t>(T, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1,
                                            1, A, E);
    }
    default: return hipErrorInvalidValue;
  }
}

}  // namespace nttmul
