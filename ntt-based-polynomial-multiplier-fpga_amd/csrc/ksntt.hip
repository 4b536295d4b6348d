// ksntt.hip — launchers of the kernels of ksntt_dev.hpp.  The translation unit of the kernels
// lib/libnttmul_ksntt.so holds beyond libnttmul_mdntt.so's.  modup's inverse half is mdntt.hip's
// (launch_mdntt_inverse: k_mdntt_inv, or k_mdntt_inv_rows and rnsmp.hip's k_rnsmp_cols_inv) on a
// view of the Q limbs' folded table: no second copy of those kernels here.
#include "ksntt.hpp"
#include "ksntt_dev.hpp"

namespace nttmul {

// The forward kernels: a one-dimensional grid of bx workgroups per target (d, m), the target
// fastest
template <class... KArgs>
static hipError_t emit_targets(const Emit &E, const std::string &name, void (*kernel)(KArgs...),
                               size_t bx, uint32_t targets, typename NoDeduce<KArgs>::type... args) {
  if (E.describe) {
    if (!E.describe->empty()) *E.describe += " + ";
    *E.describe += name;
    return hipSuccess;
  }
  if (bx == 0 || targets == 0) return hipSuccess;
  if (bx > 0x7FFFFFFFull / targets) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(bx * targets)), dim3(256), 0, E.s, args...);
  return hipGetLastError();
}

// "k_ksntt_fwd<Arith32P,u32,12>", "k_ksntt_mac<Arith64,u64,2>": the kernel's own template
// arguments, all of them
template <class A, class IO>
static std::string ks_name(const char *kernel, int size) {
  return std::string(kernel) + "<" + AName<A>::v + "," + word_name<IO>() + "," +
         std::to_string(size) + ">";
}

// the inverse's view: the L limbs of Q as a compact [cnt][L][n] operand
static MdTables inverse_view(const KsnttTables &T) {
  MdTables V;
  V.logn = T.logn;
  V.L = 0;
  V.K = T.L;
  V.word_bits = T.word_bits;
  V.tab_inv = T.tab_inv;
  V.tw = T.tw;
  return V;
}

template <class A, class IO>
static hipError_t modup(const KsnttTables &T, void *up, const void *xh, size_t cnt,
                        void *const *scr, const Emit &E) {
  using W = typename A::word;
  const uint32_t targets = T.dnum * (T.L + T.K);
  hipError_t e = launch_mdntt_inverse(inverse_view(T), xh, cnt, scr, E.s, E.describe);
  if (e != hipSuccess) return e;
  const auto tab = (const KParams<A> *)T.tab_fwd;
  const auto tw = (const TwPair<W> *)T.tw;
  const auto to = (const BconvTo<W> *)T.to;
  const auto passes = [&](auto l1) {
    constexpr int L1 = decltype(l1)::value;
    hipError_t e2 = emit_targets(E, ks_name<A, IO>("k_ksntt_cols_fwd", L1),
                                 k_ksntt_cols_fwd<A, IO, L1>, ((cnt << kMpLogs) + 255) / 256,
                                 targets, tab, tw, to, (const W *)T.w, (const W *)scr[kMdY],
                                 (IO *)up, cnt, T.L, T.K, T.dnum, T.alpha);
    if (e2 != hipSuccess) return e2;
    return emit_targets(E, ks_name<A, IO>("k_ksntt_rows", L1), k_ksntt_rows<A, IO, L1>, cnt << L1,
                        targets, tab, tw, (const IO *)xh, (IO *)up, cnt << L1, T.L, T.K, T.dnum,
                        T.alpha);
  };
  switch (T.logn) {
    case 13: return passes(std::integral_constant<int, 1>{});
    case 14: return passes(std::integral_constant<int, 2>{});
    case 15: return passes(std::integral_constant<int, 3>{});
    case 16: return passes(std::integral_constant<int, 4>{});
    default: break;
  }
  if (T.logn > 12) return hipErrorNotSupported;
  return with_logn(T.logn, [&](auto logs) {
    constexpr int LOGS = decltype(logs)::value, PB = 256 / ((1 << LOGS) / 16);
    return emit_targets(E, ks_name<A, IO>("k_ksntt_fwd", LOGS), k_ksntt_fwd<A, IO, LOGS>,
                        (cnt + PB - 1) / PB, targets, tab, tw, to, (const W *)T.w,
                        (const W *)scr[kMdY], (const IO *)xh, (IO *)up, cnt, T.L, T.K, T.dnum,
                        T.alpha);
  });
}

// grid (workgroups over the batch's slices of 256 slots times rots, limbs)
template <class A, class IO, int COMPS>
static hipError_t mac(const KsnttTables &T, void *c, const void *a, const void *b,
                      const HoistArgs &H, size_t batch, uint32_t terms, const Emit &E) {
  using W = typename A::word;
  const std::string name = ks_name<A, IO>("k_ksntt_mac", COMPS);
  if (E.describe) {
    if (!E.describe->empty()) *E.describe += " + ";
    *E.describe += name;
    return hipSuccess;
  }
  const uint32_t limbs = T.L + T.K;
  const size_t slices = batch << (T.logn - 8);
  const size_t bx = (slices + kKsMacSlices - 1) / kKsMacSlices;
  if (bx == 0) return hipSuccess;
  if (!H.rots || bx > 0x7FFFFFFFull / H.rots || limbs > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_ksntt_mac<A, IO, COMPS>), dim3((unsigned)(bx * H.rots), limbs), dim3(256),
                     0, E.s, (const BconvTo<W> *)T.to, (const IO *)a, (const IO *)b, (IO *)c, H.ks,
                     H.rots, slices, terms, limbs, T.logn);
  return hipGetLastError();
}

template <class A, class IO>
static hipError_t mac_comps(const KsnttTables &T, void *c, const void *a, const void *b,
                            const HoistArgs &H, size_t batch, uint32_t terms, const Emit &E) {
  switch (H.comps) {
    case 1: return mac<A, IO, 1>(T, c, a, b, H, batch, terms, E);
    case 2: return mac<A, IO, 2>(T, c, a, b, H, batch, terms, E);
    default: return hipErrorInvalidValue;
  }
}

static bool shape_ok(const KsnttTables &T) {
  return T.L && T.K && T.alpha && T.dnum && T.logn >= 8 && T.logn <= 16 &&
         (T.word_bits == 32 || T.word_bits == 64);
}

hipError_t launch_ksntt_modup(const KsnttTables &T, void *up_hat, const void *x_hat, size_t cnt,
                              void *const *scr, hipStream_t s) {
  if (!shape_ok(T)) return hipErrorInvalidValue;
  const Emit E{s, nullptr};
  return T.word_bits == 32 ? modup<Arith32P, uint32_t>(T, up_hat, x_hat, cnt, scr, E)
                           : modup<Arith64, uint64_t>(T, up_hat, x_hat, cnt, scr, E);
}

hipError_t launch_ksntt_mac(const KsnttTables &T, void *c_hat, const void *a_hat,
                            const void *b_hat, const HoistArgs &H, size_t batch, uint32_t terms,
                            hipStream_t s) {
  if (!shape_ok(T)) return hipErrorInvalidValue;
  const Emit E{s, nullptr};
  return T.word_bits == 32
             ? mac_comps<Arith32P, uint32_t>(T, c_hat, a_hat, b_hat, H, batch, terms, E)
             : mac_comps<Arith64, uint64_t>(T, c_hat, a_hat, b_hat, H, batch, terms, E);
}

hipError_t describe_ksntt(const KsnttTables &T, int op, uint32_t comps, std::string *out) {
  out->clear();
  if (!shape_ok(T)) return hipErrorInvalidValue;
  const Emit E{nullptr, out};
  if (op == kKsnttModup) {
    void *const scr[kMdScratch] = {nullptr, nullptr, nullptr};
    return T.word_bits == 32 ? modup<Arith32P, uint32_t>(T, nullptr, nullptr, 1, scr, E)
                             : modup<Arith64, uint64_t>(T, nullptr, nullptr, 1, scr, E);
  }
  HoistArgs H = {};
  H.rots = 1;
  H.comps = comps;
  return T.word_bits == 32 ? mac_comps<Arith32P, uint32_t>(T, nullptr, nullptr, nullptr, H, 1, 1, E)
                           : mac_comps<Arith64, uint64_t>(T, nullptr, nullptr, nullptr, H, 1, 1, E);
}

}  // namespace nttmul
