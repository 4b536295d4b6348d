// tmd.hip — launchers of the kernels of tmd_dev.hpp.  The translation unit of the kernels
// lib/libnttmul_tmd.so holds beyond libnttmul_ctlin.so's.  The inverse half and the row pass
// above n = 4096 are mdntt.hip's own kernels, launched through launch_mdntt_inverse and
// launch_mdntt_rows on a view of this context's tables: no second copy of them here.
#include "tmd.hpp"
#include "tmd_dev.hpp"

namespace nttmul {

// The forward kernels: a one-dimensional grid of bx workgroups per limb of Q, the limb fastest
// (mdntt.hip emit_q_fastest)
template <class... KArgs>
static hipError_t emit_q_fastest(const Emit &E, const std::string &name, void (*kernel)(KArgs...),
                                 size_t bx, uint32_t limbs, typename NoDeduce<KArgs>::type... args) {
  if (E.describe) {
    if (!E.describe->empty()) *E.describe += " + ";
    *E.describe += name;
    return hipSuccess;
  }
  if (bx == 0 || limbs == 0) return hipSuccess;
  if (bx > 0x7FFFFFFFull / limbs) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(bx * limbs)), dim3(256), 0, E.s, args...);
  return hipGetLastError();
}

// "k_tmd_fwd<Arith32P,u32,12>", "k_tmd_cols_fwd<Arith64,u64,4>": the kernel's own template
// arguments, all of them
template <class A, class IO>
static std::string tm_name(const char *kernel, int size) {
  return std::string(kernel) + "<" + AName<A>::v + "," + word_name<IO>() + "," +
         std::to_string(size) + ">";
}

// mdntt.hip's view of this context (its w is not read by the launches taken from there)
static MdTables md_view(const TmTables &T) {
  MdTables V;
  V.logn = T.logn;
  V.L = T.L;
  V.K = T.K;
  V.word_bits = T.word_bits;
  V.tab_fwd = T.tab_fwd;
  V.tab_inv = T.tab_inv;
  V.tw = T.tw;
  V.to = T.to;
  V.w = T.w;
  return V;
}

// n <= 4096: the class is k_rns_xform's, plain Arith32P at every degree, Arith64 on 64-bit words
template <class A, class IO>
static hipError_t single(const TmTables &T, void *out, const void *xh, size_t cnt,
                         void *const *scr, const Emit &E) {
  using W = typename A::word;
  return with_logn(T.logn, [&](auto logs) {
    constexpr int LOGS = decltype(logs)::value, PB = 256 / ((1 << LOGS) / 16);
    return emit_q_fastest(E, tm_name<A, IO>("k_tmd_fwd", LOGS), k_tmd_fwd<A, IO, LOGS>,
                          (cnt + PB - 1) / PB, T.L, (const KParams<A> *)T.tab_fwd,
                          (const TwPair<W> *)T.tw, (const BconvTo<W> *)T.to, (const W *)T.w,
                          (const BconvTo<W> *)T.tt, (const W *)T.g, (const W *)scr[kMdY],
                          (const IO *)xh, (IO *)out, cnt, T.L, T.K);
  });
}

// n > 4096: one split per (class, n), 2^L1 x 4096
template <class A, class IO, int L1>
static hipError_t passes(const TmTables &T, void *out, const void *xh, size_t cnt,
                         void *const *scr, const Emit &E) {
  using W = typename A::word;
  const hipError_t e =
      emit_q_fastest(E, tm_name<A, IO>("k_tmd_cols_fwd", L1), k_tmd_cols_fwd<A, IO, L1>,
                     ((cnt << kMpLogs) + 255) / 256, T.L, (const KParams<A> *)T.tab_fwd,
                     (const TwPair<W> *)T.tw, (const BconvTo<W> *)T.to, (const W *)T.w,
                     (const BconvTo<W> *)T.tt, (const W *)T.g, (const W *)scr[kMdY],
                     (W *)scr[kMdT], cnt, T.L, T.K);
  if (e != hipSuccess) return e;
  return launch_mdntt_rows(md_view(T), out, xh, cnt, scr, E.s, E.describe);
}

template <class A, class IO>
static hipError_t dispatch(const TmTables &T, void *out, const void *xh, size_t cnt,
                           void *const *scr, const Emit &E) {
  const hipError_t e = launch_mdntt_inverse(md_view(T), xh, cnt, scr, E.s, E.describe);
  if (e != hipSuccess) return e;
  switch (T.logn) {
    case 13: return passes<A, IO, 1>(T, out, xh, cnt, scr, E);
    case 14: return passes<A, IO, 2>(T, out, xh, cnt, scr, E);
    case 15: return passes<A, IO, 3>(T, out, xh, cnt, scr, E);
    case 16: return passes<A, IO, 4>(T, out, xh, cnt, scr, E);
    default: return T.logn <= 12 ? single<A, IO>(T, out, xh, cnt, scr, E) : hipErrorNotSupported;
  }
}

static hipError_t dispatch_words(const TmTables &T, void *out, const void *xh, size_t cnt,
                                 void *const *scr, const Emit &E) {
  if (!T.L || !T.K) return hipErrorInvalidValue;
  return T.word_bits == 32 ? dispatch<Arith32P, uint32_t>(T, out, xh, cnt, scr, E)
                           : dispatch<Arith64, uint64_t>(T, out, xh, cnt, scr, E);
}

hipError_t launch_tmd(const TmTables &T, void *out, const void *x_hat, size_t cnt,
                      void *const *scr, hipStream_t s) {
  return dispatch_words(T, out, x_hat, cnt, scr, Emit{s, nullptr});
}

hipError_t describe_tmd(const TmTables &T, std::string *out) {
  out->clear();
  void *const scr[kMdScratch] = {nullptr, nullptr, nullptr};
  return dispatch_words(T, nullptr, nullptr, 1, scr, Emit{nullptr, out});
}

}  // namespace nttmul
