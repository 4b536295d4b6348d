// mdntt.hip — launchers of the kernels of mdntt_dev.hpp.  The translation unit of the kernels
// lib/libnttmul_mdntt.so holds beyond libnttmul_hoist.so's.  The inverse column pass above
// n = 4096 is rnsmp.hip's own kernel, launched through launch_rnsmp_cols on a view of the P limbs'
// tables: no second copy of it here.
#include "mdntt.hpp"
#include "mdntt_dev.hpp"

namespace nttmul {

// The inverse kernels: one row of workgroups per limb of P (rns.hip emit_limbs, 256 threads)
template <class... KArgs>
static hipError_t emit_p_limbs(const Emit &E, const std::string &name, void (*kernel)(KArgs...),
                               size_t bx, uint32_t limbs, typename NoDeduce<KArgs>::type... args) {
  if (E.describe) {
    if (!E.describe->empty()) *E.describe += " + ";
    *E.describe += name;
    return hipSuccess;
  }
  if (bx == 0 || limbs == 0) return hipSuccess;
  if (bx > 0x7FFFFFFFull || limbs > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)bx, limbs), dim3(256), 0, E.s, args...);
  return hipGetLastError();
}

// The forward kernels: a one-dimensional grid of bx workgroups per limb of Q, the limb fastest
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

// "k_mdntt_fwd<Arith32P,u32,12>", "k_mdntt_rows<Arith64,u64,4>": the kernel's own template
// arguments, all of them
template <class A, class IO>
static std::string md_name(const char *kernel, int size) {
  return std::string(kernel) + "<" + AName<A>::v + "," + word_name<IO>() + "," +
         std::to_string(size) + ">";
}

template <class A>
static const TwPair<typename A::word> *p_twiddles(const MdTables &T) {
  return (const TwPair<typename A::word> *)T.tw + (((size_t)T.L * 2) << T.logn);
}

// The inverse half, n <= 4096: limb L + j of x_hat -> y (scr[kMdY])
template <class A, class IO>
static hipError_t single_inv(const MdTables &T, const void *xh, size_t cnt, void *const *scr,
                             const Emit &E) {
  using W = typename A::word;
  return with_logn(T.logn, [&](auto logs) {
    constexpr int LOGS = decltype(logs)::value, PB = 256 / ((1 << LOGS) / 16);
    constexpr int PBI = PB * xform_upg<A, 0, 1>();
    return emit_p_limbs(E, md_name<A, IO>("k_mdntt_inv", LOGS), k_mdntt_inv<A, IO, LOGS>,
                        (cnt + PBI - 1) / PBI, T.K, (const KParams<A> *)T.tab_inv,
                        p_twiddles<A>(T), (const IO *)xh, (W *)scr[kMdY], cnt, T.L, T.K);
  });
}

// n <= 4096: the class is k_rns_xform's, plain Arith32P at every degree, Arith64 on 64-bit words
template <class A, class IO>
static hipError_t single(const MdTables &T, void *out, const void *xh, size_t cnt,
                         void *const *scr, const Emit &E) {
  using W = typename A::word;
  const hipError_t e = single_inv<A, IO>(T, xh, cnt, scr, E);
  if (e != hipSuccess) return e;
  return with_logn(T.logn, [&](auto logs) {
    constexpr int LOGS = decltype(logs)::value, PB = 256 / ((1 << LOGS) / 16);
    return emit_q_fastest(E, md_name<A, IO>("k_mdntt_fwd", LOGS), k_mdntt_fwd<A, IO, LOGS>,
                          (cnt + PB - 1) / PB, T.L, (const KParams<A> *)T.tab_fwd,
                          (const TwPair<W> *)T.tw, (const BconvTo<W> *)T.to, (const W *)T.w,
                          (const W *)scr[kMdY], (const IO *)xh, (IO *)out, cnt, T.L, T.K);
  });
}

// The inverse half, n > 4096: the rows of limb L + j into scr[kMdYLazy], the column pass into y
// (scr[kMdY])
template <class A, class IO, int L1>
static hipError_t passes_inv(const MdTables &T, const void *xh, size_t cnt, void *const *scr,
                             const Emit &E) {
  using W = typename A::word;
  hipError_t e = emit_p_limbs(E, md_name<A, IO>("k_mdntt_inv_rows", L1),
                              k_mdntt_inv_rows<A, IO, L1>, cnt << L1, T.K,
                              (const KParams<A> *)T.tab_inv, p_twiddles<A>(T), (const IO *)xh,
                              (W *)scr[kMdYLazy], cnt << L1, T.L, T.K);
  if (e != hipSuccess) return e;
  // k_rnsmp_cols_inv over the K limbs of P: launch_rnsmp_cols reads tab[kRnsTransform] and tw
  RnsTables V;
  V.logn = T.logn;
  V.limbs = T.K;
  V.word_bits = T.word_bits;
  V.tab[kRnsTransform] = T.tab_inv;
  V.tw = p_twiddles<A>(T);
  return launch_rnsmp_cols(V, 1, scr[kMdY], scr[kMdYLazy], cnt, E.s, E.describe);
}

// n > 4096: one split per (class, n), 2^L1 x 4096
template <class A, class IO, int L1>
static hipError_t passes(const MdTables &T, void *out, const void *xh, size_t cnt,
                         void *const *scr, const Emit &E) {
  using W = typename A::word;
  hipError_t e = passes_inv<A, IO, L1>(T, xh, cnt, scr, E);
  if (e != hipSuccess) return e;
  e = emit_q_fastest(E, md_name<A, IO>("k_mdntt_cols_fwd", L1), k_mdntt_cols_fwd<A, IO, L1>,
                     ((cnt << kMpLogs) + 255) / 256, T.L, (const KParams<A> *)T.tab_fwd,
                     (const TwPair<W> *)T.tw, (const BconvTo<W> *)T.to, (const W *)T.w,
                     (const W *)scr[kMdY], (W *)scr[kMdT], cnt, T.L, T.K);
  if (e != hipSuccess) return e;
  return emit_q_fastest(E, md_name<A, IO>("k_mdntt_rows", L1), k_mdntt_rows<A, IO, L1>,
                        cnt << L1, T.L, (const KParams<A> *)T.tab_fwd, (const TwPair<W> *)T.tw,
                        (const BconvTo<W> *)T.to, (const W *)scr[kMdT], (const IO *)xh, (IO *)out,
                        cnt << L1, T.L, T.K);
}

template <class A, class IO>
static hipError_t dispatch(const MdTables &T, void *out, const void *xh, size_t cnt,
                           void *const *scr, const Emit &E) {
  switch (T.logn) {
    case 13: return passes<A, IO, 1>(T, out, xh, cnt, scr, E);
    case 14: return passes<A, IO, 2>(T, out, xh, cnt, scr, E);
    case 15: return passes<A, IO, 3>(T, out, xh, cnt, scr, E);
    case 16: return passes<A, IO, 4>(T, out, xh, cnt, scr, E);
    default: return T.logn <= 12 ? single<A, IO>(T, out, xh, cnt, scr, E) : hipErrorNotSupported;
  }
}

static hipError_t dispatch_words(const MdTables &T, void *out, const void *xh, size_t cnt,
                                 void *const *scr, const Emit &E) {
  if (!T.L || !T.K) return hipErrorInvalidValue;
  return T.word_bits == 32 ? dispatch<Arith32P, uint32_t>(T, out, xh, cnt, scr, E)
                           : dispatch<Arith64, uint64_t>(T, out, xh, cnt, scr, E);
}

template <class A, class IO>
static hipError_t dispatch_inv(const MdTables &T, const void *xh, size_t cnt, void *const *scr,
                               const Emit &E) {
  switch (T.logn) {
    case 13: return passes_inv<A, IO, 1>(T, xh, cnt, scr, E);
    case 14: return passes_inv<A, IO, 2>(T, xh, cnt, scr, E);
    case 15: return passes_inv<A, IO, 3>(T, xh, cnt, scr, E);
    case 16: return passes_inv<A, IO, 4>(T, xh, cnt, scr, E);
    default: return T.logn <= 12 ? single_inv<A, IO>(T, xh, cnt, scr, E) : hipErrorNotSupported;
  }
}

hipError_t launch_mdntt_inverse(const MdTables &T, const void *x_hat, size_t cnt,
                                void *const *scr, hipStream_t s, std::string *describe) {
  if (!T.K) return hipErrorInvalidValue;
  const Emit E{s, describe};
  return T.word_bits == 32 ? dispatch_inv<Arith32P, uint32_t>(T, x_hat, cnt, scr, E)
                           : dispatch_inv<Arith64, uint64_t>(T, x_hat, cnt, scr, E);
}

template <class A, class IO>
static hipError_t dispatch_rows(const MdTables &T, void *out, const void *xh, size_t cnt,
                                void *const *scr, const Emit &E) {
  using W = typename A::word;
  const auto rows = [&](auto l1) {
    constexpr int L1 = decltype(l1)::value;
    return emit_q_fastest(E, md_name<A, IO>("k_mdntt_rows", L1), k_mdntt_rows<A, IO, L1>,
                          cnt << L1, T.L, (const KParams<A> *)T.tab_fwd, (const TwPair<W> *)T.tw,
                          (const BconvTo<W> *)T.to, (const W *)scr[kMdT], (const IO *)xh, (IO *)out,
                          cnt << L1, T.L, T.K);
  };
  switch (T.logn) {
    case 13: return rows(std::integral_constant<int, 1>{});
    case 14: return rows(std::integral_constant<int, 2>{});
    case 15: return rows(std::integral_constant<int, 3>{});
    case 16: return rows(std::integral_constant<int, 4>{});
    default: return hipErrorNotSupported;
  }
}

hipError_t launch_mdntt_rows(const MdTables &T, void *out, const void *x_hat, size_t cnt,
                             void *const *scr, hipStream_t s, std::string *describe) {
  if (!T.L || !T.K) return hipErrorInvalidValue;
  const Emit E{s, describe};
  return T.word_bits == 32 ? dispatch_rows<Arith32P, uint32_t>(T, out, x_hat, cnt, scr, E)
                           : dispatch_rows<Arith64, uint64_t>(T, out, x_hat, cnt, scr, E);
}

hipError_t launch_mdntt(const MdTables &T, void *out, const void *x_hat, size_t cnt,
                        void *const *scr, hipStream_t s) {
  return dispatch_words(T, out, x_hat, cnt, scr, Emit{s, nullptr});
}

hipError_t describe_mdntt(const MdTables &T, std::string *out) {
  out->clear();
  void *const scr[kMdScratch] = {nullptr, nullptr, nullptr};
  return dispatch_words(T, nullptr, nullptr, 1, scr, Emit{nullptr, out});
}

}  // namespace nttmul
