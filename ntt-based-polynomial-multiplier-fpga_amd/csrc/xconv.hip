// xconv.hip — launchers of the kernels of xconv_dev.hpp.  The translation unit of the kernels
// lib/libnttmul_xconv.so holds beyond libnttmul_ctmul.so's.  The inverse half and moddown's row
// pass above n = 4096 are mdntt.hip's own kernels, launched through launch_mdntt_inverse and
// launch_mdntt_rows on a view of this context's tables: no second copy of them here.
#include "xconv.hpp"
#include "xconv_dev.hpp"

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

// "k_xconv_fwd<Arith32P,u32,12,1>", "k_xconv_rows<Arith64,u64,4>": the kernel's own template
// arguments, all of them
template <class A, class IO>
static std::string xc_name(const char *kernel, int size, int op = -1) {
  return std::string(kernel) + "<" + AName<A>::v + "," + word_name<IO>() + "," +
         std::to_string(size) + (op < 0 ? "" : "," + std::to_string(op)) + ">";
}

// mdntt.hip's view of this context: extend's inverse reads a compact [cnt][K][n] operand (L = 0)
static MdTables md_view(const XcTables &T, int op, bool inverse) {
  MdTables V;
  V.logn = T.logn;
  V.L = inverse && op == kXcExtend ? 0 : T.L;
  V.K = T.K;
  V.word_bits = T.word_bits;
  V.tab_fwd = T.tab_fwd;
  V.tab_inv = T.tab_inv;
  // launch_mdntt_inverse finds P's twiddles L limbs into tw
  V.tw = inverse && op == kXcExtend
             ? (const char *)T.tw + ((((size_t)T.L * 2) << T.logn) * 2 * (T.word_bits / 8))
             : T.tw;
  V.to = T.to;
  V.w = T.w[op];
  return V;
}

// n <= 4096: the class is k_rns_xform's, plain Arith32P at every degree, Arith64 on 64-bit words
template <class A, class IO, int OP>
static hipError_t single(const XcTables &T, void *out, const void *in, size_t cnt,
                         void *const *scr, const Emit &E) {
  using W = typename A::word;
  return with_logn(T.logn, [&](auto logs) {
    constexpr int LOGS = decltype(logs)::value, PB = 256 / ((1 << LOGS) / 16);
    return emit_q_fastest(E, xc_name<A, IO>("k_xconv_fwd", LOGS, OP), k_xconv_fwd<A, IO, LOGS, OP>,
                          (cnt + PB - 1) / PB, T.L, (const KParams<A> *)T.tab_fwd,
                          (const TwPair<W> *)T.tw, (const BconvTo<W> *)T.to, (const W *)T.w[OP],
                          T.ip, (const W *)scr[kMdY], (const IO *)(OP == kXcModdown ? in : nullptr),
                          (IO *)out, cnt, T.L, T.K);
  });
}

// n > 4096: one split per (class, n), 2^L1 x 4096
template <class A, class IO, int L1>
static hipError_t passes(const XcTables &T, int op, void *out, const void *in, size_t cnt,
                         void *const *scr, const Emit &E) {
  using W = typename A::word;
  const hipError_t e =
      emit_q_fastest(E, xc_name<A, IO>("k_xconv_cols_fwd", L1), k_xconv_cols_fwd<A, IO, L1>,
                     ((cnt << kMpLogs) + 255) / 256, T.L, (const KParams<A> *)T.tab_fwd,
                     (const TwPair<W> *)T.tw, (const BconvTo<W> *)T.to, (const W *)T.w[op], T.ip,
                     (const W *)scr[kMdY], (W *)scr[kMdT], cnt, T.L, T.K);
  if (e != hipSuccess) return e;
  if (op == kXcModdown)
    return launch_mdntt_rows(md_view(T, op, false), out, in, cnt, scr, E.s, E.describe);
  return emit_q_fastest(E, xc_name<A, IO>("k_xconv_rows", L1), k_xconv_rows<A, IO, L1>, cnt << L1,
                        T.L, (const KParams<A> *)T.tab_fwd, (const TwPair<W> *)T.tw,
                        (const W *)scr[kMdT], (IO *)out, cnt << L1, T.L);
}

template <class A, class IO>
static hipError_t dispatch(const XcTables &T, int op, void *out, const void *in, size_t cnt,
                           void *const *scr, const Emit &E) {
  const hipError_t e =
      launch_mdntt_inverse(md_view(T, op, true), in, cnt, scr, E.s, E.describe);
  if (e != hipSuccess) return e;
  switch (T.logn) {
    case 13: return passes<A, IO, 1>(T, op, out, in, cnt, scr, E);
    case 14: return passes<A, IO, 2>(T, op, out, in, cnt, scr, E);
    case 15: return passes<A, IO, 3>(T, op, out, in, cnt, scr, E);
    case 16: return passes<A, IO, 4>(T, op, out, in, cnt, scr, E);
    default:
      if (T.logn > 12) return hipErrorNotSupported;
      return op == kXcModdown ? single<A, IO, kXcModdown>(T, out, in, cnt, scr, E)
                              : single<A, IO, kXcExtend>(T, out, in, cnt, scr, E);
  }
}

static hipError_t dispatch_words(const XcTables &T, int op, void *out, const void *in, size_t cnt,
                                 void *const *scr, const Emit &E) {
  if (!T.L || !T.K || (op != kXcExtend && op != kXcModdown)) return hipErrorInvalidValue;
  return T.word_bits == 32 ? dispatch<Arith32P, uint32_t>(T, op, out, in, cnt, scr, E)
                           : dispatch<Arith64, uint64_t>(T, op, out, in, cnt, scr, E);
}

hipError_t launch_xconv(const XcTables &T, int op, void *out, const void *in, size_t cnt,
                        void *const *scr, hipStream_t s) {
  return dispatch_words(T, op, out, in, cnt, scr, Emit{s, nullptr});
}

hipError_t describe_xconv(const XcTables &T, int op, std::string *out) {
  out->clear();
  void *const scr[kMdScratch] = {nullptr, nullptr, nullptr};
  return dispatch_words(T, op, nullptr, nullptr, 1, scr, Emit{nullptr, out});
}

}  // namespace nttmul
