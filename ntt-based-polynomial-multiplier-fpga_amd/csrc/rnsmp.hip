// rnsmp.hip — launchers of the limb-aware multi-pass kernels (rnsmp_dev.hpp).  The translation
// unit of the kernels lib/libnttmul_rnsmp.so holds beyond libnttmul_bconv.so's.
#include "rnsmp.hpp"
#include "rnsmp_dev.hpp"

namespace nttmul {

template <class A>
static KParams<A> mp_family_params(const LaunchTables &T, int fam) {
  using W = typename A::word;
  if (fam == kRnsProduct) return product_params<A>(T);
  KParams<A> P = make_params<A>(T);
  if (fam == kRnsInverse) {
    P.f = (W)T.fi; P.fs = (W)T.fis; P.wf = (W)T.wfi; P.wfs = (W)T.wfis;
  }
  return P;
}

hipError_t rnsmp_fill_entry(const LaunchTables &T, int fam, void *dst) {
  if (fam < 0 || fam >= kRnsFamilies || T.logn < 13 || T.logn > 16) return hipErrorInvalidValue;
  if (T.word_bits == 64) {
    *(KParams<Arith64> *)dst = mp_family_params<Arith64>(T, fam);
    return hipSuccess;
  }
  if (a32_kind(T.q) != A32Kind::Plantard) return hipErrorNotSupported;
  *(KParams<Arith32P> *)dst = mp_family_params<Arith32P>(T, fam);
  return hipSuccess;
}

// emit (kernels_dev.hpp) on a two-dimensional grid: bx workgroups over the units, one row of them
// per limb
template <class Name, class... KArgs>
static hipError_t emit_limbs(const Emit &E, Name name, void (*kernel)(KArgs...), size_t bx,
                             uint32_t limbs, typename NoDeduce<KArgs>::type... args) {
  if (E.describe) {
    if (!E.describe->empty()) *E.describe += " + ";
    *E.describe += name();
    return hipSuccess;
  }
  if (bx == 0 || limbs == 0) return hipSuccess;
  if (bx > 0x7FFFFFFFull || limbs > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)bx, limbs), dim3(256), 0, E.s, args...);
  return hipGetLastError();
}

// "k_rnsmp_cols_fwd<Arith32P,u32,1,2>": the kernel's own template arguments, all of them
template <class A>
static std::string mp_name(const char *kernel, bool io, int l1, int last = -1) {
  return std::string(kernel) + "<" + AName<A>::v +
         (io ? std::string(",") + word_name<typename A::word>() : std::string()) + "," +
         std::to_string(l1) + (last < 0 ? "" : "," + std::to_string(last)) + ">";
}

template <class A, class IO, int L1, int NPOLY>
static hipError_t cols_fwd(const RnsTables &T, int fam, const void *a, const void *b, void *ta,
                           void *tb, size_t units, const Emit &E) {
  using W = typename A::word;
  return emit_limbs(E, [] { return mp_name<A>("k_rnsmp_cols_fwd", true, L1, NPOLY); },
                    k_rnsmp_cols_fwd<A, IO, L1, NPOLY>, ((units << kMpLogs) + 255) / 256, T.limbs,
                    (const KParams<A> *)T.tab[fam], (const TwPair<W> *)T.tw, (const IO *)a,
                    (const IO *)b, (W *)ta, (W *)tb, units, T.limbs, kMpLogs);
}

template <class A, class IO, int L1>
static hipError_t cols_inv(const RnsTables &T, int fam, const void *tc, void *c, size_t units,
                           const Emit &E) {
  using W = typename A::word;
  return emit_limbs(E, [] { return mp_name<A>("k_rnsmp_cols_inv", true, L1); },
                    k_rnsmp_cols_inv<A, IO, L1>, ((units << kMpLogs) + 255) / 256, T.limbs,
                    (const KParams<A> *)T.tab[fam], (const TwPair<W> *)T.tw, (const W *)tc,
                    (IO *)c, units, T.limbs, kMpLogs);
}

template <class A, class IO, int L1, int DIR>
static hipError_t xform_rows(const RnsTables &T, const void *in, void *out, size_t batch,
                             const Emit &E) {
  using W = typename A::word;
  return emit_limbs(E, [] { return mp_name<A>("k_rnsmp_xform", true, L1, DIR); },
                    k_rnsmp_xform<A, IO, L1, DIR>, batch << L1, T.limbs,
                    (const KParams<A> *)T.tab[DIR ? kRnsInverse : kRnsTransform],
                    (const TwPair<W> *)T.tw, (const IO *)in, (IO *)out, batch << L1, T.limbs);
}

// One split per (class, n): 2^L1 x 4096
template <class A, class IO, int L1>
static hipError_t passes(const RnsTables &T, int op, void *c, const void *a, const void *b,
                         size_t batch, uint32_t terms, int shared, void *const *scr,
                         const Emit &E) {
  using W = typename A::word;
  hipError_t e;
  switch (op) {
    case kRnsMultiply:
      e = cols_fwd<A, IO, L1, 2>(T, kRnsProduct, a, b, scr[0], scr[1], batch, E);
      if (e != hipSuccess) return e;
      e = emit_limbs(E, [] { return mp_name<A>("k_rnsmp_rows", false, L1); }, k_rnsmp_rows<A, L1>,
                     batch << L1, T.limbs, (const KParams<A> *)T.tab[kRnsProduct],
                     (const TwPair<W> *)T.tw, (const W *)scr[0], (const W *)scr[1], (W *)scr[2],
                     batch << L1, T.limbs);
      if (e != hipSuccess) return e;
      return cols_inv<A, IO, L1>(T, kRnsProduct, scr[2], c, batch, E);
    case kRnsForward:
      e = cols_fwd<A, IO, L1, 1>(T, kRnsTransform, a, nullptr, scr[0], nullptr, batch, E);
      if (e != hipSuccess) return e;
      return xform_rows<A, IO, L1, 0>(T, scr[0], c, batch, E);
    case kRnsInverseOp:
      e = xform_rows<A, IO, L1, 1>(T, a, scr[0], batch, E);
      if (e != hipSuccess) return e;
      return cols_inv<A, IO, L1>(T, kRnsInverse, scr[0], c, batch, E);
    case kRnsMac:
      e = cols_fwd<A, IO, L1, 1>(T, kRnsTransform, a, nullptr, scr[0], nullptr, batch * terms, E);
      if (e != hipSuccess) return e;
      e = emit_limbs(E, [] { return mp_name<A>("k_rnsmp_mac", true, L1); }, k_rnsmp_mac<A, IO, L1>,
                     batch << L1, T.limbs, (const KParams<A> *)T.tab[kRnsTransform],
                     (const TwPair<W> *)T.tw, (const W *)scr[0], (const IO *)b, (W *)scr[2],
                     batch << L1, terms, shared ? 0u : terms, T.limbs);
      if (e != hipSuccess) return e;
      return cols_inv<A, IO, L1>(T, kRnsTransform, scr[2], c, batch, E);
    default: return hipErrorInvalidValue;
  }
}

template <class A, class IO>
static hipError_t dispatch(const RnsTables &T, int op, void *c, const void *a, const void *b,
                           size_t batch, uint32_t terms, int shared, void *const *scr,
                           const Emit &E) {
  switch (T.logn) {
    case 13: return passes<A, IO, 1>(T, op, c, a, b, batch, terms, shared, scr, E);
    case 14: return passes<A, IO, 2>(T, op, c, a, b, batch, terms, shared, scr, E);
    case 15: return passes<A, IO, 3>(T, op, c, a, b, batch, terms, shared, scr, E);
    case 16: return passes<A, IO, 4>(T, op, c, a, b, batch, terms, shared, scr, E);
    default: return hipErrorNotSupported;
  }
}

static hipError_t dispatch_words(const RnsTables &T, int op, void *c, const void *a, const void *b,
                                 size_t batch, uint32_t terms, int shared, void *const *scr,
                                 const Emit &E) {
  return T.word_bits == 32
             ? dispatch<Arith32P, uint32_t>(T, op, c, a, b, batch, terms, shared, scr, E)
             : dispatch<Arith64, uint64_t>(T, op, c, a, b, batch, terms, shared, scr, E);
}

template <class A, class IO>
static hipError_t cols_only(const RnsTables &T, int dir, void *out, const void *in, size_t units,
                            const Emit &E) {
  const auto go = [&](auto l1) {
    constexpr int L1 = decltype(l1)::value;
    return dir ? cols_inv<A, IO, L1>(T, kRnsTransform, in, out, units, E)
               : cols_fwd<A, IO, L1, 1>(T, kRnsTransform, in, nullptr, out, nullptr, units, E);
  };
  switch (T.logn) {
    case 13: return go(std::integral_constant<int, 1>{});
    case 14: return go(std::integral_constant<int, 2>{});
    case 15: return go(std::integral_constant<int, 3>{});
    case 16: return go(std::integral_constant<int, 4>{});
    default: return hipErrorNotSupported;
  }
}

hipError_t launch_rnsmp_cols(const RnsTables &T, int dir, void *out, const void *in, size_t units,
                             hipStream_t s, std::string *describe) {
  const Emit E{s, describe};
  return T.word_bits == 32 ? cols_only<Arith32P, uint32_t>(T, dir, out, in, units, E)
                           : cols_only<Arith64, uint64_t>(T, dir, out, in, units, E);
}

hipError_t launch_rnsmp(const RnsTables &T, int op, void *c, const void *a, const void *b,
                        size_t batch, uint32_t terms, int shared, void *const *scr, hipStream_t s) {
  return dispatch_words(T, op, c, a, b, batch, terms, shared, scr, Emit{s, nullptr});
}

hipError_t describe_rnsmp(const RnsTables &T, int op, std::string *out) {
  out->clear();
  void *const scr[3] = {nullptr, nullptr, nullptr};
  return dispatch_words(T, op, nullptr, nullptr, nullptr, 1, 1, 0, scr, Emit{nullptr, out});
}

}  // namespace nttmul
