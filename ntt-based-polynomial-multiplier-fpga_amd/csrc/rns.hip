// rns.hip — launchers of the limb-aware kernels (rns_dev.hpp).  The translation unit of the
// kernels lib/libnttmul_rns.so holds beyond libnttmul_mac.so's.
#include "rns.hpp"
#include "rns_dev.hpp"

namespace nttmul {

// The arithmetic class of a table entry: by word size alone (an RNS context holds q < 2^31 limbs
// on 32-bit words or q >= 2^32 limbs on 64-bit words).  Arith32P3 is Arith32P with another base
// block, so one entry layout serves a word size.
static_assert(sizeof(KParams<Arith32P3>) == sizeof(KParams<Arith32P>), "one 32-bit entry layout");

size_t rns_entry_bytes(int word_bits) {
  return word_bits == 32 ? sizeof(KParams<Arith32P>) : sizeof(KParams<Arith64>);
}

template <class A>
static KParams<A> family_params(const LaunchTables &T, int fam) {
  using W = typename A::word;
  if (fam == kRnsProduct) return product_params<A>(T);
  KParams<A> P = make_params<A>(T);
  if (fam == kRnsInverse) {
    P.f = (W)T.fi; P.fs = (W)T.fis; P.wf = (W)T.wfi; P.wfs = (W)T.wfis;
  }
  return P;
}

hipError_t rns_fill_entry(const LaunchTables &T, int fam, void *dst) {
  if (fam < 0 || fam >= kRnsFamilies || T.logn < 8 || T.logn > 12) return hipErrorInvalidValue;
  if (T.word_bits == 64) {
    *(KParams<Arith64> *)dst = family_params<Arith64>(T, fam);
    return hipSuccess;
  }
  if (a32_kind(T.q) != A32Kind::Plantard) return hipErrorNotSupported;
  if (fam == kRnsProduct && T.logn == 12) {  // D = 3 blocks at n = 4096, as kernels.hip product
    if (!p3_fold_ok(T.q)) return hipErrorNotSupported;
    *(KParams<Arith32P3> *)dst = family_params<Arith32P3>(T, fam);
    return hipSuccess;
  }
  *(KParams<Arith32P> *)dst = family_params<Arith32P>(T, fam);
  return hipSuccess;
}

// emit (kernels_dev.hpp) on a two-dimensional grid: bx workgroups over the batch, one row of them
// per limb
template <class Name, class... KArgs>
static hipError_t emit_limbs(const Emit &E, Name name, void (*kernel)(KArgs...), size_t bx,
                             uint32_t limbs, int threads,
                             typename NoDeduce<KArgs>::type... args) {
  if (E.describe) {
    if (!E.describe->empty()) *E.describe += " + ";
    *E.describe += name();
    return hipSuccess;
  }
  if (bx == 0 || limbs == 0) return hipSuccess;
  if (bx > 0x7FFFFFFFull || limbs > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)bx, limbs), dim3(threads), 0, E.s, args...);
  return hipGetLastError();
}

template <class A, class IO>
static std::string rns_name(const char *kernel, int logs, int dir = -1) {
  return std::string(kernel) + "<" + AName<A>::v + "," + word_name<IO>() + "," +
         std::to_string(logs) + (dir < 0 ? "" : "," + std::to_string(dir)) + ">";
}

template <class A, class IO, int LOGS>
static hipError_t rows(const RnsTables &T, const void *a, const void *b, void *c, size_t batch,
                       const Emit &E) {
  constexpr int NT = rows_threads(LOGS), PB = NT / ((1 << LOGS) / 16);
  return emit_limbs(E, [] { return rns_name<A, IO>("k_rns_rows", LOGS); }, k_rns_rows<A, IO, LOGS>,
                    (batch + PB - 1) / PB, T.limbs, NT, (const KParams<A> *)T.tab[kRnsProduct],
                    (const TwPair<typename A::word> *)T.tw, (const IO *)a, (const IO *)b,
                    (IO *)c, batch, T.limbs);
}

template <class A, class IO, int LOGS, int DIR>
static hipError_t xform(const RnsTables &T, const void *in, void *out, size_t batch,
                        const Emit &E) {
  constexpr int PB = 256 / ((1 << LOGS) / 16) * xform_upg<A, 0, DIR>();
  return emit_limbs(E, [] { return rns_name<A, IO>("k_rns_xform", LOGS, DIR); },
                    k_rns_xform<A, IO, LOGS, DIR>, (batch + PB - 1) / PB, T.limbs, 256,
                    (const KParams<A> *)T.tab[DIR ? kRnsInverse : kRnsTransform],
                    (const TwPair<typename A::word> *)T.tw, (const IO *)in, (IO *)out, batch,
                    T.limbs);
}

template <class A, class IO, int LOGS>
static hipError_t mac(const RnsTables &T, const void *a, const void *bh, void *c, size_t batch,
                      uint32_t terms, int shared, const Emit &E) {
  constexpr int PB = 256 / ((1 << LOGS) / 16);
  return emit_limbs(E, [] { return rns_name<A, IO>("k_rns_mac", LOGS); }, k_rns_mac<A, IO, LOGS>,
                    (batch + PB - 1) / PB, T.limbs, 256,
                    (const KParams<A> *)T.tab[kRnsTransform],
                    (const TwPair<typename A::word> *)T.tw, (const IO *)a, (const IO *)bh,
                    (IO *)c, batch, terms, shared ? 0u : terms, T.limbs);
}

// One kernel per (class, n) and operation; the product at n = 4096 on 32-bit words is Arith32P3
// (no Arith32P rows kernel exists at that size), the transforms and the mac are plain Arith32P
// there: a full transform has no base blocks.
template <class A, class IO>
static hipError_t dispatch(const RnsTables &T, int op, void *c, const void *a, const void *b,
                           size_t batch, uint32_t terms, int shared, const Emit &E) {
  return with_logn(T.logn, [&](auto logs) {
    constexpr int LOGS = decltype(logs)::value;
    using AP = std::conditional_t<LOGS == 12 && std::is_same<A, Arith32P>::value, Arith32P3, A>;
    switch (op) {
      case kRnsMultiply: return rows<AP, IO, LOGS>(T, a, b, c, batch, E);
      case kRnsForward: return xform<A, IO, LOGS, 0>(T, a, c, batch, E);
      case kRnsInverseOp: return xform<A, IO, LOGS, 1>(T, a, c, batch, E);
      case kRnsMac: return mac<A, IO, LOGS>(T, a, b, c, batch, terms, shared, E);
      default: return hipErrorInvalidValue;
    }
  });
}

static hipError_t dispatch_words(const RnsTables &T, int op, void *c, const void *a, const void *b,
                                 size_t batch, uint32_t terms, int shared, const Emit &E) {
  if (T.logn > 12) return hipErrorNotSupported;
  return T.word_bits == 32
             ? dispatch<Arith32P, uint32_t>(T, op, c, a, b, batch, terms, shared, E)
             : dispatch<Arith64, uint64_t>(T, op, c, a, b, batch, terms, shared, E);
}

hipError_t launch_rns(const RnsTables &T, int op, void *c, const void *a, const void *b,
                      size_t batch, uint32_t terms, int shared, hipStream_t s) {
  return dispatch_words(T, op, c, a, b, batch, terms, shared, Emit{s, nullptr});
}

hipError_t describe_rns(const RnsTables &T, int op, std::string *out) {
  out->clear();
  return dispatch_words(T, op, nullptr, nullptr, nullptr, 1, 1, 0, Emit{nullptr, out});
}

hipError_t launch_rns_check(const RnsTables &T, const void *a, size_t total, int *bad,
                            hipStream_t s) {
  const size_t blocks = (total + 255) / 256;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  return T.word_bits == 32 ? launch(k_rns_check_range<uint32_t>, blocks, 256, s,
                                    (const uint32_t *)a, T.q, total, T.logn, T.limbs, bad)
                           : launch(k_rns_check_range<uint64_t>, blocks, 256, s,
                                    (const uint64_t *)a, T.q, total, T.logn, T.limbs, bad);
}

}  // namespace nttmul
