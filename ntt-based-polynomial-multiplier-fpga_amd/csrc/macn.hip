// macn.hip — launchers of the kernels of macn_dev.hpp.  The translation unit of the kernels
// lib/libnttmul_macn.so holds beyond libnttmul_ks.so's.  The column passes above n = 4096 are
// rnsmp.hip's own kernels, launched through launch_rnsmp_cols: no second copy of them here.
#include "macn.hpp"
#include "macn_dev.hpp"

namespace nttmul {

// one row of workgroups per limb (rns.hip / rnsmp.hip emit_limbs, 256 threads)
template <class... KArgs>
static hipError_t emit_limbs(const Emit &E, const std::string &name, void (*kernel)(KArgs...),
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

// "k_rns_macn<Arith32P,u32,12,2>", "k_rnsmp_macn<Arith64,u64,4,2>": the kernel's own template
// arguments, all of them
template <class A, class IO>
static std::string macn_name(const char *kernel, int size, int comps) {
  return std::string(kernel) + "<" + AName<A>::v + "," + word_name<IO>() + "," +
         std::to_string(size) + "," + std::to_string(comps) + ">";
}

// The class is k_rns_mac's: plain Arith32P at every n <= 4096 (a full transform has no base
// blocks), Arith64 on 64-bit words
template <class A, class IO, int COMPS>
static hipError_t rns_macn(const RnsTables &T, void *c, const void *a, const void *b, size_t batch,
                           uint32_t terms, int shared, const Emit &E) {
  return with_logn(T.logn, [&](auto logs) {
    constexpr int LOGS = decltype(logs)::value, PB = 256 / ((1 << LOGS) / 16);
    return emit_limbs(E, macn_name<A, IO>("k_rns_macn", LOGS, COMPS),
                      k_rns_macn<A, IO, LOGS, COMPS>, (batch + PB - 1) / PB, T.limbs,
                      (const KParams<A> *)T.tab[kRnsTransform],
                      (const TwPair<typename A::word> *)T.tw, (const IO *)a, (const IO *)b,
                      (IO *)c, batch, terms, shared ? 0u : COMPS * terms, T.limbs);
  });
}

static hipError_t rns_macn_words(const RnsTables &T, void *c, const void *a, const void *b,
                                 size_t batch, uint32_t terms, uint32_t comps, int shared,
                                 const Emit &E) {
  if (T.logn > 12 || comps != 2) return hipErrorNotSupported;
  return T.word_bits == 32 ? rns_macn<Arith32P, uint32_t, 2>(T, c, a, b, batch, terms, shared, E)
                           : rns_macn<Arith64, uint64_t, 2>(T, c, a, b, batch, terms, shared, E);
}

hipError_t launch_rns_macn(const RnsTables &T, void *c, const void *a, const void *b, size_t batch,
                           uint32_t terms, uint32_t comps, int shared, hipStream_t s,
                           const void *) {
  return rns_macn_words(T, c, a, b, batch, terms, comps, shared, Emit{s, nullptr});
}

hipError_t describe_rns_macn(const RnsTables &T, uint32_t comps, std::string *out) {
  out->clear();
  return rns_macn_words(T, nullptr, nullptr, nullptr, 1, 1, comps, 0, Emit{nullptr, out});
}

template <class A, class IO, int L1, int COMPS>
static hipError_t mp_rows(const RnsTables &T, const void *b, size_t batch, uint32_t terms,
                          int shared, void *const *scr, const Emit &E) {
  using W = typename A::word;
  return emit_limbs(E, macn_name<A, IO>("k_rnsmp_macn", L1, COMPS),
                    k_rnsmp_macn<A, IO, L1, COMPS>, batch << L1, T.limbs,
                    (const KParams<A> *)T.tab[kRnsTransform], (const TwPair<W> *)T.tw,
                    (const W *)scr[0], (const IO *)b, (W *)scr[2], batch << L1, terms,
                    shared ? 0u : COMPS * terms, T.limbs);
}

template <class A, class IO, int COMPS>
static hipError_t mp_rows_at(const RnsTables &T, const void *b, size_t batch, uint32_t terms,
                             int shared, void *const *scr, const Emit &E) {
  switch (T.logn) {
    case 13: return mp_rows<A, IO, 1, COMPS>(T, b, batch, terms, shared, scr, E);
    case 14: return mp_rows<A, IO, 2, COMPS>(T, b, batch, terms, shared, scr, E);
    case 15: return mp_rows<A, IO, 3, COMPS>(T, b, batch, terms, shared, scr, E);
    case 16: return mp_rows<A, IO, 4, COMPS>(T, b, batch, terms, shared, scr, E);
    default: return hipErrorNotSupported;
  }
}

static hipError_t mp_macn(const RnsTables &T, void *c, const void *a, const void *b, size_t batch,
                          uint32_t terms, uint32_t comps, int shared, void *const *scr,
                          const Emit &E) {
  if (comps != 2) return hipErrorNotSupported;
  hipError_t e = launch_rnsmp_cols(T, 0, scr[0], a, batch * terms, E.s, E.describe);
  if (e != hipSuccess) return e;
  e = T.word_bits == 32 ? mp_rows_at<Arith32P, uint32_t, 2>(T, b, batch, terms, shared, scr, E)
                        : mp_rows_at<Arith64, uint64_t, 2>(T, b, batch, terms, shared, scr, E);
  if (e != hipSuccess) return e;
  return launch_rnsmp_cols(T, 1, c, scr[2], batch * comps, E.s, E.describe);
}

hipError_t launch_rnsmp_macn(const RnsTables &T, void *c, const void *a, const void *b,
                             size_t batch, uint32_t terms, uint32_t comps, int shared,
                             void *const *scr, hipStream_t s) {
  return mp_macn(T, c, a, b, batch, terms, comps, shared, scr, Emit{s, nullptr});
}

hipError_t describe_rnsmp_macn(const RnsTables &T, uint32_t comps, std::string *out) {
  out->clear();
  void *const scr[3] = {nullptr, nullptr, nullptr};
  return mp_macn(T, nullptr, nullptr, nullptr, 1, 1, comps, 0, scr, Emit{nullptr, out});
}

}  // namespace nttmul
