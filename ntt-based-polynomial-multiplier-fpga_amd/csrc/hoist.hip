// hoist.hip — launchers of the kernels of hoist_dev.hpp.  The translation unit of the kernels
// lib/libnttmul_hoist.so holds beyond libnttmul_macn.so's.  The column pass above n = 4096 is
// rnsmp.hip's own kernel, launched through launch_rnsmp_cols: no second copy of it here.
#include "hoist.hpp"
#include "hoist_dev.hpp"

namespace nttmul {

// one row of workgroups per limb (rns.hip / rnsmp.hip / macn.hip emit_limbs, 256 threads)
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

// "k_rns_hoist<Arith32P,u32,12,2>", "k_rnsmp_hoist<Arith64,u64,4,1>": the kernel's own template
// arguments, all of them
template <class A, class IO>
static std::string hoist_name(const char *kernel, int size, int comps) {
  return std::string(kernel) + "<" + AName<A>::v + "," + word_name<IO>() + "," +
         std::to_string(size) + "," + std::to_string(comps) + ">";
}

// The class is k_rns_mac's: plain Arith32P at every n <= 4096, Arith64 on 64-bit words
template <class A, class IO, int COMPS>
static hipError_t rns_hoist(const RnsTables &T, void *c, const void *a, const void *b,
                            size_t batch, uint32_t terms, const HoistArgs &H, const Emit &E) {
  return with_logn(T.logn, [&](auto logs) {
    constexpr int LOGS = decltype(logs)::value, PB = 256 / ((1 << LOGS) / 16);
    return emit_limbs(E, hoist_name<A, IO>("k_rns_hoist", LOGS, COMPS),
                      k_rns_hoist<A, IO, LOGS, COMPS>, (batch + PB - 1) / PB * H.rots, T.limbs,
                      (const KParams<A> *)T.tab[kRnsTransform],
                      (const TwPair<typename A::word> *)T.tw, (const IO *)a, (const IO *)b,
                      (IO *)c, H.ks, H.rots, batch, terms, T.limbs);
  });
}

template <class A, class IO>
static hipError_t rns_hoist_comps(const RnsTables &T, void *c, const void *a, const void *b,
                                  size_t batch, uint32_t terms, const HoistArgs &H,
                                  const Emit &E) {
  switch (H.comps) {
    case 1: return rns_hoist<A, IO, 1>(T, c, a, b, batch, terms, H, E);
    case 2: return rns_hoist<A, IO, 2>(T, c, a, b, batch, terms, H, E);
    default: return hipErrorNotSupported;
  }
}

static hipError_t rns_hoist_words(const RnsTables &T, void *c, const void *a, const void *b,
                                  size_t batch, uint32_t terms, const HoistArgs &H,
                                  const Emit &E) {
  if (T.logn > 12 || !H.rots || H.rots > kGaloisMaxCount) return hipErrorNotSupported;
  return T.word_bits == 32 ? rns_hoist_comps<Arith32P, uint32_t>(T, c, a, b, batch, terms, H, E)
                           : rns_hoist_comps<Arith64, uint64_t>(T, c, a, b, batch, terms, H, E);
}

hipError_t launch_rns_hoist(const RnsTables &T, void *c, const void *a, const void *b,
                            size_t batch, uint32_t terms, uint32_t comps_all, int shared,
                            hipStream_t s, const void *aux) {
  const HoistArgs &H = *(const HoistArgs *)aux;
  if (!shared || comps_all != H.rots * H.comps) return hipErrorInvalidValue;
  return rns_hoist_words(T, c, a, b, batch, terms, H, Emit{s, nullptr});
}

static HoistArgs dry_args(uint32_t comps) {
  HoistArgs H;
  for (uint32_t &k : H.ks.k) k = 1;
  H.rots = 1;
  H.comps = comps;
  return H;
}

hipError_t describe_rns_hoist(const RnsTables &T, uint32_t comps, std::string *out) {
  out->clear();
  return rns_hoist_words(T, nullptr, nullptr, nullptr, 1, 1, dry_args(comps), Emit{nullptr, out});
}

template <class A, class IO, int L1, int COMPS>
static hipError_t mp_rows(const RnsTables &T, const void *a, const void *b, size_t u0, size_t cnt,
                          uint32_t terms, const HoistArgs &H, void *const *scr, const Emit &E) {
  using W = typename A::word;
  return emit_limbs(E, hoist_name<A, IO>("k_rnsmp_hoist", L1, COMPS),
                    k_rnsmp_hoist<A, IO, L1, COMPS>, cnt << L1, T.limbs,
                    (const KParams<A> *)T.tab[kRnsTransform], (const TwPair<W> *)T.tw,
                    (const IO *)a, (const IO *)b, (W *)scr[2], H.ks, H.rots, u0, cnt << L1, terms,
                    T.limbs);
}

template <class A, class IO, int COMPS>
static hipError_t mp_rows_at(const RnsTables &T, const void *a, const void *b, size_t u0,
                             size_t cnt, uint32_t terms, const HoistArgs &H, void *const *scr,
                             const Emit &E) {
  switch (T.logn) {
    case 13: return mp_rows<A, IO, 1, COMPS>(T, a, b, u0, cnt, terms, H, scr, E);
    case 14: return mp_rows<A, IO, 2, COMPS>(T, a, b, u0, cnt, terms, H, scr, E);
    case 15: return mp_rows<A, IO, 3, COMPS>(T, a, b, u0, cnt, terms, H, scr, E);
    case 16: return mp_rows<A, IO, 4, COMPS>(T, a, b, u0, cnt, terms, H, scr, E);
    default: return hipErrorNotSupported;
  }
}

template <class A, class IO>
static hipError_t mp_rows_comps(const RnsTables &T, const void *a, const void *b, size_t u0,
                                size_t cnt, uint32_t terms, const HoistArgs &H, void *const *scr,
                                const Emit &E) {
  switch (H.comps) {
    case 1: return mp_rows_at<A, IO, 1>(T, a, b, u0, cnt, terms, H, scr, E);
    case 2: return mp_rows_at<A, IO, 2>(T, a, b, u0, cnt, terms, H, scr, E);
    default: return hipErrorNotSupported;
  }
}

static hipError_t mp_hoist(const RnsTables &T, void *c, const void *a, const void *b, size_t u0,
                           size_t cnt, uint32_t terms, const HoistArgs &H, void *const *scr,
                           const Emit &E) {
  if (!H.rots || H.rots > kGaloisMaxCount) return hipErrorNotSupported;
  const hipError_t e =
      T.word_bits == 32 ? mp_rows_comps<Arith32P, uint32_t>(T, a, b, u0, cnt, terms, H, scr, E)
                        : mp_rows_comps<Arith64, uint64_t>(T, a, b, u0, cnt, terms, H, scr, E);
  if (e != hipSuccess) return e;
  return launch_rnsmp_cols(T, 1, c, scr[2], cnt * H.comps, E.s, E.describe);
}

hipError_t launch_rnsmp_hoist(const RnsTables &T, void *c, const void *a, const void *b, size_t u0,
                              size_t cnt, uint32_t terms, const void *aux, void *const *scr,
                              hipStream_t s) {
  return mp_hoist(T, c, a, b, u0, cnt, terms, *(const HoistArgs *)aux, scr, Emit{s, nullptr});
}

hipError_t describe_rnsmp_hoist(const RnsTables &T, uint32_t comps, std::string *out) {
  out->clear();
  void *const scr[3] = {nullptr, nullptr, nullptr};
  return mp_hoist(T, nullptr, nullptr, nullptr, 0, 1, 1, dry_args(comps), scr,
                  Emit{nullptr, out});
}

}  // namespace nttmul
