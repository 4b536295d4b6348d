// mac.hip — launchers of the fused multiply-accumulate against NTT-domain operands (mac_dev.hpp
// k_mac).  The translation unit of the kernels lib/libnttmul_mac.so holds beyond libnttmul.so's.
#include "mac.hpp"
#include "mac_dev.hpp"

namespace nttmul {

// One kernel per (arithmetic class, caller word, n): the class follows (word_bits, q) as in
// kernels.hip with_arith, and at n = 4096 the Plantard class is plain Arith32P (Arith32P3 differs
// in its base blocks only, which a full transform does not have).  Arith64 takes u64 words only.
template <class A, class IO>
static hipError_t mac(const LaunchTables &T, const void *a, const void *bh, void *c, size_t batch,
                      uint32_t terms, int shared, const Emit &E) {
  return with_logn(T.logn, [&](auto logs) {
    constexpr int LOGS = decltype(logs)::value, PB = 256 / ((1 << LOGS) / 16);
    const auto name = [] {
      return std::string("k_mac<") + AName<A>::v + "," + word_name<IO>() + "," + word_name<IO>() +
             "," + std::to_string(LOGS) + ">";
    };
    return emit(E, name, k_mac<A, IO, IO, LOGS>, (batch + PB - 1) / PB, 256, make_params<A>(T),
                (const IO *)a, (const IO *)bh, (IO *)c, batch, terms, shared ? 0u : terms);
  });
}

static hipError_t mac_dispatch(const LaunchTables &T, const void *a, const void *bh, void *c,
                               size_t batch, uint32_t terms, int shared, int io_bits,
                               const Emit &E) {
  if (T.logn > 12) return hipErrorNotSupported;
  if (T.word_bits == 32) {
    if (a32_kind(T.q) == A32Kind::Wide)
      return io_bits == 64 ? mac<Arith32W, uint64_t>(T, a, bh, c, batch, terms, shared, E)
                           : mac<Arith32W, uint32_t>(T, a, bh, c, batch, terms, shared, E);
    return io_bits == 64 ? mac<Arith32P, uint64_t>(T, a, bh, c, batch, terms, shared, E)
                         : mac<Arith32P, uint32_t>(T, a, bh, c, batch, terms, shared, E);
  }
  if (io_bits != 64) return hipErrorInvalidValue;
  return mac<Arith64, uint64_t>(T, a, bh, c, batch, terms, shared, E);
}

hipError_t launch_mac(const LaunchTables &T, const void *a, const void *b_hat, void *c,
                      size_t batch, uint32_t terms, int shared, int io_bits, hipStream_t s) {
  return mac_dispatch(T, a, b_hat, c, batch, terms, shared, io_bits, Emit{s, nullptr});
}

hipError_t describe_mac(const LaunchTables &T, int io_bits, std::string *out) {
  out->clear();
  return mac_dispatch(T, nullptr, nullptr, nullptr, 1, 1, 0, io_bits, Emit{nullptr, out});
}

}  // namespace nttmul
