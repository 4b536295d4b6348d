// kernels.hip — the library's launchers (the host side of include/nttmul.h's device calls): which
// kernel of kernels_dev.hpp runs for which (n, q, word size, batch), with what launch shape.
// This is the translation unit of libnttmul.so's kernels; the tools/kbench timing binaries
// include kernels_dev.hpp with launchers of their own and never compile this file.
#if defined(NTTMUL_HOOK_ROWS_LD) || defined(NTTMUL_HOOK_ROWS_ST) || defined(NTTMUL_HOOK_ROWS_INPUT) || \
    defined(NTTMUL_HOOK_ROWS_OUTPUT) || defined(NTTMUL_HOOK_XCHG) || defined(NTTMUL_HOOK_COLS_LD) || \
    defined(NTTMUL_HOOK_COLS_ST) || defined(NTTMUL_HOOK_TW) || defined(NTTMUL_HOOK_PRIO0)
#error "NTTMUL_HOOK_* are tools/kbench instrumentation points (wrong-result pricing builds), not library switches"
#endif
#include "kernels_dev.hpp"

namespace nttmul {

// The two selections every launcher below makes, each written once.  f is a generic lambda that
// receives the selected type as a Type<...> tag (type_of<decltype(tag)> names it).
template <class T> struct Type { using type = T; };
template <class Tag> using type_of = typename Tag::type;

// The arithmetic class of (word_bits, q): 64-bit storage of a q < 2^32 product keeps the 32-bit
// arithmetic
template <class F>
static hipError_t with_arith(const LaunchTables &T, F f) {
  if (T.word_bits == 32) {
    switch (a32_kind(T.q)) {
      case A32Kind::Wide: return f(Type<Arith32W>{});
      case A32Kind::Plantard: return f(Type<Arith32P>{});
    }
  }
  return f(Type<Arith64>{});
}

// The word type of the caller's buffers
template <class F>
static hipError_t with_io(int io_bits, F f) {
  return io_bits == 64 ? f(Type<uint64_t>{}) : f(Type<uint32_t>{});
}

// Multi-pass product, n = 2^logn in (4096, 65536]: rows of 4096, L1 = logn - 12 column stages.
template <class A, class IO, int L1, int LOGS = 12>
static hipError_t multipass_l1(const LaunchTables &T, const void *a, const void *b, void *c,
                               size_t batch, void **scr, const Emit &E) {
  using W = typename A::word;
  const KParams<A> P = product_params<A>(T);
  const size_t cblocks = ((batch << LOGS) + 255) / 256;
  const auto name = [](const char *kernel) {
    return [kernel] {
      return std::string(kernel) + "<" + AName<A>::v + "," + word_name<IO>() + "," +
             std::to_string(L1) + ">";
    };
  };
  hipError_t e = emit(E, name("k_cols_fwd"), k_cols_fwd<A, IO, L1>, cblocks, 256, P, (const IO *)a,
                      (const IO *)b, (W *)scr[0], (W *)scr[1], batch, LOGS);
  if (e != hipSuccess) return e;
  e = launch_rows<A, W, W, LOGS, L1>(T, scr[0], scr[1], scr[2], batch << L1, E);
  if (e != hipSuccess) return e;
  return emit(E, name("k_cols_inv"), k_cols_inv<A, IO, L1>, cblocks, 256, P, (const W *)scr[2],
              (IO *)c, batch, LOGS);
}

// Multi-pass product of the square split, n = 65536 = 256 x 256 (64-bit words, NTTMUL_C5_SQ):
// k_cols8 forward (global stages 0..7 of a and b), the row pass k_rows<..., 8, 8> (stages 8..15,
// base multiplication, inverse stages 15..8 of 256-coefficient rows), k_cols8 inverse.
template <class A, class IO>
static hipError_t multipass_sq(const LaunchTables &T, const void *a, const void *b, void *c,
                               size_t batch, void **scr, const Emit &E) {
  using W = typename A::word;
  const KParams<A> P = product_params<A>(T);
  const size_t groups = batch * 16;  // 16 workgroups of 16 columns per polynomial
  const auto name = [](const char *dir) {
    return [dir] {
      return std::string("k_cols8<") + AName<A>::v + "," + word_name<IO>() + "," + dir + ">";
    };
  };
  hipError_t e = emit(E, name("fwd"), k_cols8<A, IO, W, 0>, groups, 256, P, (const IO *)a,
                      (const IO *)b, (W *)scr[0], (W *)scr[1], groups);
  if (e != hipSuccess) return e;
  e = launch_rows<A, W, W, 8, 8>(T, scr[0], scr[1], scr[2], batch << 8, E);
  if (e != hipSuccess) return e;
  return emit(E, name("inv"), k_cols8<A, W, IO, 1>, groups, 256, P, (const W *)scr[2], nullptr,
              (IO *)c, nullptr, groups);
}

// c = a * b with arithmetic A on IO words: one fused launch up to n = 4096, else three passes
// through the scratch
template <class A, class IO>
static hipError_t product(const LaunchTables &T, const void *a, const void *b, void *c,
                          size_t batch, void **scr, const Emit &E) {
  if constexpr (std::is_same<A, Arith32P>::value) {  // D = 3 blocks at n = 4096 (Arith32P3)
    if (T.logn == 12 && p3_fold_ok(T.q))
      return launch_rows<Arith32P3, IO, IO, 12, 0>(T, a, b, c, batch, E);
  }
  if (T.logn <= 12)
    return with_logn(T.logn, [&](auto logs) {
      return launch_rows<A, IO, IO, decltype(logs)::value, 0>(T, a, b, c, batch, E);
    });
  if constexpr (sizeof(typename A::word) == 8 && NTTMUL_C5_SQ) {
    if (T.logn == 16) return multipass_sq<A, IO>(T, a, b, c, batch, scr, E);
  }
  switch (T.logn) {
    case 13: return multipass_l1<A, IO, 1>(T, a, b, c, batch, scr, E);
    case 14: return multipass_l1<A, IO, 2>(T, a, b, c, batch, scr, E);
    case 15: return multipass_l1<A, IO, 3>(T, a, b, c, batch, scr, E);
    case 16:
      if (NTTMUL_SPLIT16 == 5)  // 32 x 2048: one more stage in the (HBM-bound) column passes
        return multipass_l1<A, IO, 5, 11>(T, a, b, c, batch, scr, E);
      return multipass_l1<A, IO, 4>(T, a, b, c, batch, scr, E);
    default: return hipErrorInvalidValue;
  }
}

static hipError_t polymul(const LaunchTables &T, const void *a, const void *b, void *c,
                          size_t batch, int io_bits, void **scr, const Emit &E) {
  return with_arith(T, [&](auto ar) {
    return with_io(io_bits, [&](auto io) {
      return product<type_of<decltype(ar)>, type_of<decltype(io)>>(T, a, b, c, batch, scr, E);
    });
  });
}

hipError_t launch_polymul(const LaunchTables &T, const void *a, const void *b, void *c,
                          size_t batch, int io_bits, void **scr, hipStream_t s) {
  return polymul(T, a, b, c, batch, io_bits, scr, Emit{s, nullptr});
}

hipError_t describe_polymul(const LaunchTables &T, int io_bits, size_t batch, std::string *out) {
  out->clear();
  void *scr[3] = {nullptr, nullptr, nullptr};
  return polymul(T, nullptr, nullptr, nullptr, batch ? batch : (size_t)1 << 24, io_bits, scr,
                 Emit{nullptr, out});
}

hipError_t launch_server(const LaunchTables &T, const ServerReq *req, ServerBox *box,
                         unsigned long long idle_ticks, unsigned long long life_ticks,
                         hipStream_t s) {
  const size_t pairs = T.tw_bytes / sizeof(TwPair<uint32_t>);
  if (T.word_bits != 32 || a32_kind(T.q) != A32Kind::Plantard || T.logn < 8 || T.logn > 10 ||
      pairs > (1u << T.logn))
    return hipErrorNotSupported;
  const KParams<Arith32P> P = product_params<Arith32P>(T);
  const unsigned tp = (unsigned)pairs;
  switch (T.logn) {
    case 8: return launch(k_server<Arith32P, 8>, 1, 512, s, P, req, box, tp, idle_ticks, life_ticks);
    case 9: return launch(k_server<Arith32P, 9>, 1, 64, s, P, req, box, tp, idle_ticks, life_ticks);
    default: return launch(k_server<Arith32P, 10>, 1, 128, s, P, req, box, tp, idle_ticks, life_ticks);
  }
}

template <class A, class TIn, class TOut, int LOGS, int L1, int DIR>
static hipError_t launch_xform_rows(const KParams<A> &P, const void *in, void *out, size_t units,
                                    hipStream_t s) {
  constexpr int PB = 256 / ((1 << LOGS) / 16) * xform_upg<A, L1, DIR>();
  return launch(k_xform<A, TIn, TOut, LOGS, L1, DIR>, (units + PB - 1) / PB, 256, s, P,
                (const TIn *)in, (TOut *)out, units);
}

// KParams of a standalone transform; the inverse scales by n^-1 only (no Montgomery factor)
template <class A, int DIR>
static KParams<A> xform_params(const LaunchTables &T) {
  KParams<A> P = make_params<A>(T);
  if (DIR == 1) {
    P.f = (typename A::word)T.fi; P.fs = (typename A::word)T.fis;
    P.wf = (typename A::word)T.wfi; P.wfs = (typename A::word)T.wfis;
  }
  return P;
}

template <class A, class IO, int L1, int DIR>
static hipError_t xform_multipass_l1(const LaunchTables &T, const void *in, void *out,
                                     size_t batch, void **scr, hipStream_t s) {
  using W = typename A::word;
  constexpr int LOGS = 12;
  const KParams<A> P = xform_params<A, DIR>(T);
  const size_t cblocks = ((batch << LOGS) + 255) / 256;
  if (DIR == 0) {
    const hipError_t e = launch(k_cols_fwd<A, IO, L1, 1>, cblocks, 256, s, P, (const IO *)in,
                                nullptr, (W *)scr[0], nullptr, batch, LOGS);
    if (e != hipSuccess) return e;
    return launch_xform_rows<A, W, IO, LOGS, L1, 0>(P, scr[0], out, batch << L1, s);
  }
  const hipError_t e = launch_xform_rows<A, IO, W, LOGS, L1, 1>(P, in, scr[0], batch << L1, s);
  if (e != hipSuccess) return e;
  return launch(k_cols_inv<A, IO, L1>, cblocks, 256, s, P, (const W *)scr[0], (IO *)out, batch,
                LOGS);
}

// Standalone transforms of the square split (64-bit words at n = 65536, NTTMUL_C5_SQ, as the
// product): forward = k_cols8 on one polynomial (tiled scratch) + the 256-coefficient row pass
// (k_xform<..., 8, 8, 0>); inverse = the row pass into the tiled scratch + k_cols8 inverse.
template <class A, class IO, int DIR>
static hipError_t xform_sq(const LaunchTables &T, const void *in, void *out, size_t batch,
                           void **scr, hipStream_t s) {
  using W = typename A::word;
  const KParams<A> P = xform_params<A, DIR>(T);
  const size_t groups = batch * 16;
  if (DIR == 0) {
    const hipError_t e = launch(k_cols8<A, IO, W, 0, 1>, groups, 256, s, P, (const IO *)in,
                                nullptr, (W *)scr[0], nullptr, groups);
    if (e != hipSuccess) return e;
    return launch_xform_rows<A, W, IO, 8, 8, 0>(P, scr[0], out, batch << 8, s);
  }
  const hipError_t e = launch_xform_rows<A, IO, W, 8, 8, 1>(P, in, scr[0], batch << 8, s);
  if (e != hipSuccess) return e;
  return launch(k_cols8<A, W, IO, 1>, groups, 256, s, P, (const W *)scr[0], nullptr, (IO *)out,
                nullptr, groups);
}

template <class A, class IO, int DIR>
static hipError_t xform(const LaunchTables &T, const void *in, void *out, size_t batch,
                        void **scr, hipStream_t s) {
  if constexpr (sizeof(typename A::word) == 8 && NTTMUL_C5_SQ) {
    if (T.logn == 16) return xform_sq<A, IO, DIR>(T, in, out, batch, scr, s);
  }
  switch (T.logn) {
    case 13: return xform_multipass_l1<A, IO, 1, DIR>(T, in, out, batch, scr, s);
    case 14: return xform_multipass_l1<A, IO, 2, DIR>(T, in, out, batch, scr, s);
    case 15: return xform_multipass_l1<A, IO, 3, DIR>(T, in, out, batch, scr, s);
    case 16: return xform_multipass_l1<A, IO, 4, DIR>(T, in, out, batch, scr, s);
    default:  // one launch up to n = 4096
      return with_logn(T.logn, [&](auto logs) {
        return launch_xform_rows<A, IO, IO, decltype(logs)::value, 0, DIR>(
            xform_params<A, DIR>(T), in, out, batch, s);
      });
  }
}

template <int DIR>
static hipError_t xform_dir(const LaunchTables &T, const void *in, void *out, size_t batch,
                            int io_bits, void **scr, hipStream_t s) {
  return with_arith(T, [&](auto ar) {
    return with_io(io_bits, [&](auto io) {
      return xform<type_of<decltype(ar)>, type_of<decltype(io)>, DIR>(T, in, out, batch, scr, s);
    });
  });
}

hipError_t launch_xform(const LaunchTables &T, const void *in, void *out, size_t batch,
                        int io_bits, int inverse, void **scr, hipStream_t s) {
  return inverse ? xform_dir<1>(T, in, out, batch, io_bits, scr, s)
                 : xform_dir<0>(T, in, out, batch, io_bits, scr, s);
}

hipError_t launch_pointwise(const LaunchTables &T, const void *a, const void *b, void *c,
                            size_t batch, int io_bits, hipStream_t s) {
  const size_t total = batch << T.logn;
  return with_arith(T, [&](auto ar) {
    return with_io(io_bits, [&](auto io) {
      // Montgomery products only (no twiddle tables): Arith32 in Arith32P's place (q < 2^31)
      using A0 = type_of<decltype(ar)>;
      using A = std::conditional_t<std::is_same<A0, Arith32P>::value, Arith32, A0>;
      using IO = type_of<decltype(io)>;
      KParams<A> P = make_params<A>(T);
      P.f = (typename A::word)T.r2;
      return launch(k_pointwise<A, IO>, (total + 255) / 256, 256, s, P, (const IO *)a,
                    (const IO *)b, (IO *)c, total);
    });
  });
}

hipError_t launch_bitrev(const void *in, void *out, uint32_t logn, size_t batch, int io_bits,
                         hipStream_t s) {
  const size_t total = batch << logn, blocks = (total + 255) / 256;
  return with_io(io_bits, [&](auto io) {
    using W = type_of<decltype(io)>;
    return in == out ? launch(k_bitrev_inplace<W>, blocks, 256, s, (W *)out, logn, total)
                     : launch(k_bitrev<W>, blocks, 256, s, (const W *)in, (W *)out, logn, total);
  });
}

hipError_t launch_fill(void *a, void *b, uint32_t logn, uint64_t q, uint64_t seed, uint64_t p0,
                       size_t count, int io_bits, hipStream_t s) {
  const size_t total = count << logn;
  return with_io(io_bits, [&](auto io) {
    using W = type_of<decltype(io)>;
    return launch(k_fill<W>, (total + 255) / 256, 256, s, (W *)a, (W *)b, logn, q, seed, p0, total);
  });
}

hipError_t launch_check_range(const void *a, const void *b, uint64_t q, size_t total, int io_bits,
                              int *bad, hipStream_t s) {
  return with_io(io_bits, [&](auto io) {
    using W = type_of<decltype(io)>;
    return launch(k_check_range<W>, (total + 255) / 256, 256, s, (const W *)a, (const W *)b, q,
                  total, bad);
  });
}

}  // namespace nttmul
