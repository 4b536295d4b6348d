// arith_probe.hip — lib/libnttmul_probe.so: the device primitives of csrc/modarith.hpp and the
// mac_add overloads of csrc/mac_dev.hpp, one at a time, on operands the caller chooses.
//
// Test-only (tests/test_gpu_arith_probe.py, tests/arith_contracts.py); nothing here is part of
// libnttmul*.so.  Each op is an element-wise kernel: thread i reads operand tuple i from plain
// arrays, calls one primitive in one of the template instantiations the kernels use, and stores
// its outputs.  No index depends on data, so a wrong primitive can only produce wrong numbers.
//
// The arithmetic constants come from the library's own host code: make_plan(256, q, 0) and
// make_params<A>, exactly as a launch of the product kernels fills them.  probe_tables exports
// that plan's twiddle pair tables (with the signed-form typing of p_signed_fw_entry) and
// probe_consts its scale pairs, so the tests multiply by the pairs the kernels really load.
//
// Operands and results cross the ABI as uint64_t words whatever the class's word, operand k of
// tuple i at in[k * count + i]; a 32-bit class reads the low word.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "mac_dev.hpp"
#include "nttmul.h"
#include "planner.hpp"

using namespace nttmul;

namespace {

template <class Op>
__global__ __launch_bounds__(256) void k_probe(typename Op::A ar, const uint64_t *__restrict__ in,
                                               uint64_t *__restrict__ out, uint32_t count) {
  using W = typename Op::A::word;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  W x[Op::NIN], y[Op::NOUT];
#pragma unroll
  for (int k = 0; k < Op::NIN; k++) x[k] = (W)in[(size_t)k * count + i];
  Op::run(ar, x, y);
#pragma unroll
  for (int k = 0; k < Op::NOUT; k++) out[(size_t)k * count + i] = y[k];
}

// the modulus range a class serves (kernels.hip with_arith): 0: q < 2^31, 1: 2^31 <= q < 2^32,
// 2: 2^32 <= q < 2^62 (the plan's -q^-1 is mod 2^64 only there)
template <class A>
constexpr int range_of() {
  return std::is_same<A, Arith64>::value ? 2 : std::is_same<A, Arith32W>::value ? 1 : 0;
}

struct Entry {
  const char *name;
  int nin, nout, bits, range;
  hipError_t (*run)(const LaunchTables &, const uint64_t *, uint64_t *, uint32_t);
};

std::vector<Entry> &registry() {
  static std::vector<Entry> r;
  return r;
}

template <class Op>
hipError_t run_op(const LaunchTables &T, const uint64_t *in, uint64_t *out, uint32_t count) {
  const KParams<typename Op::A> P = make_params<typename Op::A>(T);
  k_probe<Op><<<(count + 255) / 256, 256>>>(P.ar, in, out, count);
  return hipGetLastError();
}

template <class Op>
struct Reg {
  Reg() {
    using A = typename Op::A;
    registry().push_back({Op::kName, Op::NIN, Op::NOUT, (int)sizeof(typename A::word) * 8,
                          range_of<A>(), run_op<Op>});
  }
};

#define OP(ID, CLS, NAME, NI, NO, ...)                                              \
  struct ID {                                                                       \
    using A = CLS;                                                                  \
    using W = CLS::word;                                                            \
    static constexpr int NIN = NI, NOUT = NO;                                       \
    static constexpr const char *kName = NAME;                                      \
    __device__ static __forceinline__ void run(const A &ar, const W *x, W *y) {     \
      __VA_ARGS__                                                                   \
    }                                                                               \
  };                                                                                \
  static Reg<ID> reg_##ID;

// (X, Y, pair) -> (X', Y')
#define BFLY(CALL)        \
  W X = x[0], Y = x[1];   \
  CALL(X, Y, x[2], x[3]); \
  y[0] = X, y[1] = Y;
#define BFLY_SCALED(CALL)             \
  W X = x[0], Y = x[1];               \
  CALL(X, Y, x[2], x[3], x[4], x[5]); \
  y[0] = X, y[1] = Y;
// (a[B], b[B], pair) -> a[B]
#define BASE(B, CALL)                                           \
  W a[B], b[B];                                                 \
  _Pragma("unroll") for (int i = 0; i < B; i++) a[i] = x[i], b[i] = x[B + i]; \
  CALL;                                                         \
  _Pragma("unroll") for (int i = 0; i < B; i++) y[i] = a[i];

// ---- Arith32 -----------------------------------------------------------------------------------
OP(A32_csub, Arith32, "Arith32.csub", 2, 1, y[0] = A::csub(x[0], x[1]);)
OP(A32_mont, Arith32, "Arith32.mont", 2, 1, y[0] = ar.mont(x[0], x[1]);)
OP(A32_canon, Arith32, "Arith32.canon", 1, 1, y[0] = ar.canon(x[0]);)
OP(A32_canon_inv, Arith32, "Arith32.canon_inv", 1, 1, y[0] = ar.canon_inv(x[0]);)

// ---- Arith32P ----------------------------------------------------------------------------------
OP(P_csub, Arith32P, "Arith32P.csub", 2, 1, y[0] = A::csub(x[0], x[1]);)
OP(P_cadd, Arith32P, "Arith32P.cadd", 1, 1, y[0] = ar.cadd(x[0]);)
OP(P_pmul, Arith32P, "Arith32P.pmul", 3, 1, y[0] = ar.pmul(x[0], x[1], x[2]);)
OP(P_pmul_s, Arith32P, "Arith32P.pmul_s", 3, 1, y[0] = ar.pmul_s(x[0], x[1], x[2]);)
OP(P_shoup, Arith32P, "Arith32P.shoup", 3, 1, y[0] = ar.shoup(x[0], x[1], x[2]);)
OP(P_pmul_diff, Arith32P, "Arith32P.pmul_diff", 4, 1,
   y[0] = ar.pmul_diff(x[0], x[1], x[2], x[3]);)
// ct<XC, XN, YN>: the six combinations kernels_dev.hpp instantiates (T = true, F = false)
OP(P_ct_TFF, Arith32P, "Arith32P.ct<T,F,F>", 4, 2, BFLY((ar.ct<true, false, false>)))
OP(P_ct_TFT, Arith32P, "Arith32P.ct<T,F,T>", 4, 2, BFLY((ar.ct<true, false, true>)))
OP(P_ct_FFF, Arith32P, "Arith32P.ct<F,F,F>", 4, 2, BFLY((ar.ct<false, false, false>)))
OP(P_ct_FFT, Arith32P, "Arith32P.ct<F,F,T>", 4, 2, BFLY((ar.ct<false, false, true>)))
OP(P_ct_FTF, Arith32P, "Arith32P.ct<F,T,F>", 4, 2, BFLY((ar.ct<false, true, false>)))
OP(P_ct_FTT, Arith32P, "Arith32P.ct<F,T,T>", 4, 2, BFLY((ar.ct<false, true, true>)))
OP(P_gs, Arith32P, "Arith32P.gs", 4, 2, BFLY(ar.gs))
OP(P_gs_scaled, Arith32P, "Arith32P.gs_scaled", 6, 2, BFLY_SCALED(ar.gs_scaled))
OP(P_mont, Arith32P, "Arith32P.mont", 2, 1, y[0] = ar.mont(x[0], x[1]);)
OP(P_canon, Arith32P, "Arith32P.canon", 1, 1, y[0] = ar.canon(x[0]);)
OP(P_canon_inv, Arith32P, "Arith32P.canon_inv", 1, 1, y[0] = ar.canon_inv(x[0]);)
// basemul<4, NEG, ZC>
OP(P_base_FF, Arith32P, "Arith32P.basemul<4,F,F>", 10, 4,
   BASE(4, (ar.basemul<4, false, false>(a, b, x[8], x[9]))))
OP(P_base_FT, Arith32P, "Arith32P.basemul<4,F,T>", 10, 4,
   BASE(4, (ar.basemul<4, false, true>(a, b, x[8], x[9]))))
OP(P_base_TF, Arith32P, "Arith32P.basemul<4,T,F>", 10, 4,
   BASE(4, (ar.basemul<4, true, false>(a, b, x[8], x[9]))))
OP(P_base_TT, Arith32P, "Arith32P.basemul<4,T,T>", 10, 4,
   BASE(4, (ar.basemul<4, true, true>(a, b, x[8], x[9]))))
OP(P_lane_F, Arith32P, "Arith32P.basemul4_lane<F>", 10, 4,
   BASE(4, ar.basemul4_lane(a, b, x[8], x[9], false)))
OP(P_lane_T, Arith32P, "Arith32P.basemul4_lane<T>", 10, 4,
   BASE(4, ar.basemul4_lane(a, b, x[8], x[9], true)))

// ---- Arith32P3 ---------------------------------------------------------------------------------
OP(P3_base_FF, Arith32P3, "Arith32P3.basemul<8,F,F>", 18, 8,
   BASE(8, (ar.basemul<8, false, false>(a, b, x[16], x[17]))))
OP(P3_base_FT, Arith32P3, "Arith32P3.basemul<8,F,T>", 18, 8,
   BASE(8, (ar.basemul<8, false, true>(a, b, x[16], x[17]))))
OP(P3_base_TF, Arith32P3, "Arith32P3.basemul<8,T,F>", 18, 8,
   BASE(8, (ar.basemul<8, true, false>(a, b, x[16], x[17]))))
OP(P3_base_TT, Arith32P3, "Arith32P3.basemul<8,T,T>", 18, 8,
   BASE(8, (ar.basemul<8, true, true>(a, b, x[16], x[17]))))

// ---- Arith32W ----------------------------------------------------------------------------------
OP(W_addmod, Arith32W, "Arith32W.addmod", 2, 1, y[0] = ar.addmod(x[0], x[1]);)
OP(W_submod, Arith32W, "Arith32W.submod", 2, 1, y[0] = ar.submod(x[0], x[1]);)
OP(W_shoup, Arith32W, "Arith32W.shoup", 3, 1, y[0] = ar.shoup(x[0], x[1], x[2]);)
OP(W_mont, Arith32W, "Arith32W.mont", 2, 1, y[0] = ar.mont(x[0], x[1]);)
OP(W_ct, Arith32W, "Arith32W.ct", 4, 2, BFLY(ar.ct))
OP(W_gs, Arith32W, "Arith32W.gs", 4, 2, BFLY(ar.gs))
OP(W_gs_scaled, Arith32W, "Arith32W.gs_scaled", 6, 2, BFLY_SCALED(ar.gs_scaled))
OP(W_canon, Arith32W, "Arith32W.canon", 1, 1, y[0] = ar.canon(x[0]);)
OP(W_canon_inv, Arith32W, "Arith32W.canon_inv", 1, 1, y[0] = ar.canon_inv(x[0]);)

// ---- Arith64 -----------------------------------------------------------------------------------
OP(L_csub, Arith64, "Arith64.csub", 2, 1, y[0] = A::csub(x[0], x[1]);)
OP(L_mulhi_F, Arith64, "Arith64.mulhi64<F>", 2, 1, y[0] = A::mulhi64<false>(x[0], x[1]);)
OP(L_mulhi_T, Arith64, "Arith64.mulhi64<T>", 2, 1, y[0] = A::mulhi64<true>(x[0], x[1]);)
OP(L_mullo, Arith64, "Arith64.mullo64", 2, 1, y[0] = A::mullo64(x[0], x[1]);)
// shoup<MADC>(x, w, w', acc)
OP(L_shoup_T, Arith64, "Arith64.shoup<T>", 4, 1, y[0] = ar.shoup<true>(x[0], x[1], x[2], x[3]);)
OP(L_shoup_F, Arith64, "Arith64.shoup<F>", 4, 1, y[0] = ar.shoup<false>(x[0], x[1], x[2], x[3]);)
OP(L_ct_F, Arith64, "Arith64.ct<F>", 4, 2, BFLY(ar.ct<false>))
OP(L_ct_T, Arith64, "Arith64.ct<T>", 4, 2, BFLY(ar.ct<true>))
OP(L_gs, Arith64, "Arith64.gs", 4, 2, BFLY(ar.gs))
OP(L_gs_scaled, Arith64, "Arith64.gs_scaled", 6, 2, BFLY_SCALED(ar.gs_scaled))
OP(L_canon, Arith64, "Arith64.canon", 1, 1, y[0] = ar.canon(x[0]);)
OP(L_canon_inv, Arith64, "Arith64.canon_inv", 1, 1, y[0] = ar.canon_inv(x[0]);)
OP(L_mont, Arith64, "Arith64.mont", 2, 1, y[0] = ar.mont(x[0], x[1]);)
OP(L_base_F, Arith64, "Arith64.basemul<4,F>", 10, 4,
   BASE(4, (ar.basemul<4, false>(a, b, x[8], x[9]))))
OP(L_base_T, Arith64, "Arith64.basemul<4,T>", 10, 4,
   BASE(4, (ar.basemul<4, true>(a, b, x[8], x[9]))))

// ---- mac_dev.hpp -------------------------------------------------------------------------------
OP(M_P, Arith32P, "mac_add.Arith32P", 2, 1, y[0] = mac_add(ar, x[0], x[1]);)
OP(M_W, Arith32W, "mac_add.Arith32W", 2, 1, y[0] = mac_add(ar, x[0], x[1]);)
OP(M_L, Arith64, "mac_add.Arith64", 2, 1, y[0] = mac_add(ar, x[0], x[1]);)

const Entry *find(const char *op) {
  for (const Entry &e : registry())
    if (!strcmp(e.name, op)) return &e;
  return nullptr;
}

int range_of_q(uint64_t q) { return q < (1ull << 31) ? 0 : q < (1ull << 32) ? 1 : 2; }

constexpr uint32_t kN = 256;  // the plan every op's constants come from

// the launch tables of make_plan(256, q), as nttmul.cpp fills them (no device tables: the probe
// ops take their twiddle pairs as operands)
int tables_of(uint64_t q, Plan *P, LaunchTables *T) {
  const int st = make_plan(kN, q, 0, P);
  if (st) return st;
  memset((void *)T, 0, sizeof *T);
  T->logn = P->logn;
  T->word_bits = P->word_bits;
  T->q = P->q, T->qinv_neg = P->qinv_neg;
  T->f = P->f, T->fs = P->fs, T->wf = P->wf, T->wfs = P->wfs;
  T->f4 = P->f4, T->f4s = P->f4s, T->wf4 = P->wf4, T->wf4s = P->wf4s;
  T->f8 = P->f8, T->f8s = P->f8s, T->wf8 = P->wf8, T->wf8s = P->wf8s;
  T->fi = P->fi, T->fis = P->fis, T->wfi = P->wfi, T->wfis = P->wfis;
  T->r2 = P->r2;
  T->fw = T->iw = nullptr;
  T->prio_ok = 1;
  return 0;
}

}  // namespace

extern "C" {

int probe_op_count() { return (int)registry().size(); }

const char *probe_op_name(int i) {
  return i >= 0 && i < (int)registry().size() ? registry()[i].name : nullptr;
}

// operands, results and word width of an op; NTTMUL_EINVAL for an unknown name
int probe_op_shape(const char *op, int *nin, int *nout, int *bits) {
  const Entry *e = find(op);
  if (!e) return NTTMUL_EINVAL;
  *nin = e->nin, *nout = e->nout, *bits = e->bits;
  return NTTMUL_OK;
}

// The pair tables of make_plan(256, q): fw, iw = 256 (value, companion) pairs each, widened to
// u64 (entry 0 unused); fw_signed[i] = 1 where the forward entry is in Arith32P's signed-input
// form (the inverse table of an Arith32P plan is in that form throughout).
int probe_tables(uint64_t q, uint64_t *fw, uint64_t *iw, uint8_t *fw_signed) {
  Plan P;
  LaunchTables T;
  const int st = tables_of(q, &P, &T);
  if (st) return st;
  for (uint32_t i = 0; i < 2 * kN; i++) {
    if (P.word_bits == 32) {
      fw[i] = ((const uint32_t *)P.fw.data())[i];
      iw[i] = ((const uint32_t *)P.iw.data())[i];
    } else {
      fw[i] = ((const uint64_t *)P.fw.data())[i];
      iw[i] = ((const uint64_t *)P.iw.data())[i];
    }
  }
  for (uint32_t i = 0; i < kN; i++)
    fw_signed[i] = a32_kind(q) == A32Kind::Plantard && q < (1ull << 32) &&
                   p_signed_fw_entry((int)P.logn, i);
  return NTTMUL_OK;
}

// The scale pairs of that plan, as (value, companion): F, w F, 4F, w 4F, 8F, w 8F (w = iw[1]);
// then the class constants make_params derives: -q^-1, 2^32 mod q, ceil(1.5 q), 2q.  16 words.
int probe_consts(uint64_t q, uint64_t *out) {
  Plan P;
  LaunchTables T;
  const int st = tables_of(q, &P, &T);
  if (st) return st;
  const uint64_t v[12] = {P.f, P.fs, P.wf, P.wfs, P.f4, P.f4s, P.wf4, P.wf4s,
                          P.f8, P.f8s, P.wf8, P.wf8s};
  memcpy(out, v, sizeof v);
  out[12] = P.qinv_neg;
  out[13] = out[14] = out[15] = 0;
  if (P.word_bits == 64) {
    out[15] = make_params<Arith64>(T).ar.q2;
  } else if (a32_kind(q) == A32Kind::Plantard) {
    const Arith32P ar = make_params<Arith32P>(T).ar;
    out[13] = ar.c32, out[14] = ar.as;
  }
  return NTTMUL_OK;
}

// out[k * count + i] = result k of `op` on the operands in[0 * count + i], in[1 * count + i], ...
// (host arrays).  NTTMUL_EINVAL: unknown op, or q outside the range its class serves.
int probe_run(const char *op, uint64_t q, const uint64_t *in, uint64_t *out, size_t count) {
  const Entry *e = find(op);
  if (!e || !count || count > (1u << 28) || range_of_q(q) != e->range) return NTTMUL_EINVAL;
  Plan P;
  LaunchTables T;
  const int st = tables_of(q, &P, &T);
  if (st) return st;
  const size_t ib = (size_t)e->nin * count * 8, ob = (size_t)e->nout * count * 8;
  uint64_t *din = nullptr, *dout = nullptr;
  hipError_t err = hipMalloc((void **)&din, ib);
  if (err == hipSuccess) err = hipMalloc((void **)&dout, ob);
  if (err == hipSuccess) err = hipMemcpy(din, in, ib, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = e->run(T, din, dout, (uint32_t)count);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
  (void)hipFree(din);
  (void)hipFree(dout);
  return err == hipSuccess ? NTTMUL_OK : NTTMUL_EHIP;
}

}  // extern "C"
