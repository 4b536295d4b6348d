// level_plan.hpp — the host-only part of include/nttmul_level.h: what a view call decides before
// any device access, the address arithmetic of a viewed operand and the grids of the launches.
// Plain C++ with no HIP header, so that a CPU build can run it under sanitizers
// (tests/sanitize/level_san.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ctmul_plan.hpp"
#include "ksntt_plan.hpp"
#include "nttmul_level.h"

namespace nttmul {

// The view's own status, after the dense call's: a NULL view; top_q_limbs below the context's L;
// top_q_limbs + K above NTTMUL_RNS_MAX_LIMBS; top_terms below the call's terms
inline int level_view_status(const nttmul_level_view *view, uint32_t L, uint32_t K,
                             uint32_t terms) {
  if (!view) return NTTMUL_EINVAL;
  if (view->top_q_limbs < L) return NTTMUL_EINVAL;
  if ((uint64_t)view->top_q_limbs + K > NTTMUL_RNS_MAX_LIMBS) return NTTMUL_EINVAL;
  if (view->top_terms < terms) return NTTMUL_EINVAL;
  return NTTMUL_OK;
}

// A viewed operand as a launch addresses it.  A key is [outer][top_terms][top_limbs][n], a
// diagonal set [outer][top_limbs][n]; limb m < L + K of the context is limb top(m) of the operand.
// kstep and kcstep are the two strides of the kernels, in words: a term and an outer index of a key
struct LevelAddr {
  uint32_t L = 0, K = 0, logn = 0;
  uint32_t top_limbs = 0, top_terms = 0;  // L_top + K, and the terms the key was made with
  uint32_t shift = 0;                     // L_top - L: what a limb of P moves by
  size_t kstep = 0, kcstep = 0;           // top_limbs n, top_terms top_limbs n
};

inline LevelAddr level_addr(uint32_t L, uint32_t K, uint32_t logn, const nttmul_level_view &view) {
  LevelAddr A;
  A.L = L;
  A.K = K;
  A.logn = logn;
  A.top_limbs = view.top_q_limbs + K;
  A.top_terms = view.top_terms;
  A.shift = view.top_q_limbs - L;
  A.kstep = (size_t)A.top_limbs << logn;
  A.kcstep = A.kstep * A.top_terms;
  return A;
}

// top(m): the operand's limb behind limb m of the context
inline uint32_t level_top(const LevelAddr &A, uint32_t m) { return m < A.L ? m : m + A.shift; }

// Word offset of slot j of limb m of term t of outer index o of a key, and of a diagonal set
// (which has no term index), the way the kernels form it: two strides and the limb shift
inline size_t level_key_word(const LevelAddr &A, size_t o, uint32_t t, uint32_t m, uint32_t j) {
  return o * A.kcstep + (size_t)t * A.kstep + ((size_t)level_top(A, m) << A.logn) + j;
}
inline size_t level_diag_word(const LevelAddr &A, size_t o, uint32_t m, uint32_t j) {
  return o * A.kstep + ((size_t)level_top(A, m) << A.logn) + j;
}

// Words of a whole viewed operand (what a host form stages): a key of `outer` = rots comps (or 2)
// components, a diagonal set of `outer` = rots
inline size_t level_key_words(const LevelAddr &A, size_t outer) { return outer * A.kcstep; }
inline size_t level_diag_words(const LevelAddr &A, size_t outer) { return outer * A.kstep; }

// The range check of a viewed operand: one thread per selected word, outer terms (L + K) n of
// them (terms = 1 and stride kstep for a diagonal set), 256 per workgroup.  ok: the workgroups fit
// a grid dimension
struct LevelCheckGrid {
  size_t total, wgx;
  bool ok;
};
inline LevelCheckGrid level_check_grid(const LevelAddr &A, size_t outer, uint32_t terms) {
  LevelCheckGrid G;
  G.total = (outer * terms * ((size_t)A.L + A.K)) << A.logn;
  G.wgx = G.total / 256 + (G.total % 256 != 0);
  G.ok = G.wgx <= 0x7FFFFFFFull;
  return G;
}

// k_level_mac's grid, k_ksntt_mac's: (ceil(slices / V) rots, L + K), slices = batch n / 256,
// V = 4 slices of 256 slots per workgroup.  tail: the slices of the last, partial workgroup
constexpr uint32_t kLevelMacSlices = 4;
struct LevelMacGrid {
  size_t slices, bx, wgx;
  uint32_t tail;
  bool ok;
};
inline LevelMacGrid level_mac_grid(size_t batch, uint32_t logn, uint32_t rots) {
  LevelMacGrid G;
  G.slices = batch << (logn - 8);
  G.bx = G.slices / kLevelMacSlices + (G.slices % kLevelMacSlices != 0);
  G.tail = (uint32_t)(G.slices % kLevelMacSlices);
  G.ok = rots != 0 && G.bx <= 0x7FFFFFFFull / rots;
  G.wgx = G.ok ? G.bx * rots : 0;
  return G;
}

// k_level_lintrans's and k_level_relin's grids are the dense kernels': lintrans_grid's
// batch-sliced form with V = kLtSlices and ctmul_relin_grid with V = kCtSlices
inline LtGrid level_lintrans_grid(size_t batch, uint32_t logn) {
  return lintrans_grid(batch, logn, false, kLtSlices);
}
inline LtGrid level_relin_grid(size_t batch, uint32_t logn) {
  return ctmul_relin_grid(batch, logn, kCtSlices);
}

}  // namespace nttmul
