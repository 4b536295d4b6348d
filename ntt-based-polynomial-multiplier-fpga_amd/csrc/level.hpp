// level.hpp — internal interface between the host entry points of include/nttmul_level.h
// (level.cpp) and the launchers of level.hip.  lib/libnttmul_level.so only.  The launchers have
// the shapes ksntt.cpp, lintrans.cpp and ctmul.cpp call in place of their own (ksntt.hpp
// KsnttViewed, lintrans.hpp LtViewed, ctmul.hpp CtViewed), with the call's LevelAddr behind them.
#pragma once
#include "ctmul.hpp"
#include "level_plan.hpp"
#include "lintrans.hpp"

namespace nttmul {

enum LevelOp { kLevelMac = 0, kLevelLintrans = 1, kLevelRelin = 2 };

// mac with b_hat viewed: a_hat [batch][terms][M][n], b_hat [rots][comps][top_terms][top_limbs][n]
// -> c_hat [batch][rots][comps][M][n]
hipError_t launch_level_mac(const KsnttTables &T, void *c_hat, const void *a_hat,
                            const void *b_hat, const HoistArgs &H, size_t batch, uint32_t terms,
                            const LevelAddr &A, hipStream_t s);
// apply with b_hat and, when given, w_hat [rots][top_limbs][n] viewed
hipError_t launch_level_lintrans(const LtTables &T, void *c_hat, const void *a_hat,
                                 const void *b_hat, const void *w_hat, const void *c0_hat,
                                 const HoistArgs &H, size_t batch, uint32_t terms,
                                 const LevelAddr &A, hipStream_t s);
// relin with key_hat [2][top_terms][top_limbs][n] viewed
hipError_t launch_level_relin(const CtTables &T, void *c_hat, const void *up_hat,
                              const void *key_hat, const void *x_hat, const void *y_hat,
                              size_t batch, uint32_t pairs, uint32_t terms, const LevelAddr &A,
                              hipStream_t s);
// The strided k_rns_check_range: the words of `op` the view selects, `outer` components of
// `terms` terms each (has_terms: a key; otherwise a diagonal set and terms = 1), against
// q[0 .. L + K); sets *bad
hipError_t launch_level_check(const void *op, const uint64_t *q, int word_bits, const LevelAddr &A,
                              size_t outer, uint32_t terms, bool has_terms, int *bad,
                              hipStream_t s);
// "k_level_mac<Arith64,u64,2>", "k_level_lintrans<Arith64,u64,2,1>", "k_level_relin<Arith64,u64>":
// the dry run of the launching statement itself
hipError_t describe_level(int op, uint32_t logn, int word_bits, uint32_t comps, bool weighted,
                          std::string *out);

}  // namespace nttmul
