// level_san.cpp — the host-only part of include/nttmul_level.h under ASan / UBSan, with a main of
// its own (tests/test_level_sanitizers.py): csrc/level_plan.hpp level_view_status after the dense
// calls' statuses, in the header's order; level_addr, level_top, level_key_word and
// level_diag_word against a naive recomputation in 128-bit integers, at sizes whose top-level
// operand passes 2^32 words; and the grids of the three launches and of the range check at batch
// 0, 1, V - 1, V, V + 1 -- the very functions csrc/level.cpp and csrc/level.hip call.  None of
// them needs a device.  A launch's key reads are walked through a heap block of exactly the viewed
// operand's size, one byte per polynomial of n words, with the limb, the term and the outer index
// formed as the kernels form them, so a read that starts outside the operand is a report, and a
// second block marks what the view selects, so a read outside the view is a failure.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "level_plan.hpp"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      return 1;                                                   \
    }                                                             \
  } while (0)

using namespace nttmul;
using u128 = unsigned __int128;

static long g_walks = 0;

// the statuses in the header's order: the dense call's (a NULL context, then its arguments), then
// a NULL view, top_q_limbs < L, top_q_limbs + K > NTTMUL_RNS_MAX_LIMBS, top_terms < terms
static int check_status() {
  const uint32_t L = 4, K = 2, n = 4096;
  const nttmul_level_view good = {5, 3}, low = {3, 3}, few = {5, 1};
  const nttmul_level_view wide = {NTTMUL_RNS_MAX_LIMBS - K + 1, 3};
  const nttmul_level_view low_few = {3, 1}, wide_few = {NTTMUL_RNS_MAX_LIMBS, 1};
  CHECK(level_view_status(&good, L, K, 2) == NTTMUL_OK);
  CHECK(level_view_status(&good, L, K, 3) == NTTMUL_OK);
  CHECK(level_view_status(nullptr, L, K, 2) == NTTMUL_EINVAL);
  CHECK(level_view_status(&low, L, K, 2) == NTTMUL_EINVAL);
  CHECK(level_view_status(&wide, L, K, 2) == NTTMUL_EINVAL);
  CHECK(level_view_status(&few, L, K, 2) == NTTMUL_EINVAL);
  CHECK(level_view_status(&low_few, L, K, 2) == NTTMUL_EINVAL);
  CHECK(level_view_status(&wide_few, L, K, 2) == NTTMUL_EINVAL);
  // the identity, and the widest operand a context can view
  const nttmul_level_view same = {L, 2}, widest = {NTTMUL_RNS_MAX_LIMBS - K, 2};
  CHECK(level_view_status(&same, L, K, 2) == NTTMUL_OK);
  CHECK(level_view_status(&widest, L, K, 2) == NTTMUL_OK);
  // top_q_limbs + K is formed in 64 bits
  const nttmul_level_view huge = {0xFFFFFFFFu, 2};
  CHECK(level_view_status(&huge, L, K, 2) == NTTMUL_EINVAL);

  // the dense statuses come first, whatever the view is: the entry points call them in this order
  uint32_t kv[NTTMUL_HOIST_MAX_ROTS];
  const uint32_t k1[1] = {5};
  int x = 0;
  const void *p = &x;
  auto mac = [&](bool ctx, const void *c, const uint32_t *k, uint32_t rots, size_t batch,
                 uint32_t terms, uint32_t comps, const nttmul_level_view *v) {
    if (const int st = ksntt_mac_status(ctx, ctx ? n : 0, c, p, p, k, rots, batch, terms, comps, kv))
      return st;
    return level_view_status(v, L, K, terms);
  };
  CHECK(mac(true, p, k1, 1, 1, 2, 1, &good) == NTTMUL_OK);
  CHECK(mac(true, p, k1, 1, 0, 2, 1, &good) == NTTMUL_OK);           // batch = 0 after the checks
  CHECK(mac(true, p, k1, 1, 0, 2, 1, nullptr) == NTTMUL_EINVAL);     // also at batch = 0
  CHECK(mac(false, p, k1, 1, 1, 2, 1, &good) == NTTMUL_EINVAL);
  CHECK(mac(true, nullptr, k1, 1, 1, 2, 1, &good) == NTTMUL_EINVAL);
  CHECK(mac(true, p, nullptr, 1, 1, 2, 1, &good) == NTTMUL_EINVAL);
  CHECK(mac(true, p, k1, 0, 1, 2, 1, &good) == NTTMUL_EINVAL);
  CHECK(mac(true, p, k1, 1, 1, 0, 1, &good) == NTTMUL_EINVAL);
  CHECK(mac(true, p, k1, 1, 1, 2, 3, &good) == NTTMUL_EINVAL);
  const uint32_t even[1] = {4};
  CHECK(mac(true, p, even, 1, 1, 2, 1, &good) == NTTMUL_EINVAL);
  auto relin = [&](bool ctx, const void *c, size_t batch, uint32_t pairs, uint32_t terms,
                   const nttmul_level_view *v) {
    if (const int st = ctmul_relin_status(ctx, c, p, p, p, p, batch, pairs, terms)) return st;
    return level_view_status(v, L, K, terms);
  };
  CHECK(relin(true, p, 1, 1, 2, &good) == NTTMUL_OK);
  CHECK(relin(true, p, 1, 1, 2, nullptr) == NTTMUL_EINVAL);
  CHECK(relin(true, p, 1, 0, 2, &good) == NTTMUL_EINVAL);
  CHECK(relin(true, p, 1, 1, 0, &good) == NTTMUL_EINVAL);
  CHECK(relin(true, nullptr, 1, 1, 2, &good) == NTTMUL_EINVAL);
  CHECK(relin(true, nullptr, 0, 1, 2, &good) == NTTMUL_OK);
  CHECK(relin(true, p, 1, 1, 3, &good) == NTTMUL_OK);
  CHECK(relin(true, p, 1, 1, 4, &good) == NTTMUL_EINVAL);            // top_terms < terms
  CHECK(lintrans_apply_status(true, n, p, p, p, k1, 1, 1, 2, 2, kv) == NTTMUL_OK);
  return 0;
}

// level_addr and the word offsets against a naive recomputation, and every read of a launch
// through blocks of exactly the operand's size in polynomials
static int check_addr(uint32_t L, uint32_t K, uint32_t logn, uint32_t L_top, uint32_t top_terms,
                      uint32_t terms, uint32_t outer) {
  const nttmul_level_view view = {L_top, top_terms};
  CHECK(level_view_status(&view, L, K, terms) == NTTMUL_OK);
  const LevelAddr A = level_addr(L, K, logn, view);
  const u128 n = (u128)1 << logn, TL = (u128)L_top + K;
  CHECK(A.top_limbs == L_top + K && A.shift == L_top - L && A.top_terms == top_terms);
  CHECK((u128)A.kstep == TL * n && (u128)A.kcstep == TL * n * top_terms);
  CHECK((u128)level_key_words(A, outer) == (u128)outer * top_terms * TL * n);
  CHECK((u128)level_diag_words(A, outer) == (u128)outer * TL * n);
  // one byte per polynomial: key [outer][top_terms][top_limbs], diag [outer][top_limbs]
  const size_t kpolys = (size_t)outer * top_terms * A.top_limbs, dpolys = (size_t)outer * A.top_limbs;
  uint8_t *key = (uint8_t *)calloc(kpolys, 1), *diag = (uint8_t *)calloc(dpolys, 1);
  CHECK(key && diag);
  for (uint32_t o = 0; o < outer; o++)
    for (uint32_t m = 0; m < L + K; m++) {
      const uint32_t tm = m < L ? m : m - L + L_top;                 // the header's top(m)
      CHECK(level_top(A, m) == tm && tm < A.top_limbs);
      for (uint32_t t = 0; t < terms; t++) {
        for (uint32_t j : {0u, 1u, (uint32_t)n - 1}) {
          const u128 want = (((u128)o * top_terms + t) * TL + tm) * n + j;
          const size_t got = level_key_word(A, o, t, m, j);
          CHECK((u128)got == want && got < level_key_words(A, outer));
          key[got >> logn]++;                                        // inside the block, or a report
          g_walks++;
        }
      }
      for (uint32_t j : {0u, (uint32_t)n - 1}) {
        const u128 want = ((u128)o * TL + tm) * n + j;
        const size_t got = level_diag_word(A, o, m, j);
        CHECK((u128)got == want && got < level_diag_words(A, outer));
        diag[got >> logn]++;
        g_walks++;
      }
    }
  // exactly the view's polynomials were read, each as often as the others
  size_t kread = 0, dread = 0;
  for (size_t i = 0; i < kpolys; i++) {
    const uint32_t limb = (uint32_t)(i % A.top_limbs), t = (uint32_t)(i / A.top_limbs % top_terms);
    const bool in_view = t < terms && (limb < L || limb >= L_top);
    CHECK(key[i] == (in_view ? 3 : 0));
    kread += key[i] != 0;
  }
  for (size_t i = 0; i < dpolys; i++) {
    const uint32_t limb = (uint32_t)(i % A.top_limbs);
    CHECK(diag[i] == ((limb < L || limb >= L_top) ? 2 : 0));
    dread += diag[i] != 0;
  }
  CHECK(kread == (size_t)outer * terms * (L + K) && dread == (size_t)outer * (L + K));
  // the range check's grid covers exactly the selected words
  const LevelCheckGrid G = level_check_grid(A, outer, terms);
  CHECK((u128)G.total == (u128)outer * terms * (L + K) * n && G.wgx * 256 >= G.total &&
        (G.wgx == 0 || (G.wgx - 1) * 256 < G.total));
  const LevelCheckGrid D = level_check_grid(A, outer, 1);
  CHECK((u128)D.total == (u128)outer * (L + K) * n);
  free(key);
  free(diag);
  return 0;
}

static int check_addresses() {
  // the GPU tests' chain, every level
  for (uint32_t L : {5u, 4u, 3u, 1u})
    for (uint32_t logn : {8u, 9u, 13u})
      if (check_addr(L, 2, logn, 5, 3, (L + 1) / 2, 6)) return 1;
  // the issue's example: n = 65536, L = 24, K = 6, alpha = 6; one rotation key is
  // 2 * 4 * 30 * 65536 words, a set of 300 of them passes 2^32 words
  for (uint32_t L : {24u, 23u, 18u, 13u, 6u, 1u})
    if (check_addr(L, 6, 16, 24, 4, (L + 5) / 6, 600)) return 1;
  {
    const nttmul_level_view view = {24, 4};
    const LevelAddr A = level_addr(18, 6, 16, view);
    CHECK(level_key_words(A, 600) > ((size_t)1 << 32));
    CHECK(level_key_word(A, 599, 2, 23, 65535) > ((size_t)1 << 32));
    CHECK(level_diag_words(A, 4096) > ((size_t)1 << 32));
  }
  // the widest operand: 62 + 2 limbs, 31 terms
  if (check_addr(2, 2, 16, NTTMUL_RNS_MAX_LIMBS - 2, 31, 1, 32)) return 1;
  if (check_addr(62, 2, 16, NTTMUL_RNS_MAX_LIMBS - 2, 62, 62, 2)) return 1;
  return 0;
}

// the grids at batch 0, 1, V - 1, V, V + 1 and where they leave a grid dimension
static int check_grids() {
  const uint32_t V = kLevelMacSlices;
  CHECK(V == 4 && kLtSlices == 4 && kCtSlices == 4);
  for (uint32_t logn = 8; logn <= 16; logn++) {
    const size_t per = (size_t)1 << (logn - 8);  // slices, and slot ranges, of a polynomial
    for (size_t batch : {(size_t)0, (size_t)1, (size_t)V - 1, (size_t)V, (size_t)V + 1}) {
      for (uint32_t rots : {1u, 3u, 16u}) {
        const LevelMacGrid G = level_mac_grid(batch, logn, rots);
        CHECK(G.ok && G.slices == batch * per && G.bx == (G.slices + V - 1) / V);
        CHECK(G.wgx == G.bx * rots && G.tail == G.slices % V);
        // every slice is taken by exactly one workgroup and none lies past the end unguarded
        std::vector<uint8_t> seen(G.slices, 0);
        for (size_t x = 0; x < G.wgx; x++)
          for (uint32_t v = 0; v < V; v++) {
            const size_t s = (x / rots) * V + v;
            if (s < G.slices && x % rots == 0) seen[s]++;
            g_walks++;
          }
        for (uint8_t c : seen) CHECK(c == 1);
      }
      for (const LtGrid &G : {level_lintrans_grid(batch, logn), level_relin_grid(batch, logn)}) {
        CHECK(G.ok && G.units == batch && G.groups == (batch + V - 1) / V);
        CHECK(G.wgx == G.groups * per && G.tail == batch % V);
        std::vector<uint8_t> seen(batch * per, 0);
        for (size_t x = 0; x < G.wgx; x++) {
          const size_t g = x >> (logn - 8), s = x & (per - 1);
          for (uint32_t v = 0; v < V; v++) {
            const size_t e = g * V + v;
            if (e < batch) seen[e * per + s]++;
            g_walks++;
          }
        }
        for (uint8_t c : seen) CHECK(c == 1);
      }
    }
  }
  CHECK(!level_mac_grid(1, 16, 0).ok);
  CHECK(level_mac_grid(((size_t)0x7FFFFFFF * 4) >> 8, 16, 1).ok);
  CHECK(!level_mac_grid((((size_t)0x7FFFFFFF * 4) >> 8) + 1, 16, 1).ok);
  CHECK(!level_mac_grid((size_t)1 << 32, 8, 3).ok);
  CHECK(!level_lintrans_grid((size_t)1 << 33, 8).ok && !level_relin_grid((size_t)1 << 26, 16).ok);
  {
    const nttmul_level_view view = {60, 30};
    const LevelAddr A = level_addr(60, 4, 16, view);
    CHECK(level_check_grid(A, 32, 30).ok && !level_check_grid(A, 8192, 30).ok);
  }
  return 0;
}

int main() {
  if (check_status() || check_addresses() || check_grids()) return 1;
  printf("level sanitizer run ok: %ld walks\n", g_walks);
  return 0;
}
