// ctmul_san.cpp — the host-only part of include/nttmul_ctmul.h under ASan / UBSan, with a main of
// its own (tests/test_ctmul_sanitizers.py): csrc/ctmul_plan.hpp ctmul_validate over csrc/basis.cpp
// (create's statuses and their order), ctmul_constants against values recomputed here naively, the
// calls' statuses in the header's order, and ctmul_relin_grid, ctmul_high_grid and the word counts,
// the very functions csrc/ctmul.cpp and csrc/ctmul.hip call.  None of them needs a device.  A
// launch's workgroups are walked through heap blocks of exactly the operands' sizes, with the
// entry, the slot range and the vector formed from the workgroup and lane index as the kernels
// form them, so a workgroup that starts or ends outside an operand is a report; the word offsets
// are computed for shapes where they pass 2^32.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ctmul_plan.hpp"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      return 1;                                                   \
    }                                                             \
  } while (0)

using namespace nttmul;
using u128 = unsigned __int128;

// primes = 1 mod 2^17 (tests/dispatch_cases.py, tests/rnsmp_cases.py): two below 2^31, two of 62
// and 61 bits, one in [2^31, 2^32)
static const uint64_t kQ31 = 2013265921ull, kQ31b = 2147352577ull;
static const uint64_t kQ62 = 0x3FFFFFFFFFE80001ull, kQ61 = 2305843009211596801ull;
static const uint64_t kQ32 = 4293918721ull;

static int status(uint32_t n, const uint64_t *q, uint32_t L, const uint64_t *p, uint32_t K,
                  uint32_t flags = 0, uint64_t pq = 0, size_t size = sizeof(nttmul_params)) {
  nttmul_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.n = n;
  prm.q = pq;
  prm.ndev = 1;
  prm.flags = flags;
  CtPlan P;
  const int st = ctmul_validate(&prm, size, q, L, p, K, &P);
  // nttmul_lintrans_create's status is the same decision
  LtPlan T;
  if (lintrans_validate(&prm, size, q, L, p, K, &T) != st) return -99;
  if (st == NTTMUL_OK) {
    if (P.L != L || P.K != K || P.m.size() != (size_t)L + K || P.n != n) return -100;
    if (P.logn != T.logn || P.word_bits != T.word_bits || P.flags != T.flags) return -106;
    ctmul_constants(&P);  // every table at its size, every value against a naive recomputation
    if (P.r1.size() != (size_t)L + K || P.pr.size() != L) return -101;
    for (uint32_t l = 0; l < L + K; l++) {
      const uint64_t m = l < L ? q[l] : p[l - L];
      if (P.m[l] != m) return -102;
      u128 r = 1;
      for (int b = 0; b < P.word_bits; b++) r = r * 2 % m;
      if (P.r1[l] != (uint64_t)r || P.r1[l] >= m) return -103;
    }
    for (uint32_t l = 0; l < L; l++) {
      u128 v = 1;
      for (uint32_t j = 0; j < K; j++) v = v * (p[j] % q[l]) % q[l];
      for (int b = 0; b < P.word_bits; b++) v = v * 2 % q[l];   // P R mod q_l
      if (P.pr[l] != (uint64_t)v || P.pr[l] == 0 || P.pr[l] >= q[l]) return -105;
    }
  }
  return st;
}

static int check_create() {
  const uint64_t q32[2] = {kQ31, kQ31b}, q64[2] = {kQ62, kQ61};
  for (uint32_t n : {256u, 4096u, 8192u, 65536u}) {
    CHECK(status(n, q32, 1, q32 + 1, 1) == NTTMUL_OK);
    CHECK(status(n, q64, 1, q64 + 1, 1) == NTTMUL_OK);
    CHECK(status(n, q32, 0, q32 + 1, 1) == NTTMUL_EINVAL);          // q_limbs = 0
    CHECK(status(n, q32, 1, q32 + 1, 0) == NTTMUL_EINVAL);          // p_limbs = 0
    CHECK(status(n, nullptr, 1, q32 + 1, 1) == NTTMUL_EINVAL);
    CHECK(status(n, q32, 1, nullptr, 1) == NTTMUL_EINVAL);
    CHECK(status(n, q32, 1, q32, 1) == NTTMUL_EINVAL);              // a prime in both bases
    CHECK(status(n, q32, 1, q32 + 1, 1, 0, kQ31) == NTTMUL_EINVAL); // params->q
    CHECK(status(n, q32, 1, q32 + 1, 1, 0, 0, 4) == NTTMUL_EINVAL); // params size
    CHECK(status(n, q32, 1, q32 + 1, 1, NTTMUL_FLAG_CYCLIC) == NTTMUL_EUNSUPPORTED);
    CHECK(status(n, q32, 1, q64, 1) == NTTMUL_EUNSUPPORTED);        // mixed classes
    CHECK(status(n, q64, 1, q32, 1) == NTTMUL_EUNSUPPORTED);
    CHECK(status(n, q32, 1, &kQ32, 1) == NTTMUL_EUNSUPPORTED);      // [2^31, 2^32)
    const uint64_t comp[1] = {kQ31 + 2};
    CHECK(status(n, q32, 1, comp, 1) == NTTMUL_EINVAL);             // not prime
    // the order: every EINVAL before any EUNSUPPORTED
    CHECK(status(n, &kQ32, 1, comp, 1) == NTTMUL_EINVAL);
    CHECK(status(n, q32, 1, q32 + 1, 1, NTTMUL_FLAG_CYCLIC, kQ31) == NTTMUL_EINVAL);
  }
  CHECK(status(128, q32, 1, q32 + 1, 1) == NTTMUL_EINVAL);
  CHECK(status(10000, q32, 1, q32 + 1, 1) == NTTMUL_EINVAL);
  CHECK(status(131072, q32, 1, q32 + 1, 1) == NTTMUL_EINVAL);       // 2^18 does not divide q - 1
  // limb counts: exactly NTTMUL_RNS_MAX_LIMBS entries on the heap per basis, so a read past a
  // basis' own count is a report
  uint64_t *many = (uint64_t *)malloc(sizeof(uint64_t) * NTTMUL_RNS_MAX_LIMBS);
  CHECK(many);
  for (uint32_t i = 0; i < NTTMUL_RNS_MAX_LIMBS; i++) many[i] = 3 + i;
  CHECK(status(256, many, NTTMUL_RNS_MAX_LIMBS + 1, q32, 1) == NTTMUL_EINVAL);
  CHECK(status(256, q32, 1, many, NTTMUL_RNS_MAX_LIMBS + 1) == NTTMUL_EINVAL);
  CHECK(status(256, many, NTTMUL_RNS_MAX_LIMBS, q32, 1) == NTTMUL_EINVAL);
  free(many);
  return 0;
}

// the calls' statuses in the header's order: a NULL context; pairs = 0; terms = 0 (relin); a NULL
// operand with batch > 0; batch = 0 succeeds
static int check_calls() {
  int one = 0;
  const void *a = &one;
  CHECK(ctmul_high_status(true, a, a, a, 1, 1) == NTTMUL_OK);
  CHECK(ctmul_high_status(true, a, a, a, 1, 1u << 31) == NTTMUL_OK);
  CHECK(ctmul_high_status(true, nullptr, nullptr, nullptr, 0, 1) == NTTMUL_OK);
  // each refusal with everything after it in the order wrong as well: the first one decides
  CHECK(ctmul_high_status(false, a, a, a, 1, 1) == NTTMUL_EINVAL);
  CHECK(ctmul_high_status(false, nullptr, nullptr, nullptr, 0, 0) == NTTMUL_EINVAL);
  CHECK(ctmul_high_status(true, a, a, a, 1, 0) == NTTMUL_EINVAL);                 // pairs
  CHECK(ctmul_high_status(true, nullptr, nullptr, nullptr, 0, 0) == NTTMUL_EINVAL);  // at batch 0
  for (int mask = 0; mask < 7; mask++)                              // a NULL operand, batch > 0
    CHECK(ctmul_high_status(true, mask & 1 ? a : nullptr, mask & 2 ? a : nullptr,
                            mask & 4 ? a : nullptr, 1, 1) == NTTMUL_EINVAL);

  CHECK(ctmul_relin_status(true, a, a, a, a, a, 1, 1, 1) == NTTMUL_OK);
  CHECK(ctmul_relin_status(true, a, a, a, a, a, 1, 1u << 31, 1u << 31) == NTTMUL_OK);
  CHECK(ctmul_relin_status(true, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, 1) ==
        NTTMUL_OK);
  CHECK(ctmul_relin_status(false, a, a, a, a, a, 1, 1, 1) == NTTMUL_EINVAL);
  CHECK(ctmul_relin_status(true, a, a, a, a, a, 1, 0, 1) == NTTMUL_EINVAL);       // pairs
  CHECK(ctmul_relin_status(true, a, a, a, a, a, 1, 1, 0) == NTTMUL_EINVAL);       // terms
  CHECK(ctmul_relin_status(true, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1) ==
        NTTMUL_EINVAL);                                             // at batch 0
  CHECK(ctmul_relin_status(true, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, 0) ==
        NTTMUL_EINVAL);
  for (int mask = 0; mask < 31; mask++)
    CHECK(ctmul_relin_status(true, mask & 1 ? a : nullptr, mask & 2 ? a : nullptr,
                             mask & 4 ? a : nullptr, mask & 8 ? a : nullptr,
                             mask & 16 ? a : nullptr, 1, 1, 1) == NTTMUL_EINVAL);
  return 0;
}

// k_ctmul_relin's workgroups over a block of one byte per (entry, limb, slot range) of c_hat:
// every byte is written exactly once, dead slices read entry 0 and never store
static int walk_relin(size_t batch, uint32_t logn, uint32_t M, uint32_t v) {
  const LtGrid G = ctmul_relin_grid(batch, logn, v);
  const uint32_t lgs = logn - 8;
  const size_t ranges = (size_t)1 << lgs;
  CHECK(G.units == batch && G.groups == (batch + v - 1) / v && G.tail == batch % v && G.ok);
  CHECK(G.wgx == G.groups * ranges);
  if (!batch) {
    CHECK(G.wgx == 0);
    return 0;
  }
  uint8_t *c = (uint8_t *)calloc(batch * M * ranges, 1), *a = (uint8_t *)calloc(batch * ranges, 1);
  CHECK(c && a);
  size_t dead = 0;
  for (uint32_t l = 0; l < M; l++)
    for (size_t x = 0; x < G.wgx; x++)
      for (uint32_t s = 0; s < v; s++) {
        const size_t e = (x >> lgs) * v + s;                       // the range is the faster index
        const bool live = e < batch;
        const size_t p = live ? e : 0, range = x & (ranges - 1);
        CHECK(p < batch && range < ranges);
        a[p * ranges + range] |= 1;                                // a read of up_hat, x_hat, y_hat
        if (live) c[(p * M + l) * ranges + range]++;
        else dead++;
      }
  for (size_t i = 0; i < batch * M * ranges; i++) CHECK(c[i] == 1);
  for (size_t i = 0; i < batch * ranges; i++) CHECK(a[i] == 1);
  CHECK(dead == (G.groups * v - batch) * M * ranges);
  free(c);
  free(a);
  return 0;
}

// k_ctmul_high's lanes over a block of one byte per vector of d2_hat, [batch][L][n / vec], and one
// per vector of component 1 of x_hat, [batch][pairs][2][L][n / vec]: every vector of d2_hat is
// written exactly once, every vector of component 1 read once and none of component 0
static int walk_high(size_t batch, uint32_t logn, uint32_t L, uint32_t pairs, int word_bits) {
  const CtHighGrid G = ctmul_high_grid(batch, logn, word_bits);
  const uint32_t vec = word_bits == 32 ? 4 : 2, lgp = logn - (vec == 4 ? 2 : 1);
  const size_t pv = (size_t)1 << lgp;
  CHECK(G.vec == vec && ctmul_vec_words(word_bits) == vec && vec * (word_bits / 8) == 16);
  CHECK(G.vectors == batch * pv && G.wgx == (G.vectors + 255) / 256 && G.ok);
  CHECK(G.tail == G.vectors % 256 && G.per == (pv < 256 ? 256 / pv : 1));
  if (!batch) {
    CHECK(G.wgx == 0);
    return 0;
  }
  uint8_t *d = (uint8_t *)calloc(batch * L * pv, 1);
  uint8_t *x = (uint8_t *)calloc(batch * pairs * 2 * L * pv, 1);
  CHECK(d && x);
  size_t idle = 0;
  for (uint32_t l = 0; l < L; l++)
    for (size_t b = 0; b < G.wgx; b++)
      for (uint32_t t = 0; t < 256; t++) {
        const size_t g = b * 256 + t;
        if (g >= G.vectors) {
          idle++;
          continue;
        }
        const size_t p = g >> lgp, j = g & (pv - 1);
        CHECK(p < batch);
        const size_t xo = ((p * pairs * 2 + 1) * L + l) * pv + j;
        for (uint32_t s = 0; s < pairs; s++) x[xo + (size_t)s * 2 * L * pv]++;
        d[(p * L + l) * pv + j]++;
      }
  for (size_t i = 0; i < batch * L * pv; i++) CHECK(d[i] == 1);
  for (size_t i = 0; i < batch * pairs * 2 * L * pv; i++)
    CHECK(x[i] == ((i / (L * pv)) & 1));                            // component 1 only
  CHECK(idle == (G.wgx * 256 - G.vectors) * L);
  free(d);
  free(x);
  return 0;
}

int main() {
  if (check_create() || check_calls()) return 1;
  int walks = 0;
  const uint32_t V = kCtSlices;
  CHECK(V == 4 && V == kLtSlices && ctmul_slices(32) == V && ctmul_slices(64) == V);
  for (uint32_t logn : {8u, 9u, 12u, 13u, 16u})
    for (size_t batch : {(size_t)0, (size_t)1, (size_t)V - 1, (size_t)V, (size_t)V + 1,
                         (size_t)2 * V - 1, (size_t)33})
      for (uint32_t M : {2u, 6u}) {
        for (uint32_t v : {V, 2u}) {                                // the library's, the A/B's
          if (walk_relin(batch, logn, M, v)) return 1;
          walks++;
        }
        for (int bits : {32, 64})
          for (uint32_t pairs : {1u, 3u}) {
            if (walk_high(batch, logn, M - 1, pairs, bits)) return 1;
            walks++;
          }
      }
  // the partial last workgroups, in the header's words
  CHECK(ctmul_relin_grid(V + 1, 8).groups == 2 && ctmul_relin_grid(V + 1, 8).tail == 1);
  CHECK(ctmul_relin_grid(2 * V - 1, 12).wgx == 32 && ctmul_relin_grid(2 * V - 1, 12).tail == V - 1);
  CHECK(ctmul_relin_grid(5, 16).wgx == 512);
  CHECK(ctmul_high_grid(1, 8, 32).per == 4 && ctmul_high_grid(1, 8, 32).tail == 64);
  CHECK(ctmul_high_grid(5, 8, 32).wgx == 2 && ctmul_high_grid(5, 8, 32).tail == 64);
  CHECK(ctmul_high_grid(1, 8, 64).per == 2 && ctmul_high_grid(7, 9, 32).tail == 128);
  CHECK(ctmul_high_grid(7, 9, 64).per == 1 && ctmul_high_grid(7, 9, 64).tail == 0);
  // sizes past 2^32 words.  No memory is touched: the counts and offsets alone
  {
    const uint32_t n = 65536, L = 60, K = 4;
    const size_t batch = 2048;
    size_t rw[4], hw[2];
    ctmul_relin_words(L, K, n, batch, 3, 4, rw);
    ctmul_high_words(L, n, batch, 3, hw);
    CHECK(rw[0] == batch * 2 * 64 * 65536 && rw[0] > ((size_t)1 << 32));
    CHECK(rw[1] == batch * 4 * 64 * 65536 && rw[1] == (size_t)1 << 35);
    CHECK(rw[2] == (size_t)2 * 4 * 64 * 65536);
    CHECK(rw[3] == batch * 3 * 2 * 60 * 65536 && rw[3] > ((size_t)1 << 32) && hw[1] == rw[3]);
    CHECK(hw[0] == batch * 60 * 65536 && hw[0] > ((size_t)1 << 32));
    // the last entry's polynomial offsets as the kernels form them
    const size_t p = batch - 1, u_off = ((p * 4 * 64 + 63) << 16), c_off = ((p * 2 * 64 + 63) << 16);
    CHECK(u_off + (size_t)3 * 64 * n + n == rw[1] && c_off + (size_t)64 * n + n == rw[0]);
    const size_t x_off = ((p * 3 * 2 * 60 + 59) << 16), half = (size_t)60 << 16;
    CHECK(x_off + (size_t)2 * 2 * half + half + n == rw[3]);        // pair 2, component 1, relin
    const size_t h_off = (((p * 3 * 2 + 1) * 60 + 59) << 16);
    CHECK(h_off + (size_t)2 * 2 * half + n == hw[1]);               // pair 2, high
    CHECK(((p * 60 + 59) << 16) + n == hw[0]);
    const LtGrid G = ctmul_relin_grid(batch, 16);
    CHECK(G.ok && G.wgx == (size_t)512 * 256 && G.tail == 0);
    const CtHighGrid H = ctmul_high_grid(batch, 16, 64);
    CHECK(H.ok && H.vectors == batch * 32768 && H.wgx == batch * 128 && H.tail == 0);
    // a batch whose workgroups no longer fit a grid dimension is refused, not wrapped
    CHECK(!ctmul_relin_grid((size_t)1 << 34, 16).ok && ctmul_relin_grid((size_t)1 << 24, 16).ok);
    CHECK(!ctmul_high_grid((size_t)1 << 34, 16, 64).ok && ctmul_high_grid((size_t)1 << 24, 16, 32).ok);
  }
  printf("ctmul sanitizer run ok: %d walks\n", walks);
  return 0;
}
