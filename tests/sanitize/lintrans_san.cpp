// lintrans_san.cpp — the host-only part of include/nttmul_lintrans.h under ASan / UBSan, with a
// main of its own (tests/test_lintrans_sanitizers.py): csrc/lintrans_plan.hpp lintrans_validate
// over csrc/basis.cpp (create's statuses and their order), lintrans_constants against values
// recomputed here naively, apply's statuses in the header's order, and lintrans_grid and
// lintrans_words, the very functions csrc/lintrans.cpp and csrc/lintrans.hip call.  None of them
// needs a device.  A launch's workgroups are walked through heap blocks of exactly the operands'
// sizes, one byte per (batch entry, limb, range of 256 slots), with the entry and the slot range
// formed from the workgroup index as k_lintrans forms them, so a workgroup that starts or ends
// outside an operand is a report; the word offsets are computed for shapes where they pass 2^32.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lintrans_plan.hpp"

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
  LtPlan P;
  const int st = lintrans_validate(&prm, size, q, L, p, K, &P);
  if (st == NTTMUL_OK) {
    if (P.L != L || P.K != K || P.m.size() != (size_t)L + K || P.n != n) return -100;
    lintrans_constants(&P);  // every table at its size, every value against a naive recomputation
    if (P.r1.size() != (size_t)L + K || P.r2.size() != (size_t)L + K || P.pq.size() != L)
      return -101;
    for (uint32_t l = 0; l < L + K; l++) {
      const uint64_t m = l < L ? q[l] : p[l - L];
      if (P.m[l] != m) return -102;
      u128 r = 1;
      for (int b = 0; b < P.word_bits; b++) r = r * 2 % m;
      if (P.r1[l] != (uint64_t)r || P.r2[l] != (uint64_t)(r * r % m)) return -103;
      if (P.r1[l] >= m || P.r2[l] >= m) return -104;
    }
    for (uint32_t l = 0; l < L; l++) {
      u128 v = 1;
      for (uint32_t j = 0; j < K; j++) v = v * (p[j] % q[l]) % q[l];
      if (P.pq[l] != (uint64_t)v || P.pq[l] == 0) return -105;
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

// apply's statuses, in nttmul_ksntt_mac_device's order; w_hat and c0_hat are not arguments of it
static int check_calls() {
  int one = 0;
  const void *a = &one;
  const uint32_t n = 256;
  // exactly `rots` entries on the heap: a read past the caller's list is a report
  for (uint32_t rots = 1; rots <= NTTMUL_HOIST_MAX_ROTS; rots++) {
    uint32_t *k = (uint32_t *)malloc(sizeof(uint32_t) * rots), kv[NTTMUL_HOIST_MAX_ROTS];
    CHECK(k);
    for (uint32_t r = 0; r < rots; r++) k[r] = 2 * r + 1;
    CHECK(lintrans_apply_status(true, n, a, a, a, k, rots, 1, 1, 1, kv) == NTTMUL_OK);
    for (uint32_t r = 0; r < NTTMUL_HOIST_MAX_ROTS; r++) CHECK(kv[r] == (r < rots ? 2 * r + 1 : 1));
    CHECK(lintrans_apply_status(true, n, nullptr, nullptr, nullptr, k, rots, 0, 1, 2, kv) ==
          NTTMUL_OK);
    // each refusal with everything after it in the order wrong as well: the first one decides
    CHECK(lintrans_apply_status(false, n, a, a, a, k, rots, 1, 1, 1, kv) == NTTMUL_EINVAL);
    CHECK(lintrans_apply_status(true, n, a, a, a, k, rots, 1, 0, 1, kv) == NTTMUL_EINVAL);  // terms
    CHECK(lintrans_apply_status(true, n, a, a, a, k, rots, 1, 1, 0, kv) == NTTMUL_EINVAL);  // comps
    CHECK(lintrans_apply_status(true, n, a, a, a, k, rots, 1, 1, NTTMUL_MACN_MAX_COMPS + 1, kv) ==
          NTTMUL_EINVAL);
    CHECK(lintrans_apply_status(true, n, a, a, a, k, 0, 1, 1, 1, kv) == NTTMUL_EINVAL);     // rots
    CHECK(lintrans_apply_status(true, n, a, a, a, nullptr, rots, 1, 1, 1, kv) == NTTMUL_EINVAL);
    CHECK(lintrans_apply_status(true, n, a, a, a, nullptr, NTTMUL_HOIST_MAX_ROTS + 1, 1, 1, 1,
                                kv) == NTTMUL_EINVAL);              // the count before the list
    k[rots - 1] = 2 * n + 1;                                        // >= 2n
    CHECK(lintrans_apply_status(true, n, a, a, a, k, rots, 1, 1, 1, kv) == NTTMUL_EINVAL);
    CHECK(lintrans_apply_status(true, n, a, a, a, k, rots, 0, 1, 1, kv) == NTTMUL_EINVAL);  // batch 0
    k[rots - 1] = 2 * n - 1;
    CHECK(lintrans_apply_status(true, n, a, a, a, k, rots, 1, 1, 1, kv) == NTTMUL_OK);
    k[0] = 4;                                                       // even
    CHECK(lintrans_apply_status(true, n, a, a, a, k, rots, 1, 1, 1, kv) == NTTMUL_EINVAL);
    k[0] = 0;
    CHECK(lintrans_apply_status(true, n, a, a, a, k, rots, 1, 1, 1, kv) == NTTMUL_EINVAL);
    k[0] = 1;
    for (int mask = 0; mask < 7; mask++)                            // a NULL operand, batch > 0
      CHECK(lintrans_apply_status(true, n, mask & 1 ? a : nullptr, mask & 2 ? a : nullptr,
                                  mask & 4 ? a : nullptr, k, rots, 1, 1, 1, kv) == NTTMUL_EINVAL);
    free(k);
  }
  return 0;
}

// one launch's workgroups over a block of one byte per (entry, limb, slot range) of c_hat: every
// byte is written exactly once, dead slices read entry (slice) 0 and never store
static int walk(size_t batch, uint32_t logn, uint32_t M, bool slots, uint32_t v) {
  const LtGrid G = lintrans_grid(batch, logn, slots, v);
  const uint32_t lgs = logn - 8;
  const size_t ranges = (size_t)1 << lgs;
  CHECK(G.units == (slots ? batch * ranges : batch));
  CHECK(G.groups == (G.units + v - 1) / v && G.tail == G.units % v && G.ok);
  CHECK(G.wgx == (slots ? G.groups : G.groups * ranges));
  if (!batch) {
    CHECK(G.wgx == 0 && G.groups == 0 && G.tail == 0);
    return 0;
  }
  uint8_t *c = (uint8_t *)calloc(batch * M * ranges, 1), *a = (uint8_t *)calloc(batch * ranges, 1);
  CHECK(c && a);
  size_t dead = 0;
  for (uint32_t l = 0; l < M; l++)
    for (size_t x = 0; x < G.wgx; x++)
      for (uint32_t s = 0; s < v; s++) {
        size_t p, range;
        bool live;
        if (slots) {                                               // k_ksntt_mac's slicing
          const size_t u = x * v + s;
          live = u < G.units;
          const size_t ul = live ? u : 0;
          p = ul >> lgs;
          range = ul & (ranges - 1);
        } else {                                                   // the library's
          const size_t e = (x >> lgs) * v + s;                     // the range is the faster index
          live = e < G.units;
          p = live ? e : 0;
          range = x & (ranges - 1);
        }
        CHECK(p < batch && range < ranges);
        a[p * ranges + range] |= 1;                                // a read of a_hat: in bounds
        if (live) c[(p * M + l) * ranges + range]++;
        else dead++;
      }
  for (size_t i = 0; i < batch * M * ranges; i++) CHECK(c[i] == 1);
  for (size_t i = 0; i < batch * ranges; i++) CHECK(a[i] == 1);
  CHECK(dead == (G.groups * v - G.units) * M * (slots ? 1 : ranges));
  free(c);
  free(a);
  return 0;
}

int main() {
  if (check_create() || check_calls()) return 1;
  int walks = 0;
  const uint32_t V = kLtSlices;
  CHECK(V == 4);
  for (uint32_t logn : {8u, 9u, 12u, 13u, 16u})
    for (size_t batch : {(size_t)0, (size_t)1, (size_t)V - 1, (size_t)V, (size_t)V + 1,
                         (size_t)2 * V - 1, (size_t)33})
      for (uint32_t M : {2u, 6u})
        for (int slots = 0; slots <= 1; slots++)
          for (uint32_t v : {V, 8u}) {
            if (walk(batch, logn, M, slots != 0, v)) return 1;
            walks++;
          }
  // the partial last workgroup, in the header's words
  CHECK(lintrans_grid(V + 1, 8).groups == 2 && lintrans_grid(V + 1, 8).tail == 1);
  CHECK(lintrans_grid(2 * V - 1, 12).wgx == 32 && lintrans_grid(2 * V - 1, 12).tail == V - 1);
  CHECK(lintrans_grid(5, 16).wgx == 512);
  // sizes past 2^32 words.  No memory is touched: the counts and offsets alone
  {
    const uint32_t n = 65536, L = 60, K = 4;
    const size_t batch = 2048;
    size_t words[5];
    lintrans_words(L, K, n, batch, 4, 16, 2, words);
    CHECK(words[0] == batch * 2 * 64 * 65536 && words[0] > ((size_t)1 << 32));
    CHECK(words[1] == batch * 4 * 64 * 65536 && words[1] == (size_t)1 << 35);
    CHECK(words[2] == (size_t)16 * 2 * 4 * 64 * 65536 && words[3] == (size_t)16 * 64 * 65536);
    CHECK(words[4] == batch * 60 * 65536 && words[4] > ((size_t)1 << 32));
    // the last entry's polynomial offsets as the kernel forms them, (p terms M + l) n and
    // (p comps M + l) n
    const size_t p = batch - 1, a_off = ((p * 4 * 64 + 63) << 16), c_off = ((p * 2 * 64 + 63) << 16);
    CHECK(a_off + (size_t)3 * 64 * n + n == words[1] && c_off + (size_t)64 * n + n == words[0]);
    const LtGrid G = lintrans_grid(batch, 16);
    CHECK(G.ok && G.wgx == (size_t)512 * 256 && G.tail == 0);
    // a batch whose workgroups no longer fit a grid dimension is refused, not wrapped
    CHECK(!lintrans_grid((size_t)1 << 34, 16).ok && lintrans_grid((size_t)1 << 24, 16).ok);
    CHECK(!lintrans_grid((size_t)1 << 34, 8, true).ok && lintrans_grid((size_t)1 << 32, 8).ok);
  }
  printf("lintrans sanitizer run ok: %d walks\n", walks);
  return 0;
}
