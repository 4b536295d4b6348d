// hoist_san.cpp — the host-only arithmetic behind include/nttmul_hoist.h under ASan / UBSan, with a
// main of its own (tests/test_hoist_sanitizers.py): csrc/hoist_plan.hpp hoist_args, the status
// every call decides before any device access and its order, and csrc/subbatch.hpp mp_unit_chunk,
// mp_unit_words, mp_subs and mp_sub, the very functions csrc/rnsmp.cpp run_units calls for the
// sub-batches of output units.  Neither header
// needs a device.  The rule is checked against its definition, computed here another way (a linear
// search for the largest count that fits), and a call's sub-batches are walked through a heap block
// of exactly c's size, one byte per (unit, component), with every unit's (p, r) formed as the
// kernel forms it and the words of a_hat and b_hat it reads bounded by blocks of the operands'
// sizes, so a sub-batch that starts or ends outside an operand is a report; the byte offsets
// rnsmp.cpp forms from a sub-batch are computed for shapes where they pass 2^32 words.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hoist_plan.hpp"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      return 1;                                                   \
    }                                                             \
  } while (0)

using namespace nttmul;

static int check_args() {
  int one = 0;
  const void *p = &one;
  const uint32_t n = 256;
  uint32_t kv[NTTMUL_HOIST_MAX_ROTS];
  // exactly NTTMUL_HOIST_MAX_ROTS entries on the heap: a read past rots' entries is a report
  uint32_t *full = (uint32_t *)malloc(sizeof(uint32_t) * NTTMUL_HOIST_MAX_ROTS);
  CHECK(full);
  for (uint32_t r = 0; r < NTTMUL_HOIST_MAX_ROTS; r++) full[r] = 2 * r + 1;
  for (uint32_t comps = 0; comps <= NTTMUL_MACN_MAX_COMPS + 1; comps++)
    for (uint32_t rots : {0u, 1u, 3u, 16u, 17u})
      for (uint32_t terms = 0; terms <= 2; terms++)
        for (size_t batch = 0; batch <= 1; batch++)
          for (int mask = 0; mask < 16; mask++)
            for (int ctx = 0; ctx <= 1; ctx++) {
              const void *c = mask & 1 ? p : nullptr, *a = mask & 2 ? p : nullptr,
                         *b = mask & 4 ? p : nullptr;
              const uint32_t *k = mask & 8 ? full : nullptr;
              const bool bad = !ctx || !terms || !comps || comps > NTTMUL_MACN_MAX_COMPS ||
                               !rots || rots > NTTMUL_HOIST_MAX_ROTS || !k ||
                               (batch && (mask & 7) != 7);
              CHECK(hoist_args(ctx, n, c, a, b, k, rots, batch, terms, comps, kv) ==
                    (bad ? NTTMUL_EINVAL : NTTMUL_OK));
              if (!bad)
                for (uint32_t r = 0; r < NTTMUL_HOIST_MAX_ROTS; r++)
                  CHECK(kv[r] == (r < rots ? full[r] : 1u));
            }
  free(full);
  // the rotations: odd and below 2n; only the first rots entries are read (a block of rots)
  for (uint32_t rots = 1; rots <= NTTMUL_HOIST_MAX_ROTS; rots++)
    for (uint32_t bad : {0u, 2u, 2 * n, 2 * n + 1, UINT32_MAX}) {
      uint32_t *k = (uint32_t *)malloc(sizeof(uint32_t) * rots);
      CHECK(k);
      for (uint32_t r = 0; r < rots; r++) k[r] = 2 * n - 1 - 2 * r;
      CHECK(hoist_args(true, n, p, p, p, k, rots, 1, 1, 2, kv) == NTTMUL_OK);
      k[rots - 1] = bad;
      CHECK(hoist_args(true, n, p, p, p, k, rots, 1, 1, 2, kv) == NTTMUL_EINVAL);
      CHECK(hoist_args(true, n, nullptr, nullptr, nullptr, k, rots, 0, 1, 2, kv) == NTTMUL_EINVAL);
      free(k);
    }
  // the order: a bad k is reported with NULL operands too, and NULL operands with a good k
  const uint32_t good[1] = {5}, even[1] = {4};
  CHECK(hoist_args(true, n, nullptr, p, p, even, 1, 1, 1, 1, kv) == NTTMUL_EINVAL);
  CHECK(hoist_args(true, n, nullptr, p, p, good, 1, 1, 1, 1, kv) == NTTMUL_EINVAL);
  CHECK(hoist_args(true, n, nullptr, nullptr, nullptr, good, 1, 0, 1, 1, kv) == NTTMUL_OK);
  CHECK(hoist_k_ok(65536, 131071) && !hoist_k_ok(65536, 131072) && !hoist_k_ok(65536, 131073));
  // a batch that does not fit 32 bits changes nothing
  CHECK(hoist_args(true, n, p, p, p, good, 1, (size_t)1 << 40, UINT32_MAX, 2, kv) == NTTMUL_OK);
  return 0;
}

// one call's sub-batches over a block of one byte per (unit, component) of c: every byte is touched
// exactly once, and every unit's a_hat polynomials and b_hat polynomials lie inside their operands
static int walk(size_t limit, size_t poly, uint32_t terms, uint32_t comps, size_t batch,
                uint32_t rots, size_t *count) {
  const size_t units = batch * rots, chunk = mp_unit_chunk(limit, poly, comps, batch * rots);
  size_t want = 1;
  for (size_t k = 1; k <= units; k++)
    if (k * poly * comps <= limit) want = k;
  CHECK(chunk == want);
  size_t words[3];
  mp_unit_words(1, 1, batch, terms, rots, comps, words);          // polynomials of one word
  CHECK(words[0] == units * comps && words[1] == batch * terms &&
        words[2] == (size_t)rots * comps * terms);
  uint8_t *c = (uint8_t *)calloc(words[0], 1), *a = (uint8_t *)calloc(words[1], 1),
          *b = (uint8_t *)calloc(words[2], 1);
  CHECK(a && b && c);
  const size_t subs = mp_subs(units, chunk);
  size_t done = 0;
  for (size_t k = 0; k < subs; k++) {
    const MpSub u = mp_sub(units, chunk, k);
    CHECK(u.p == done && u.cnt >= 1 && u.cnt <= chunk && u.p + u.cnt <= units);
    CHECK(k + 1 == subs || u.cnt == chunk);
    uint8_t *cu = c + u.p * comps;                              // the sub-batch's c
    for (size_t v = 0; v < u.cnt; v++) {
      const size_t ug = u.p + v, p = ug / rots, r = ug - p * rots;   // as k_rnsmp_hoist forms them
      CHECK(p < batch && r < rots);
      for (uint32_t i = 0; i < comps; i++) {
        cu[v * comps + i]++;
        for (uint32_t t = 0; t < terms; t++) b[(r * comps + i) * terms + t] |= 1;
      }
      for (uint32_t t = 0; t < terms; t++) a[p * terms + t] |= 1;
    }
    done += u.cnt;
  }
  CHECK(done == units);
  for (size_t i = 0; i < words[0]; i++) CHECK(c[i] == 1);
  for (size_t i = 0; i < words[1]; i++) CHECK(a[i] == 1);
  for (size_t i = 0; i < words[2]; i++) CHECK(b[i] == 1);
  free(a);
  free(b);
  free(c);
  *count = subs;
  return 0;
}

int main() {
  if (check_args()) return 1;
  int walks = 0;
  size_t subs = 0;
  // tests/hoist_cases.py SUBBATCH: n = 8192, three 32-bit limbs, scratch_mb = 1
  const size_t mib = (size_t)1 << 20, poly = (size_t)3 * 8192 * 4;
  if (walk(mib, poly, 2, 2, 4, 3, &subs)) return 1;
  CHECK(subs == 3 && mp_unit_chunk(mib, poly, 2, 4 * 3) == 5);
  if (walk(mib, poly, 1, 1, 7, 3, &subs)) return 1;
  CHECK(subs == 3 && mp_unit_chunk(mib, poly, 1, 7 * 3) == 10);
  if (walk(mib, (size_t)3 * 65536 * 8, 1, 1, 2, 2, &subs)) return 1;
  CHECK(subs == 4);
  walks += 3;
  // every small shape: limits around the polynomial's size, one unit above the limit
  for (size_t limit : {(size_t)1, (size_t)7, (size_t)64, (size_t)1000})
    for (size_t pb : {(size_t)1, (size_t)3, (size_t)64, (size_t)65, (size_t)2000})
      for (uint32_t terms = 1; terms <= 7; terms += 3)
        for (uint32_t comps = 1; comps <= NTTMUL_MACN_MAX_COMPS; comps++)
          for (uint32_t rots : {1u, 3u, 16u})
            for (size_t batch : {(size_t)1, (size_t)2, (size_t)17}) {
              if (walk(limit, pb, terms, comps, batch, rots, &subs)) return 1;
              walks++;
            }
  // the largest shapes: 64 limbs of n = 65536 on 64-bit words, 32 MiB per polynomial; scratch of
  // 4095 MiB; 16 rotations of a batch whose c passes 2^32 words.  No memory is touched: the
  // offsets alone
  {
    const size_t big = (size_t)64 * 65536 * 8, limit = (size_t)4095 << 20;
    const uint32_t comps = 2, rots = 16, terms = 16;
    const size_t batch = 512, units = batch * rots;             // c: 2^13 * 2 * 2^22 = 2^36 words
    const size_t chunk = mp_unit_chunk(limit, big, comps, units);
    CHECK(chunk == 63);                                         // 4095 MiB / 64 MiB
    const size_t n_subs = mp_subs(units, chunk);
    CHECK(n_subs == 131);
    const MpSub last = mp_sub(units, chunk, n_subs - 1);
    CHECK(last.p == 8190 && last.cnt == 2);
    const size_t c_off = last.p * big * comps;                  // run_units: u.p * cunit
    CHECK(c_off / 8 > ((size_t)1 << 32) && c_off == (size_t)8190 << 26);
    CHECK(c_off + last.cnt * big * comps == units * big * comps);
    size_t words[3];
    mp_unit_words(64, 65536, batch, terms, rots, comps, words);
    CHECK(words[0] == (size_t)1 << 36 && words[1] == (size_t)1 << 35 &&
          words[2] == (size_t)1 << 31);
    const MpSub mid = mp_sub(units, chunk, 100);
    CHECK(mid.p == 6300 && mid.cnt == 63 && mid.p / rots == 393 && mid.p % rots == 12);
    // the last unit's a_hat polynomials end with the operand
    const size_t p = (units - 1) / rots;
    CHECK(p == batch - 1 && ((p * terms + terms) * 64 << 16) == words[1]);
    // one unit above the limit: sub-batches of one
    CHECK(mp_unit_chunk((size_t)1 << 20, big, comps, units) == 1);
    CHECK(mp_subs(units, 1) == units);
  }
  printf("hoist sanitizer run ok: %d walks\n", walks);
  return 0;
}
