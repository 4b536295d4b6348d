// macn_san.cpp — the host-only arithmetic behind include/nttmul_macn.h under ASan / UBSan, with a
// main of its own (tests/test_macn_sanitizers.py): csrc/macn_plan.hpp macn_args, the status every
// call decides before any device access, and csrc/subbatch.hpp mp_chunk / mp_subs / mp_sub, the
// sub-batch rule csrc/rnsmp.cpp run applies to every multi-pass operation.  Neither header needs a
// device.  The rule is checked against its definition, computed here another way (a linear search
// for the largest count that fits), and a call's sub-batches are walked through heap blocks of
// exactly the operands' sizes, one byte per polynomial, so a sub-batch that starts or ends outside
// its operand is a report; the byte offsets rnsmp.cpp forms from a sub-batch (p times the bytes
// per batch entry) are computed for shapes where they pass 2^32 words and 2^35 bytes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "macn_plan.hpp"
#include "subbatch.hpp"

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
  for (uint32_t comps = 0; comps <= NTTMUL_MACN_MAX_COMPS + 2; comps++)
    for (uint32_t terms = 0; terms <= 3; terms++)
      for (size_t batch = 0; batch <= 2; batch++)
        for (int mask = 0; mask < 8; mask++)
          for (int ctx = 0; ctx <= 1; ctx++) {
            const void *c = mask & 1 ? p : nullptr, *a = mask & 2 ? p : nullptr,
                       *b = mask & 4 ? p : nullptr;
            const bool bad = !ctx || !terms || !comps || comps > NTTMUL_MACN_MAX_COMPS ||
                             (batch && mask != 7);
            CHECK(macn_args(ctx, c, a, b, batch, terms, comps) ==
                  (bad ? NTTMUL_EINVAL : NTTMUL_OK));
          }
  // a batch that does not fit 32 bits changes nothing
  CHECK(macn_args(true, p, p, p, (size_t)1 << 40, 1, 2) == NTTMUL_OK);
  CHECK(macn_args(true, p, nullptr, p, (size_t)1 << 40, 1, 2) == NTTMUL_EINVAL);
  CHECK(macn_args(true, p, p, p, 1, UINT32_MAX, 2) == NTTMUL_OK);
  CHECK(macn_args(true, p, p, p, 1, 1, UINT32_MAX) == NTTMUL_EINVAL);
  return 0;
}

// one call's sub-batches over blocks of one byte per (polynomial, term) of a and per
// (polynomial, component) of c: every byte of both is touched exactly once
static int walk(size_t limit, size_t poly, uint32_t terms, uint32_t comps, size_t batch,
                size_t *count) {
  const size_t in = poly * terms, out = poly * comps;
  const size_t chunk = mp_chunk(limit, in, out, batch);
  // the definition: the largest count in 1 .. batch whose buffers both fit, else 1
  size_t want = 1;
  for (size_t k = 1; k <= batch; k++)
    if (k * in <= limit && k * out <= limit) want = k;
  CHECK(chunk == want);
  uint8_t *a = (uint8_t *)calloc(batch * terms, 1), *c = (uint8_t *)calloc(batch * comps, 1);
  CHECK(a && c);
  const size_t subs = mp_subs(batch, chunk);
  size_t done = 0;
  for (size_t k = 0; k < subs; k++) {
    const MpSub u = mp_sub(batch, chunk, k);
    CHECK(u.p == done && u.cnt >= 1 && u.cnt <= chunk && u.p + u.cnt <= batch);
    CHECK(k + 1 == subs || u.cnt == chunk);
    for (size_t i = 0; i < u.cnt * terms; i++) a[u.p * terms + i]++;
    for (size_t i = 0; i < u.cnt * comps; i++) c[u.p * comps + i]++;
    done += u.cnt;
  }
  CHECK(done == batch);
  for (size_t i = 0; i < batch * terms; i++) CHECK(a[i] == 1);
  for (size_t i = 0; i < batch * comps; i++) CHECK(c[i] == 1);
  free(a);
  free(c);
  *count = subs;
  return 0;
}

int main() {
  if (check_args()) return 1;
  int walks = 0;
  size_t subs = 0;
  // tests/macn_cases.py SUBBATCH: n = 8192, three 32-bit limbs, scratch_mb = 1
  const size_t mib = (size_t)1 << 20, poly = (size_t)3 * 8192 * 4;
  if (walk(mib, poly, 3, 2, 8, &subs)) return 1;
  CHECK(subs == 3 && mp_chunk(mib, poly * 3, poly * 2, 8) == 3);
  if (walk(mib, poly, 1, 2, 11, &subs)) return 1;
  CHECK(subs == 3 && mp_chunk(mib, poly, poly * 2, 11) == 5);
  CHECK(mp_chunk(mib, poly, poly, 11) == 10);                  // mac_ntt's own rule at comps = 1
  walks += 2;
  // every small shape: limits around the polynomial's size, one polynomial above the limit
  for (size_t limit : {(size_t)1, (size_t)7, (size_t)64, (size_t)1000})
    for (size_t pb : {(size_t)1, (size_t)3, (size_t)64, (size_t)65, (size_t)2000})
      for (uint32_t terms = 1; terms <= 7; terms += 2)
        for (uint32_t comps = 1; comps <= NTTMUL_MACN_MAX_COMPS; comps++)
          for (size_t batch : {(size_t)1, (size_t)2, (size_t)17, (size_t)100}) {
            if (walk(limit, pb, terms, comps, batch, &subs)) return 1;
            walks++;
          }
  // the largest shapes: 64 limbs of n = 65536 on 64-bit words, 32 MiB per polynomial; scratch of
  // 4095 MiB; a batch whose operands pass 2^32 words.  No memory is touched: the offsets alone
  {
    const size_t big = (size_t)64 * 65536 * 8, limit = (size_t)4095 << 20;
    const uint32_t terms = 16, comps = 2;
    const size_t batch = 4096;                                  // a: 2^12 * 2^4 * 2^22 = 2^38 words
    const size_t chunk = mp_chunk(limit, big * terms, big * comps, batch);
    CHECK(chunk == 7);                                          // 4095 MiB / 512 MiB
    const size_t n_subs = mp_subs(batch, chunk);
    CHECK(n_subs == 586);
    const MpSub last = mp_sub(batch, chunk, n_subs - 1);
    CHECK(last.p == 4095 && last.cnt == 1);
    const size_t a_off = last.p * big * terms, c_off = last.p * big * comps;
    CHECK(a_off / 8 > ((size_t)1 << 32) && a_off == (size_t)4095 << 29);
    CHECK(c_off / 8 > ((size_t)1 << 32) && c_off == (size_t)4095 << 26);
    CHECK(a_off + last.cnt * big * terms == batch * big * terms);
    const MpSub mid = mp_sub(batch, chunk, 300);
    CHECK(mid.p == 2100 && mid.cnt == 7 && mid.p * big * terms == (size_t)2100 << 29);
    // one polynomial above the limit: sub-batches of one
    CHECK(mp_chunk((size_t)1 << 20, big * terms, big * comps, batch) == 1);
    CHECK(mp_subs(batch, 1) == batch);
  }
  printf("macn sanitizer run ok: %d walks\n", walks);
  return 0;
}
