// ksntt_san.cpp — the host-only part of include/nttmul_ksntt.h under ASan / UBSan, with a main of
// its own (tests/test_ksntt_sanitizers.py): csrc/ksntt_plan.hpp ksntt_validate over
// csrc/ks_plan.cpp and csrc/basis.cpp (create's statuses and their order), the two calls'
// statuses in the header's order, the digit table with short last digits, and ksntt_shape over
// csrc/subbatch.hpp for both scratch choices, the very functions csrc/ksntt.cpp calls.  None of
// them needs a device.  The sub-batch rule is checked against its definition, computed here
// another way (a linear search for the largest count that fits), and a call's sub-batches are
// walked through heap blocks of exactly the operands' sizes, one byte per polynomial and limb,
// with the offsets ksntt.cpp run_modup forms and the targets ks_target forms, so a sub-batch or a
// digit that starts or ends outside an operand is a report; the byte offsets are computed for
// shapes where they pass 2^32 words.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ksntt_plan.hpp"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      return 1;                                                   \
    }                                                             \
  } while (0)

using namespace nttmul;

// primes = 1 mod 2^17 (tests/dispatch_cases.py, tests/rnsmp_cases.py): two below 2^31, two of 62
// and 61 bits, one in [2^31, 2^32)
static const uint64_t kQ31 = 2013265921ull, kQ31b = 2147352577ull;
static const uint64_t kQ62 = 0x3FFFFFFFFFE80001ull, kQ61 = 2305843009211596801ull;
static const uint64_t kQ32 = 4293918721ull;

static int status(uint32_t n, const uint64_t *q, uint32_t L, const uint64_t *p, uint32_t K,
                  uint32_t alpha, uint32_t flags = 0, uint64_t pq = 0,
                  size_t size = sizeof(nttmul_params)) {
  nttmul_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.n = n;
  prm.q = pq;
  prm.ndev = 1;
  prm.flags = flags;
  KsPlan P;
  const int st = ksntt_validate(&prm, size, q, L, p, K, alpha, &P);
  if (st == NTTMUL_OK) {
    if (P.L != L || P.K != K || P.alpha != alpha || P.dnum != ksntt_digits(L, alpha)) return -100;
    ks_constants(&P);  // every table at its size: inv [L], w [L][L + K]
    if (P.inv.size() != L || P.w.size() != (size_t)L * (L + K)) return -101;
  }
  return st;
}

static int check_create() {
  const uint64_t q32[2] = {kQ31, kQ31b}, q64[2] = {kQ62, kQ61};
  for (uint32_t n : {256u, 4096u, 8192u, 65536u}) {
    CHECK(status(n, q32, 1, q32 + 1, 1, 1) == NTTMUL_OK);
    CHECK(status(n, q64, 1, q64 + 1, 1, 1) == NTTMUL_OK);
    CHECK(status(n, q32, 0, q32 + 1, 1, 1) == NTTMUL_EINVAL);          // q_limbs = 0
    CHECK(status(n, q32, 1, q32 + 1, 0, 1) == NTTMUL_EINVAL);          // p_limbs = 0
    CHECK(status(n, nullptr, 1, q32 + 1, 1, 1) == NTTMUL_EINVAL);
    CHECK(status(n, q32, 1, nullptr, 1, 1) == NTTMUL_EINVAL);
    CHECK(status(n, q32, 1, q32, 1, 1) == NTTMUL_EINVAL);              // a prime in both bases
    CHECK(status(n, q32, 1, q32 + 1, 1, 1, 0, kQ31) == NTTMUL_EINVAL); // params->q
    CHECK(status(n, q32, 1, q32 + 1, 1, 1, 0, 0, 4) == NTTMUL_EINVAL); // params size
    CHECK(status(n, q32, 1, q32 + 1, 1, 0) == NTTMUL_EINVAL);          // digit_limbs = 0
    CHECK(status(n, q32, 1, q32 + 1, 1, 2) == NTTMUL_EINVAL);          // digit_limbs > q_limbs
    CHECK(status(n, q32, 1, q32 + 1, 1, 1, NTTMUL_FLAG_CYCLIC) == NTTMUL_EUNSUPPORTED);
    CHECK(status(n, q32, 1, q64, 1, 1) == NTTMUL_EUNSUPPORTED);        // mixed classes
    CHECK(status(n, q64, 1, q32, 1, 1) == NTTMUL_EUNSUPPORTED);
    CHECK(status(n, q32, 1, &kQ32, 1, 1) == NTTMUL_EUNSUPPORTED);      // [2^31, 2^32)
    const uint64_t comp[1] = {kQ31 + 2};
    CHECK(status(n, q32, 1, comp, 1, 1) == NTTMUL_EINVAL);             // not prime
    // the order: every EINVAL, the digit width's too, before any EUNSUPPORTED
    CHECK(status(n, &kQ32, 1, comp, 1, 1) == NTTMUL_EINVAL);
    CHECK(status(n, q32, 1, q32 + 1, 1, 1, NTTMUL_FLAG_CYCLIC, kQ31) == NTTMUL_EINVAL);
    CHECK(status(n, q32, 1, q32 + 1, 1, 0, NTTMUL_FLAG_CYCLIC) == NTTMUL_EINVAL);
    CHECK(status(n, q32, 1, &kQ32, 1, 2) == NTTMUL_EINVAL);
  }
  CHECK(status(128, q32, 1, q32 + 1, 1, 1) == NTTMUL_EINVAL);
  CHECK(status(10000, q32, 1, q32 + 1, 1, 1) == NTTMUL_EINVAL);
  CHECK(status(131072, q32, 1, q32 + 1, 1, 1) == NTTMUL_EINVAL);       // 2^18 does not divide q - 1
  // limb counts: exactly NTTMUL_RNS_MAX_LIMBS entries on the heap per basis, so a read past a
  // basis' own count is a report
  uint64_t *many = (uint64_t *)malloc(sizeof(uint64_t) * NTTMUL_RNS_MAX_LIMBS);
  CHECK(many);
  for (uint32_t i = 0; i < NTTMUL_RNS_MAX_LIMBS; i++) many[i] = 3 + i;
  CHECK(status(256, many, NTTMUL_RNS_MAX_LIMBS + 1, q32, 1, 1) == NTTMUL_EINVAL);
  CHECK(status(256, q32, 1, many, NTTMUL_RNS_MAX_LIMBS + 1, 1) == NTTMUL_EINVAL);
  CHECK(status(256, many, NTTMUL_RNS_MAX_LIMBS, q32, 1, 1) == NTTMUL_EINVAL);
  free(many);
  return 0;
}

// the calls: modup's two statuses, mac's in nttmul_rns_hoist_ntt_device's order
static int check_calls() {
  int one = 0;
  const void *a = &one;
  for (int ctx = 0; ctx <= 1; ctx++)
    for (size_t batch = 0; batch <= 2; batch++)
      for (int mask = 0; mask < 4; mask++) {
        const void *out = mask & 1 ? a : nullptr, *x = mask & 2 ? a : nullptr;
        const bool bad = !ctx || (batch && mask != 3);
        CHECK(ksntt_modup_status(ctx, out, x, batch) == (bad ? NTTMUL_EINVAL : NTTMUL_OK));
      }
  CHECK(ksntt_modup_status(true, a, a, (size_t)1 << 40) == NTTMUL_OK);
  const uint32_t n = 256;
  // exactly `rots` entries on the heap: a read past the caller's list is a report
  for (uint32_t rots = 1; rots <= NTTMUL_HOIST_MAX_ROTS; rots++) {
    uint32_t *k = (uint32_t *)malloc(sizeof(uint32_t) * rots), kv[NTTMUL_HOIST_MAX_ROTS];
    CHECK(k);
    for (uint32_t r = 0; r < rots; r++) k[r] = 2 * r + 1;
    CHECK(ksntt_mac_status(true, n, a, a, a, k, rots, 1, 1, 1, kv) == NTTMUL_OK);
    for (uint32_t r = 0; r < NTTMUL_HOIST_MAX_ROTS; r++) CHECK(kv[r] == (r < rots ? 2 * r + 1 : 1));
    CHECK(ksntt_mac_status(true, n, nullptr, nullptr, nullptr, k, rots, 0, 1, 2, kv) == NTTMUL_OK);
    // each refusal with everything after it in the order wrong as well: the first one decides
    CHECK(ksntt_mac_status(false, n, a, a, a, k, rots, 1, 1, 1, kv) == NTTMUL_EINVAL);
    CHECK(ksntt_mac_status(true, n, a, a, a, k, rots, 1, 0, 1, kv) == NTTMUL_EINVAL);   // terms
    CHECK(ksntt_mac_status(true, n, a, a, a, k, rots, 1, 1, 0, kv) == NTTMUL_EINVAL);   // comps
    CHECK(ksntt_mac_status(true, n, a, a, a, k, rots, 1, 1, NTTMUL_MACN_MAX_COMPS + 1, kv) ==
          NTTMUL_EINVAL);
    CHECK(ksntt_mac_status(true, n, a, a, a, k, 0, 1, 1, 1, kv) == NTTMUL_EINVAL);      // rots
    CHECK(ksntt_mac_status(true, n, a, a, a, nullptr, rots, 1, 1, 1, kv) == NTTMUL_EINVAL);
    CHECK(ksntt_mac_status(true, n, a, a, a, nullptr, NTTMUL_HOIST_MAX_ROTS + 1, 1, 1, 1, kv) ==
          NTTMUL_EINVAL);                                             // the count before the list
    k[rots - 1] = 2 * n + 1;                                          // >= 2n
    CHECK(ksntt_mac_status(true, n, a, a, a, k, rots, 1, 1, 1, kv) == NTTMUL_EINVAL);
    CHECK(ksntt_mac_status(true, n, a, a, a, k, rots, 0, 1, 1, kv) == NTTMUL_EINVAL);   // at batch 0 too
    k[rots - 1] = 2 * n - 1;
    CHECK(ksntt_mac_status(true, n, a, a, a, k, rots, 1, 1, 1, kv) == NTTMUL_OK);
    k[0] = 4;                                                         // even
    CHECK(ksntt_mac_status(true, n, a, a, a, k, rots, 1, 1, 1, kv) == NTTMUL_EINVAL);
    k[0] = 0;
    CHECK(ksntt_mac_status(true, n, a, a, a, k, rots, 1, 1, 1, kv) == NTTMUL_EINVAL);
    k[0] = 1;
    for (int mask = 0; mask < 7; mask++)                              // a NULL operand, batch > 0
      CHECK(ksntt_mac_status(true, n, mask & 1 ? a : nullptr, mask & 2 ? a : nullptr,
                             mask & 4 ? a : nullptr, k, rots, 1, 1, 1, kv) == NTTMUL_EINVAL);
    free(k);
  }
  return 0;
}

// the digit table: the digits tile [0, L) in order, all of alpha limbs but a last one of 1 .. alpha
static int check_digits() {
  int tables = 0;
  for (uint32_t L = 1; L <= NTTMUL_RNS_MAX_LIMBS; L++)
    for (uint32_t alpha = 1; alpha <= L; alpha++) {
      const uint32_t dnum = ksntt_digits(L, alpha);
      CHECK(dnum >= 1 && (dnum - 1) * alpha < L && dnum * alpha >= L);
      // one byte per limb of Q on the heap: a digit past L is a report
      uint8_t *seen = (uint8_t *)calloc(L, 1);
      CHECK(seen);
      uint32_t next = 0;
      for (uint32_t d = 0; d < dnum; d++) {
        const KsnttDigit D = ksntt_digit(L, alpha, d);
        CHECK(D.first == next && D.len >= 1 && D.len <= alpha);
        CHECK(d + 1 == dnum || D.len == alpha);
        for (uint32_t i = 0; i < D.len; i++) seen[D.first + i]++;
        for (uint32_t m = 0; m < L + 2; m++)
          CHECK(ksntt_own(L, alpha, d, m) == (m >= D.first && m < D.first + D.len));
        next += D.len;
      }
      CHECK(next == L);
      for (uint32_t i = 0; i < L; i++) CHECK(seen[i] == 1);
      free(seen);
      tables++;
    }
  CHECK(ksntt_digit(5, 2, 2).first == 4 && ksntt_digit(5, 2, 2).len == 1);     // short last digits
  CHECK(ksntt_digit(12, 5, 2).first == 10 && ksntt_digit(12, 5, 2).len == 2);
  CHECK(ksntt_digit(60, 15, 3).len == 15 && ksntt_digits(60, 15) == 4);
  CHECK(tables == 64 * 65 / 2);
  return 0;
}

// one modup's sub-batches over blocks of one byte per (polynomial, limb) of x_hat and of up_hat:
// every byte of up_hat is written exactly once (the own limbs by a copy, the others by a
// transform), every limb of x_hat is read by the inverse and by its digit's copy, and the scratch
// block of a sub-batch is never indexed past chunk polynomials
static int walk(size_t limit, uint32_t n, uint32_t L, uint32_t K, uint32_t alpha, int bits,
                size_t batch, bool t_scr, size_t *subs) {
  const KsnttShape S = ksntt_shape(limit, n, L, K, alpha, bits, batch, t_scr);
  const uint32_t M = L + K, dnum = ksntt_digits(L, alpha);
  const size_t wb = bits / 8, yb = (size_t)L * n * wb, tb = (size_t)dnum * M * n * wb;
  const size_t per = n > 4096 && t_scr ? tb : yb;
  size_t want = 1;
  for (size_t k = 1; k <= batch; k++)
    if (k * per <= limit) want = k;
  CHECK(S.chunk == want && S.subs == (batch + want - 1) / want);
  CHECK(S.in_words == (size_t)L * n && S.out_words == (size_t)dnum * M * n);
  CHECK(S.y_bytes == yb && S.t_bytes == (n > 4096 && t_scr ? tb : 0));
  uint8_t *x = (uint8_t *)calloc(batch * L, 1), *up = (uint8_t *)calloc(batch * dnum * M, 1);
  uint8_t *y = (uint8_t *)calloc(S.chunk * L, 1);
  CHECK(x && up && y);
  size_t done = 0;
  for (size_t k = 0; k < S.subs; k++) {
    const MpSub u = mp_sub(batch, S.chunk, k);
    CHECK(u.p == done && u.cnt >= 1 && u.cnt <= S.chunk && u.p + u.cnt <= batch);
    CHECK(k + 1 == S.subs || u.cnt == S.chunk);
    CHECK(u.p * S.in_words % n == 0 && u.p * S.out_words % n == 0);
    uint8_t *xu = x + u.p * S.in_words / n, *ou = up + u.p * S.out_words / n;
    for (size_t v = 0; v < u.cnt; v++) {
      for (uint32_t i = 0; i < L; i++) {
        xu[v * L + i]++;                                          // the inverse reads limb i
        y[v * L + i] = 1;
      }
      for (uint32_t dm = 0; dm < dnum * M; dm++) {                // ks_target
        const uint32_t d = dm / M, m = dm - d * M;
        const KsnttDigit D = ksntt_digit(L, alpha, d);
        if (ksntt_own(L, alpha, d, m)) {
          xu[v * L + m]++;                                        // the copy reads x_hat[p][m]
        } else {
          for (uint32_t i = 0; i < D.len; i++) CHECK(y[v * L + D.first + i] == 1);
        }
        ou[(v * dnum + d) * M + m]++;
      }
    }
    done += u.cnt;
  }
  CHECK(done == batch);
  for (size_t i = 0; i < batch * L; i++) CHECK(x[i] == 2);
  for (size_t i = 0; i < batch * dnum * M; i++) CHECK(up[i] == 1);
  free(x);
  free(up);
  free(y);
  *subs = S.subs;
  return 0;
}

int main() {
  if (check_create() || check_calls() || check_digits()) return 1;
  int walks = 0;
  size_t subs = 0;
  const size_t mib = (size_t)1 << 20;
  // tests/ksntt_cases.py SUBBATCH, scratch_mb = 1
  if (walk(mib, 4096, 3, 2, 2, 64, 23, false, &subs)) return 1;
  CHECK(subs == 3 && ksntt_shape(mib, 4096, 3, 2, 2, 64, 23).chunk == 10);
  if (walk(mib, 65536, 2, 1, 1, 32, 5, false, &subs)) return 1;
  CHECK(subs == 3 && ksntt_shape(mib, 65536, 2, 1, 1, 32, 5).chunk == 2);
  // the other scratch choice shrinks the sub-batch above n = 4096 only
  CHECK(ksntt_shape(mib, 65536, 2, 1, 1, 32, 5, true).chunk == 1);
  CHECK(ksntt_shape(mib, 4096, 3, 2, 2, 64, 23, true).chunk == 10);
  walks += 2;
  // the empty batch: no sub-batch
  CHECK(ksntt_shape(mib, 256, 1, 1, 1, 32, 0).subs == 0);
  // every small shape: limits around one polynomial's scratch, one polynomial above the limit
  for (size_t limit : {(size_t)1, (size_t)4096, (size_t)65536, mib})
    for (uint32_t n : {256u, 4096u, 8192u, 65536u})
      for (uint32_t L : {1u, 3u, 5u, 60u})
        for (uint32_t alpha : {1u, 2u, 15u})
          for (int bits : {32, 64})
            for (size_t batch : {(size_t)1, (size_t)2, (size_t)33})
              for (int t_scr = 0; t_scr <= 1; t_scr++) {
                if (alpha > L) continue;
                if (walk(limit, n, L, 2, alpha, bits, batch, t_scr != 0, &subs)) return 1;
                walks++;
              }
  // the largest shapes: 60 + 4 limbs of n = 65536 on 64-bit words in 4 digits, a scratch of
  // 4095 MiB, a batch whose up_hat passes 2^32 words.  No memory is touched: the offsets alone
  {
    const uint32_t n = 65536, L = 60, K = 4, alpha = 15;
    const size_t batch = 2048, limit = (size_t)4095 << 20;
    const KsnttShape S = ksntt_shape(limit, n, L, K, alpha, 64, batch);
    CHECK(S.y_bytes == (size_t)60 << 19 && S.t_bytes == 0);
    CHECK(S.chunk == 136 && S.subs == 16);                      // 4095 MiB / 30 MiB
    const MpSub last = mp_sub(batch, S.chunk, S.subs - 1);
    CHECK(last.p == 2040 && last.cnt == 8);
    const size_t in_off = last.p * S.in_words, out_off = last.p * S.out_words;
    CHECK(in_off > ((size_t)1 << 32) && in_off == (size_t)2040 * 60 * 65536);
    CHECK(out_off > ((size_t)1 << 32) && out_off == (size_t)2040 * 4 * 64 * 65536);
    CHECK(out_off + last.cnt * S.out_words == batch * S.out_words);
    CHECK(batch * S.out_words == (size_t)1 << 35);
    CHECK(out_off * 8 == (size_t)2040 << 27);                   // byte offsets, as run adds them
    // the other choice: 128 MiB of t per polynomial
    const KsnttShape T = ksntt_shape(limit, n, L, K, alpha, 64, batch, true);
    CHECK(T.t_bytes == (size_t)128 << 20 && T.chunk == 31 && T.subs == 67);
    // one polynomial above the limit: sub-batches of one
    CHECK(ksntt_shape(mib, n, L, K, alpha, 64, batch).chunk == 1);
    CHECK(ksntt_shape(mib, n, L, K, alpha, 64, batch).subs == batch);
    // scratch_mb at its largest does not overflow the limit's shift
    CHECK(ksntt_shape((size_t)UINT32_MAX << 20, n, L, K, alpha, 64, batch).chunk == batch);
    // mac's operand words past 2^32
    size_t words[3];
    ksntt_mac_words(L + K, n, batch, 4, 16, 2, words);
    CHECK(words[0] == batch * 32 * 64 * 65536 && words[0] > ((size_t)1 << 32));
    CHECK(words[1] == batch * 4 * 64 * 65536 && words[2] == (size_t)128 * 64 * 65536);
  }
  printf("ksntt sanitizer run ok: %d walks\n", walks);
  return 0;
}
