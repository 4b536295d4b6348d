// mdntt_san.cpp — the host-only part of include/nttmul_mdntt.h under ASan / UBSan, with a main of
// its own (tests/test_mdntt_sanitizers.py): csrc/mdntt_plan.hpp mdntt_validate over csrc/basis.cpp
// (create's statuses and their order), mdntt_call_status, and mdntt_shape over csrc/subbatch.hpp,
// the very functions csrc/mdntt.cpp calls.  None of them needs a device.  The sub-batch rule is
// checked against its definition, computed here another way (a linear search for the largest count
// that fits), and a call's sub-batches are walked through heap blocks of exactly the operands'
// sizes, one byte per polynomial and limb, with the offsets mdntt.cpp run forms, so a sub-batch that
// starts or ends outside an operand is a report; the byte offsets are computed for shapes where
// they pass 2^32 words.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mdntt_plan.hpp"

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
                  uint32_t flags = 0, uint64_t pq = 0, size_t size = sizeof(nttmul_params)) {
  nttmul_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.n = n;
  prm.q = pq;
  prm.ndev = 1;
  prm.flags = flags;
  BasisRequest B;
  return mdntt_validate(&prm, size, q, L, p, K, &B);
}

static int check_statuses() {
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
    // the order: an EINVAL of P comes before an EUNSUPPORTED of Q
    CHECK(status(n, &kQ32, 1, comp, 1) == NTTMUL_EINVAL);
    CHECK(status(n, q32, 1, q32 + 1, 1, NTTMUL_FLAG_CYCLIC, kQ31) == NTTMUL_EINVAL);
  }
  CHECK(status(128, q32, 1, q32 + 1, 1) == NTTMUL_EINVAL);
  CHECK(status(10000, q32, 1, q32 + 1, 1) == NTTMUL_EINVAL);
  CHECK(status(131072, q32, 1, q32 + 1, 1) == NTTMUL_EINVAL);       // 2^18 does not divide q - 1
  // limb counts: exactly NTTMUL_RNS_MAX_LIMBS entries on the heap per basis, so a read past a
  // basis' own count is a report.  The moduli are not prime: the count's EINVAL must come first
  // for 65 limbs in one basis, and the primality EINVAL comes before the sum's
  uint64_t *many = (uint64_t *)malloc(sizeof(uint64_t) * NTTMUL_RNS_MAX_LIMBS);
  CHECK(many);
  for (uint32_t i = 0; i < NTTMUL_RNS_MAX_LIMBS; i++) many[i] = 3 + i;
  CHECK(status(256, many, NTTMUL_RNS_MAX_LIMBS + 1, q32, 1) == NTTMUL_EINVAL);
  CHECK(status(256, q32, 1, many, NTTMUL_RNS_MAX_LIMBS + 1) == NTTMUL_EINVAL);
  CHECK(status(256, many, NTTMUL_RNS_MAX_LIMBS, q32, 1) == NTTMUL_EINVAL);
  free(many);
  // the calls
  int one = 0;
  const void *a = &one;
  for (int ctx = 0; ctx <= 1; ctx++)
    for (size_t batch = 0; batch <= 2; batch++)
      for (int mask = 0; mask < 4; mask++) {
        const void *out = mask & 1 ? a : nullptr, *x = mask & 2 ? a : nullptr;
        const bool bad = !ctx || (batch && mask != 3);
        CHECK(mdntt_call_status(ctx, out, x, batch) == (bad ? NTTMUL_EINVAL : NTTMUL_OK));
      }
  CHECK(mdntt_call_status(true, a, a, (size_t)1 << 40) == NTTMUL_OK);
  return 0;
}

// one call's sub-batches over blocks of one byte per (polynomial, limb) of x_hat and of out: every
// byte of out is written exactly once, every byte of x_hat read exactly once, and the scratch
// blocks of a sub-batch are never indexed past chunk polynomials
static int walk(size_t limit, uint32_t n, uint32_t L, uint32_t K, int bits, size_t batch,
                size_t *subs) {
  const MdShape S = mdntt_shape(limit, n, L, K, bits, batch);
  const size_t wb = bits / 8, per = n > 4096 ? (L > K ? L : K) * (size_t)n * wb : (size_t)K * n * wb;
  size_t want = 1;
  for (size_t k = 1; k <= batch; k++)
    if (k * per <= limit) want = k;
  CHECK(S.chunk == want && S.subs == (batch + want - 1) / want);
  CHECK(S.in_words == ((size_t)L + K) * n && S.out_words == (size_t)L * n);
  CHECK(S.y_bytes == (size_t)K * n * wb && S.t_bytes == (n > 4096 ? (size_t)L * n * wb : 0));
  uint8_t *x = (uint8_t *)calloc(batch * (L + K), 1), *out = (uint8_t *)calloc(batch * L, 1);
  uint8_t *y = (uint8_t *)calloc(S.chunk * K, 1), *t = (uint8_t *)calloc(S.chunk * L, 1);
  CHECK(x && out && y && t);
  size_t done = 0;
  for (size_t k = 0; k < S.subs; k++) {
    const MpSub u = mp_sub(batch, S.chunk, k);
    CHECK(u.p == done && u.cnt >= 1 && u.cnt <= S.chunk && u.p + u.cnt <= batch);
    CHECK(k + 1 == S.subs || u.cnt == S.chunk);
    // mdntt.cpp run: the sub-batch's operands start u.p whole polynomials in
    CHECK(u.p * S.in_words % n == 0 && u.p * S.out_words % n == 0);
    uint8_t *xu = x + u.p * S.in_words / n, *ou = out + u.p * S.out_words / n;
    for (size_t v = 0; v < u.cnt; v++) {
      for (uint32_t j = 0; j < K; j++) {
        xu[v * (L + K) + L + j]++;                                // the inverse reads limb L + j
        y[v * K + j] = 1;
      }
      for (uint32_t l = 0; l < L; l++) {
        xu[v * (L + K) + l]++;                                    // the epilogue reads limb l
        t[v * L + l] = 1;
        ou[v * L + l]++;
      }
    }
    done += u.cnt;
  }
  CHECK(done == batch);
  for (size_t i = 0; i < batch * (L + K); i++) CHECK(x[i] == 1);
  for (size_t i = 0; i < batch * L; i++) CHECK(out[i] == 1);
  free(x);
  free(out);
  free(y);
  free(t);
  *subs = S.subs;
  return 0;
}

int main() {
  if (check_statuses()) return 1;
  int walks = 0;
  size_t subs = 0;
  const size_t mib = (size_t)1 << 20;
  // tests/mdntt_cases.py SUBBATCH, scratch_mb = 1
  if (walk(mib, 4096, 3, 2, 64, 35, &subs)) return 1;
  CHECK(subs == 3 && mdntt_shape(mib, 4096, 3, 2, 64, 35).chunk == 16);
  if (walk(mib, 65536, 2, 2, 64, 3, &subs)) return 1;
  CHECK(subs == 3 && mdntt_shape(mib, 65536, 2, 2, 64, 3).chunk == 1);
  walks += 2;
  // the empty batch: no sub-batch
  CHECK(mdntt_shape(mib, 256, 1, 1, 32, 0).subs == 0);
  // every small shape: limits around one polynomial's scratch, one polynomial above the limit
  for (size_t limit : {(size_t)1, (size_t)4096, (size_t)65536, mib})
    for (uint32_t n : {256u, 4096u, 8192u, 65536u})
      for (uint32_t L : {1u, 3u, 60u})
        for (uint32_t K : {1u, 2u, 4u})
          for (int bits : {32, 64})
            for (size_t batch : {(size_t)1, (size_t)2, (size_t)33}) {
              if (walk(limit, n, L, K, bits, batch, &subs)) return 1;
              walks++;
            }
  // the largest shapes: 60 + 4 limbs of n = 65536 on 64-bit words, a scratch of 4095 MiB, a batch
  // whose x_hat passes 2^32 words.  No memory is touched: the offsets alone
  {
    const uint32_t n = 65536, L = 60, K = 4;
    const size_t batch = 2048, limit = (size_t)4095 << 20;
    const MdShape S = mdntt_shape(limit, n, L, K, 64, batch);
    CHECK(S.t_bytes == (size_t)60 << 19 && S.y_bytes == (size_t)4 << 19);
    CHECK(S.chunk == 136 && S.subs == 16);                      // 4095 MiB / 30 MiB
    const MpSub last = mp_sub(batch, S.chunk, S.subs - 1);
    CHECK(last.p == 2040 && last.cnt == 8);
    const size_t in_off = last.p * S.in_words, out_off = last.p * S.out_words;
    CHECK(in_off > ((size_t)1 << 32) && in_off == (size_t)2040 * 64 * 65536);
    CHECK(out_off > ((size_t)1 << 32) && out_off == (size_t)2040 * 60 * 65536);
    CHECK(in_off + last.cnt * S.in_words == batch * S.in_words);
    CHECK(batch * S.in_words == (size_t)1 << 33);
    // byte offsets, as run adds them to the operands
    CHECK(in_off * 8 == (size_t)2040 << 25);
    // one polynomial above the limit: sub-batches of one
    CHECK(mdntt_shape(mib, n, L, K, 64, batch).chunk == 1);
    CHECK(mdntt_shape(mib, n, L, K, 64, batch).subs == batch);
    // scratch_mb at its largest does not overflow the limit's shift
    CHECK(mdntt_shape((size_t)UINT32_MAX << 20, n, L, K, 64, batch).chunk == batch);
  }
  printf("mdntt sanitizer run ok: %d walks\n", walks);
  return 0;
}
