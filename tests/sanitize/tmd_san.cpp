// tmd_san.cpp — the host-only part of include/nttmul_tmd.h under ASan / UBSan, with a main of its
// own (tests/test_tmd_sanitizers.py): csrc/tmd_plan.hpp tmd_validate over csrc/basis.cpp (create's
// statuses and their order, the plaintext modulus' four last, the bounds of t at both ends of
// each class), tmd_constants against a naive recomputation in 128-bit integers, tmd_call_status,
// and tmd_shape over csrc/subbatch.hpp, the very functions csrc/tmd.cpp calls.  None of them needs
// a device.  A call's sub-batches are walked through heap blocks of exactly the operands' sizes,
// one byte per polynomial and limb, with the offsets tmd.cpp run forms, so a sub-batch that starts
// or ends outside an operand is a report; the byte offsets are computed for shapes where they
// pass 2^32 words.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "tmd_plan.hpp"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      return 1;                                                   \
    }                                                             \
  } while (0)

using namespace nttmul;
using u128 = unsigned __int128;

// primes = 1 mod 2^17 (tests/dispatch_cases.py, tests/rnsmp_cases.py): below 2^31, of 62 and 61
// bits, one in [2^31, 2^32)
static const uint64_t kQ31 = 2013265921ull, kQ31b = 2147352577ull;
static const uint64_t kQ62 = 0x3FFFFFFFFFE80001ull, kQ61 = 2305843009211596801ull;
static const uint64_t kQ32 = 4293918721ull;

static int status(uint32_t n, const uint64_t *q, uint32_t L, const uint64_t *p, uint32_t K,
                  uint64_t t, uint32_t flags = 0, uint64_t pq = 0,
                  size_t size = sizeof(nttmul_params)) {
  nttmul_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.n = n;
  prm.q = pq;
  prm.ndev = 1;
  prm.flags = flags;
  TmPlan P;
  return tmd_validate(&prm, size, q, L, p, K, t, &P);
}

static int check_statuses() {
  const uint64_t q32[2] = {kQ31, kQ31b}, q64[2] = {kQ62, kQ61};
  const uint64_t top32 = (uint64_t)1 << 31, top64 = (uint64_t)1 << 62;
  CHECK(tmd_t_bound(32) == top32 && tmd_t_bound(64) == top64);
  for (uint32_t n : {256u, 4096u, 8192u, 65536u}) {
    // both ends of each class: 3 and bound - 1 are the first and the last valid t
    for (uint64_t t : {(uint64_t)3, (uint64_t)5, (uint64_t)65537, top32 - 3, top32 - 1})
      CHECK(status(n, q32, 1, q32 + 1, 1, t) == NTTMUL_OK);
    for (uint64_t t : {(uint64_t)3, (uint64_t)65537, top32 - 1, top32 + 1, top64 - 3, top64 - 1})
      CHECK(status(n, q64, 1, q64 + 1, 1, t) == NTTMUL_OK);
    for (const uint64_t *b : {q32, q64}) {
      const uint64_t top = b == q32 ? top32 : top64;
      for (uint64_t t : {(uint64_t)0, (uint64_t)1, (uint64_t)2})    // t < 3, the even 0 and 2 too
        CHECK(status(n, b, 1, b + 1, 1, t) == NTTMUL_EINVAL);
      for (uint64_t t : {(uint64_t)4, top - 2, top, top + 2, UINT64_MAX - 1})   // even, any size
        CHECK(status(n, b, 1, b + 1, 1, t) == NTTMUL_EUNSUPPORTED);
      for (uint64_t t : {top + 1, top + 3, UINT64_MAX})              // odd, at or above the bound
        CHECK(status(n, b, 1, b + 1, 1, t) == NTTMUL_EINVAL);
      CHECK(status(n, b, 1, b + 1, 1, b[0]) == NTTMUL_EINVAL);       // 0 mod q_0
      CHECK(status(n, b, 1, b + 1, 1, b[1]) == NTTMUL_EINVAL);       // 0 mod p_0
      CHECK(status(n, b, 2, b == q32 ? q64 : q32, 1, b[1]) == NTTMUL_EUNSUPPORTED);  // mixed first
      // the order: t's statuses come after every status of nttmul_mdntt_create
      for (uint64_t t : {(uint64_t)0, (uint64_t)4, top + 1, b[0]}) {
        CHECK(status(n, b, 1, b + 1, 1, t, NTTMUL_FLAG_CYCLIC) == NTTMUL_EUNSUPPORTED);
        CHECK(status(n, b, 1, b, 1, t) == NTTMUL_EINVAL);            // a prime in both bases
        CHECK(status(n, b, 0, b + 1, 1, t) == NTTMUL_EINVAL);
        CHECK(status(n, b, 1, b + 1, 0, t) == NTTMUL_EINVAL);
        CHECK(status(n, nullptr, 1, b + 1, 1, t) == NTTMUL_EINVAL);
        CHECK(status(n, b, 1, nullptr, 1, t) == NTTMUL_EINVAL);
        CHECK(status(n, b, 1, b + 1, 1, t, 0, kQ31) == NTTMUL_EINVAL);   // params->q
        CHECK(status(n, b, 1, b + 1, 1, t, 0, 0, 4) == NTTMUL_EINVAL);   // params size
        CHECK(status(n, b, 1, &kQ32, 1, t) == NTTMUL_EUNSUPPORTED);      // [2^31, 2^32)
      }
    }
    CHECK(status(n, q32, 1, q32 + 1, 1, 3 * (uint64_t)715827883) == NTTMUL_EINVAL);  // = 2^31 + 1
  }
  CHECK(status(128, q32, 1, q32 + 1, 1, 3) == NTTMUL_EINVAL);
  CHECK(status(131072, q32, 1, q32 + 1, 1, 3) == NTTMUL_EINVAL);    // 2^18 does not divide q - 1
  // limb counts: exactly NTTMUL_RNS_MAX_LIMBS entries on the heap, so a read past a basis' own
  // count (by t's loops over p and q as well) is a report
  uint64_t *many = (uint64_t *)malloc(sizeof(uint64_t) * NTTMUL_RNS_MAX_LIMBS);
  CHECK(many);
  for (uint32_t i = 0; i < NTTMUL_RNS_MAX_LIMBS; i++) many[i] = 3 + i;
  CHECK(status(256, many, NTTMUL_RNS_MAX_LIMBS + 1, q32, 1, 3) == NTTMUL_EINVAL);
  CHECK(status(256, q32, 1, many, NTTMUL_RNS_MAX_LIMBS + 1, 3) == NTTMUL_EINVAL);
  free(many);
  // the calls
  int one = 0;
  const void *a = &one;
  for (int ctx = 0; ctx <= 1; ctx++)
    for (size_t batch = 0; batch <= 2; batch++)
      for (int mask = 0; mask < 4; mask++) {
        const void *out = mask & 1 ? a : nullptr, *x = mask & 2 ? a : nullptr;
        const bool bad = !ctx || (batch && mask != 3);
        CHECK(tmd_call_status(ctx, out, x, batch) == (bad ? NTTMUL_EINVAL : NTTMUL_OK));
      }
  CHECK(tmd_call_status(true, a, a, (size_t)1 << 40) == NTTMUL_OK);
  return 0;
}

static uint64_t naive_mul(uint64_t a, uint64_t b, uint64_t m) { return (uint64_t)((u128)a * b % m); }

// the tables of (q, p, t) against their definitions, by products alone: nothing of the planner's
// and no inverse of its own
static int check_tables(uint32_t n, const std::vector<uint64_t> &q, const std::vector<uint64_t> &p,
                        uint64_t t, int bits) {
  nttmul_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.n = n;
  prm.ndev = 1;
  TmPlan P;
  const uint32_t L = (uint32_t)q.size(), K = (uint32_t)p.size();
  CHECK(tmd_validate(&prm, sizeof(prm), q.data(), L, p.data(), K, t, &P) == NTTMUL_OK);
  CHECK(P.word_bits == bits && P.n == n && P.L == L && P.K == K && P.t == t);
  tmd_constants(&P);
  CHECK(P.yscale.size() == K && P.g.size() == K && P.v.size() == L);
  CHECK(P.w.size() == (size_t)(K + 2) * L);
  const auto prod = [&](uint32_t skip, uint64_t m) {
    uint64_t r = 1 % m;
    for (uint32_t j = 0; j < K; j++)
      if (j != skip) r = naive_mul(r, p[j] % m, m);
    return r;
  };
  for (uint32_t j = 0; j < K; j++) {
    // yscale_j Ph_j = 1 mod p_j;  g_j p_j = -1 mod t
    CHECK(P.yscale[j] < p[j] && P.g[j] < t);
    CHECK(naive_mul(P.yscale[j], prod(j, p[j]), p[j]) == 1);
    CHECK((naive_mul(P.g[j], p[j] % t, t) + 1) % t == 0);
  }
  for (uint32_t l = 0; l < L; l++) {
    const uint64_t m = q[l];
    for (uint32_t j = 0; j < K; j++) CHECK(P.w[(size_t)j * L + l] == prod(j, m));
    // the correction's rows: P, and w + P = 0 mod q_l
    CHECK(P.w[(size_t)K * L + l] == prod(K, m));
    CHECK(P.w[(size_t)(K + 1) * L + l] < m);
    CHECK((P.w[(size_t)(K + 1) * L + l] + prod(K, m)) % m == 0);
    // v P = 1 mod q_l
    CHECK(naive_mul(P.v[l], prod(K, m), m) == 1);
  }
  // msg_factor P = 1 mod t
  CHECK(P.msg_factor < t && naive_mul(P.msg_factor, prod(K, t), t) == 1);
  return 0;
}

// one call's sub-batches over blocks of one byte per (polynomial, limb) of x_hat and of out
static int walk(size_t limit, uint32_t n, uint32_t L, uint32_t K, int bits, size_t batch,
                size_t *subs) {
  const MdShape S = tmd_shape(limit, n, L, K, bits, batch);
  const size_t wb = bits / 8, per = n > 4096 ? (L > K ? L : K) * (size_t)n * wb : (size_t)K * n * wb;
  const uint32_t in_limbs = L + K;
  size_t want = 1;
  for (size_t k = 1; k <= batch; k++)
    if (k * per <= limit) want = k;
  CHECK(S.chunk == want && S.subs == (batch + want - 1) / want);
  CHECK(S.in_words == (size_t)in_limbs * n && S.out_words == (size_t)L * n);
  CHECK(S.y_bytes == (size_t)K * n * wb && S.t_bytes == (n > 4096 ? (size_t)L * n * wb : 0));
  uint8_t *x = (uint8_t *)calloc(batch * in_limbs, 1), *out = (uint8_t *)calloc(batch * L, 1);
  uint8_t *y = (uint8_t *)calloc(S.chunk * K, 1), *t = (uint8_t *)calloc(S.chunk * L, 1);
  CHECK(x && out && y && t);
  size_t done = 0;
  for (size_t k = 0; k < S.subs; k++) {
    const MpSub u = mp_sub(batch, S.chunk, k);
    CHECK(u.p == done && u.cnt >= 1 && u.cnt <= S.chunk && u.p + u.cnt <= batch);
    CHECK(k + 1 == S.subs || u.cnt == S.chunk);
    uint8_t *xu = x + u.p * S.in_words / n, *ou = out + u.p * S.out_words / n;
    for (size_t v = 0; v < u.cnt; v++) {
      for (uint32_t j = 0; j < K; j++) {
        xu[v * in_limbs + L + j]++;                                // the inverse reads P's limb j
        y[v * K + j] = 1;
      }
      for (uint32_t l = 0; l < L; l++) {
        xu[v * in_limbs + l]++;                                    // the epilogue reads limb l
        t[v * L + l] = 1;
        ou[v * L + l]++;
      }
    }
    done += u.cnt;
  }
  CHECK(done == batch);
  for (size_t i = 0; i < batch * in_limbs; i++) CHECK(x[i] == 1);
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
  int tables = 0;
  const uint64_t top32 = (uint64_t)1 << 31, top64 = (uint64_t)1 << 62;
  // prime and composite t, the ends of each class
  for (uint64_t t : {(uint64_t)3, (uint64_t)9, (uint64_t)65537, (uint64_t)3 * 65537, top32 - 1}) {
    if (check_tables(256, {kQ31}, {kQ31b}, t, 32)) return 1;
    if (check_tables(65536, {kQ31, kQ31b}, {1811939329ull, 2113929217ull, 2130706433ull}, t, 32))
      return 1;
    tables += 2;
  }
  for (uint64_t t : {(uint64_t)3, (uint64_t)65537, top32 + 1, top64 - 57, top64 - 1}) {
    if (check_tables(4096, {kQ62}, {kQ61}, t, 64)) return 1;
    if (check_tables(8192, {kQ61, 4296540161ull}, {kQ62, 4298506241ull}, t, 64)) return 1;
    tables += 2;
  }
  int walks = 0;
  size_t subs = 0;
  const size_t mib = (size_t)1 << 20;
  // tests/tmd_cases.py SUBBATCH, scratch_mb = 1
  if (walk(mib, 8192, 3, 2, 32, 23, &subs)) return 1;
  CHECK(subs == 3 && tmd_shape(mib, 8192, 3, 2, 32, 23).chunk == 10);
  if (walk(mib, 8192, 3, 2, 64, 12, &subs)) return 1;
  CHECK(subs == 3 && tmd_shape(mib, 8192, 3, 2, 64, 12).chunk == 5);
  walks += 2;
  CHECK(tmd_shape(mib, 256, 1, 1, 32, 0).subs == 0);              // the empty batch
  for (size_t limit : {(size_t)1, (size_t)65536, mib})
    for (uint32_t n : {256u, 4096u, 8192u, 65536u})
      for (uint32_t L : {1u, 3u, 60u})
        for (uint32_t K : {1u, 4u})
          for (int bits : {32, 64})
            for (size_t batch : {(size_t)1, (size_t)33}) {
              if (walk(limit, n, L, K, bits, batch, &subs)) return 1;
              walks++;
            }
  // the largest shapes: 60 + 4 limbs of n = 65536 on 64-bit words, a batch whose operands pass
  // 2^32 words.  No memory is touched: the offsets alone
  const uint32_t n = 65536, L = 60, K = 4;
  const size_t batch = 2048, limit = (size_t)4095 << 20;
  const MdShape S = tmd_shape(limit, n, L, K, 64, batch);
  CHECK(S.chunk == 136 && S.subs == 16);                          // 4095 MiB / 30 MiB
  const MpSub last = mp_sub(batch, S.chunk, S.subs - 1);
  CHECK(last.p == 2040 && last.cnt == 8);
  const size_t in_off = last.p * S.in_words, out_off = last.p * S.out_words;
  CHECK(out_off > ((size_t)1 << 32) && out_off == (size_t)2040 * 60 * 65536);
  CHECK(in_off > ((size_t)1 << 32) && in_off == (size_t)2040 * 64 * 65536);
  CHECK(in_off + last.cnt * S.in_words == batch * S.in_words);
  CHECK(tmd_shape((size_t)UINT32_MAX << 20, n, L, K, 64, batch).chunk == batch);
  printf("tmd sanitizer run ok: %d tables, %d walks\n", tables, walks);
  return 0;
}
