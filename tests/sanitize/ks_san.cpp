// ks_san.cpp — the host-only entry point of include/nttmul_ks.h (csrc/ks_plan.cpp: nttmul_ks_plan,
// over csrc/basis.cpp's create-time checks and csrc/planner.cpp's modular arithmetic) under ASan /
// UBSan, with a main of its own
// (tests/test_ks_sanitizers.py).  Every table is a heap block of exactly its stated size, so a
// write past either end is a report; the results are checked against the definitions, computed
// here another way (running products in 128-bit integers, inverses checked by multiplying back).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "nttmul_ks.h"
#include "planner.hpp"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      return 1;                                                   \
    }                                                             \
  } while (0)

typedef unsigned __int128 u128;

static uint64_t mm(uint64_t a, uint64_t b, uint64_t m) { return (uint64_t)((u128)a * b % m); }

// the first `count` primes = 1 mod 2^17 below top
static std::vector<uint64_t> primes_below(uint64_t top, size_t count) {
  std::vector<uint64_t> out;
  for (uint64_t q = (top - 2) / (1u << 17) * (1u << 17) + 1; out.size() < count; q -= 1u << 17)
    if (nttmul::is_prime(q)) out.push_back(q);
  return out;
}

static uint64_t *block(size_t words) {
  uint64_t *p = (uint64_t *)malloc(sizeof(uint64_t) * words);
  if (p) memset(p, 0xA5, sizeof(uint64_t) * words);
  return p;
}

static int check_plan(uint32_t n, uint64_t top, uint32_t L, uint32_t K, uint32_t alpha) {
  const std::vector<uint64_t> all = primes_below(top, L + K);
  const uint64_t *q = all.data(), *p = all.data() + L;
  const uint32_t M = L + K, dnum = (L + alpha - 1) / alpha;
  nttmul_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.n = n;
  uint64_t *inv = block(L), *w = block((size_t)L * M), *g = block((size_t)dnum * M);
  uint64_t *pinv = block(K), *pw = block((size_t)K * L), *Pinv = block(L);
  CHECK(inv && w && g && pinv && pw && Pinv);
  CHECK(nttmul_ks_plan(&prm, sizeof(prm), q, L, p, K, alpha, inv, w, g, pinv, pw, Pinv) ==
        NTTMUL_OK);
  for (uint32_t i = 0; i < L; i++) {
    const uint32_t lo = i / alpha * alpha, hi = lo + alpha < L ? lo + alpha : L;
    for (uint32_t m = 0; m < M; m++) {
      const uint64_t mod = all[m];
      uint64_t v = 1;
      for (uint32_t t = lo; t < hi; t++)
        if (t != i) v = mm(v, q[t] % mod, mod);
      CHECK(w[(size_t)i * M + m] == v);
      if (m >= lo && m < hi && m != i) CHECK(v == 0);
    }
    CHECK(inv[i] < q[i] && mm(inv[i], w[(size_t)i * M + i], q[i]) == 1);
  }
  for (uint32_t d = 0; d < dnum; d++)
    for (uint32_t m = 0; m < M; m++) {
      uint64_t want = 0;
      if (m >= d * alpha && m < (d + 1) * alpha && m < L) {
        want = 1;
        for (uint32_t j = 0; j < K; j++) want = mm(want, p[j] % q[m], q[m]);
      }
      CHECK(g[(size_t)d * M + m] == want);
    }
  for (uint32_t j = 0; j < K; j++) {
    for (uint32_t i = 0; i < L; i++) {
      uint64_t v = 1;
      for (uint32_t t = 0; t < K; t++)
        if (t != j) v = mm(v, p[t] % q[i], q[i]);
      CHECK(pw[(size_t)j * L + i] == v);
    }
    uint64_t ph = 1;
    for (uint32_t t = 0; t < K; t++)
      if (t != j) ph = mm(ph, p[t] % p[j], p[j]);
    CHECK(pinv[j] < p[j] && mm(pinv[j], ph, p[j]) == 1);
  }
  for (uint32_t i = 0; i < L; i++) {
    uint64_t v = 1;
    for (uint32_t t = 0; t < K; t++) v = mm(v, p[t] % q[i], q[i]);
    CHECK(Pinv[i] < q[i] && mm(Pinv[i], v, q[i]) == 1);
  }
  // partial tables, and no table at all
  CHECK(nttmul_ks_plan(&prm, sizeof(prm), q, L, p, K, alpha, nullptr, nullptr, g, nullptr, nullptr,
                       Pinv) == NTTMUL_OK);
  CHECK(nttmul_ks_plan(&prm, sizeof(prm), q, L, p, K, alpha, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr) == NTTMUL_OK);
  // refusals write nothing
  uint64_t one = 7;
  CHECK(nttmul_ks_plan(&prm, sizeof(prm), q, L, p, K, 0, &one, &one, &one, &one, &one, &one) ==
        NTTMUL_EINVAL);
  CHECK(nttmul_ks_plan(&prm, sizeof(prm), q, L, p, K, L + 1, &one, &one, &one, &one, &one, &one) ==
        NTTMUL_EINVAL);
  CHECK(nttmul_ks_plan(&prm, sizeof(prm), q, L, q, 1, alpha, &one, &one, &one, &one, &one, &one) ==
        NTTMUL_EINVAL);
  CHECK(nttmul_ks_plan(&prm, sizeof(prm), q, L, p, 0, alpha, &one, &one, &one, &one, &one, &one) ==
        NTTMUL_EINVAL);
  CHECK(nttmul_ks_plan(&prm, 4, q, L, p, K, alpha, &one, &one, &one, &one, &one, &one) ==
        NTTMUL_EINVAL);
  CHECK(nttmul_ks_plan(nullptr, sizeof(prm), q, L, p, K, alpha, &one, &one, &one, &one, &one,
                       &one) == NTTMUL_EINVAL);
  prm.flags = NTTMUL_FLAG_CYCLIC;
  CHECK(nttmul_ks_plan(&prm, sizeof(prm), q, L, p, K, alpha, &one, &one, &one, &one, &one, &one) ==
        NTTMUL_EUNSUPPORTED);
  CHECK(one == 7);
  for (uint64_t *b : {inv, w, g, pinv, pw, Pinv}) free(b);
  return 0;
}

int main() {
  const uint32_t shapes[][3] = {{1, 1, 1}, {4, 2, 2}, {5, 2, 2}, {5, 3, 5}, {6, 1, 1}};
  int plans = 0;
  for (uint32_t n : {256u, 4096u, 8192u, 65536u})
    for (uint64_t top : {1ull << 31, 1ull << 62})
      for (const auto &s : shapes) {
        if (check_plan(n, top, s[0], s[1], s[2])) return 1;
        plans++;
      }
  // the widest basis: L + K = NTTMUL_RNS_MAX_LIMBS, and one limb more
  if (check_plan(256, 1ull << 31, 60, 4, 15)) return 1;
  const std::vector<uint64_t> many = primes_below(1ull << 31, 65);
  nttmul_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.n = 256;
  uint64_t one = 7;
  CHECK(nttmul_ks_plan(&prm, sizeof(prm), many.data(), 60, many.data() + 60, 5, 15, &one, &one,
                       &one, &one, &one, &one) == NTTMUL_EINVAL);
  for (uint32_t bad : {0u, 128u, 768u, 0xFFFFFFFFu}) {
    prm.n = bad;
    CHECK(nttmul_ks_plan(&prm, sizeof(prm), many.data(), 2, many.data() + 2, 1, 1, &one, &one, &one,
                         &one, &one, &one) == NTTMUL_EINVAL);
  }
  CHECK(one == 7);
  printf("ks sanitizer run ok: %d plans\n", plans);
  return 0;
}
