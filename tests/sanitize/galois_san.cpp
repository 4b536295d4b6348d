// galois_san.cpp — the host-only entry points of include/nttmul_galois.h (csrc/galois_plan.cpp:
// nttmul_galois_element, nttmul_galois_plan) under ASan / UBSan, with
// a main of its own (tests/test_galois_sanitizers.py).  Every table is a heap block of exactly n
// entries, so a write past either end is a report; the results are checked against the
// definitions, computed here another way (a scatter for the coefficients, a lookup by evaluation
// exponent for the slots).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "nttmul_galois.h"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      return 1;                                                   \
    }                                                             \
  } while (0)

static uint32_t brv(uint32_t x, uint32_t bits) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < bits; i++)
    if (x & (1u << i)) r |= 1u << (bits - 1 - i);
  return r;
}

static int check_plan(uint32_t n, uint32_t k) {
  uint32_t logn = 0;
  while ((1u << logn) < n) logn++;
  // exactly n entries each, on the heap
  uint32_t *src = (uint32_t *)malloc(sizeof(uint32_t) * n);
  uint8_t *neg = (uint8_t *)malloc(n);
  uint32_t *hat = (uint32_t *)malloc(sizeof(uint32_t) * n);
  CHECK(src && neg && hat);
  CHECK(nttmul_galois_plan(n, k, src, neg, hat) == NTTMUL_OK);
  std::vector<int64_t> want_src(n, -1), want_neg(n, -1), slot_of(2 * (size_t)n, -1);
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t e = i * k % (2ull * n);
    want_src[e % n] = (int64_t)i;
    want_neg[e % n] = e >= n;
  }
  for (uint32_t j = 0; j < n; j++) slot_of[2 * brv(j, logn) + 1] = j;
  for (uint32_t j = 0; j < n; j++) {
    CHECK(src[j] == want_src[j] && neg[j] == want_neg[j]);
    const uint64_t e = (uint64_t)k * (2 * brv(j, logn) + 1) % (2ull * n);
    CHECK(slot_of[e] >= 0 && hat[j] == (uint32_t)slot_of[e]);
  }
  // partial tables
  CHECK(nttmul_galois_plan(n, k, nullptr, neg, nullptr) == NTTMUL_OK);
  CHECK(nttmul_galois_plan(n, k, nullptr, nullptr, nullptr) == NTTMUL_OK);
  free(src);
  free(neg);
  free(hat);
  return 0;
}

int main() {
  int plans = 0;
  for (uint32_t n = 256; n <= 65536; n *= 2) {
    uint32_t k5 = 0, kback = 0, kconj = 0, k = 0;
    CHECK(nttmul_galois_element(n, 1, 0, &k5) == NTTMUL_OK && k5 == 5);
    CHECK(nttmul_galois_element(n, -3, 0, &kback) == NTTMUL_OK);
    CHECK((uint64_t)kback * 125 % (2ull * n) == 1);
    CHECK(nttmul_galois_element(n, 0, 1, &kconj) == NTTMUL_OK && kconj == 2 * n - 1);
    // the extremes of the step, and the order of 5
    CHECK(nttmul_galois_element(n, INT64_MIN, 0, &k) == NTTMUL_OK && (k & 1) && k < 2 * n);
    CHECK(nttmul_galois_element(n, INT64_MAX, 1, &k) == NTTMUL_OK && (k & 1) && k < 2 * n);
    CHECK(nttmul_galois_element(n, n / 2, 0, &k) == NTTMUL_OK && k == 1);
    CHECK(nttmul_galois_element(n, -(int64_t)(n / 2) + 1, 0, &k) == NTTMUL_OK && k == 5);
    const uint32_t ks[] = {1, 3, n - 1, n + 1, 2 * n - 1, k5, kback};
    for (uint32_t kk : ks) {
      if (check_plan(n, kk)) return 1;
      plans++;
    }
    uint32_t one = 7;
    for (uint32_t bad : {0u, 2u, 2 * n, 2 * n + 1, 0xFFFFFFFFu})
      CHECK(nttmul_galois_plan(n, bad, &one, nullptr, nullptr) == NTTMUL_EINVAL && one == 7);
  }
  uint32_t k = 9;
  for (uint32_t bad : {0u, 1u, 128u, 255u, 768u, 131072u, 0x80000000u, 0xFFFFFFFFu}) {
    CHECK(nttmul_galois_element(bad, 1, 0, &k) == NTTMUL_EINVAL && k == 9);
    CHECK(nttmul_galois_plan(bad, 3, &k, nullptr, nullptr) == NTTMUL_EINVAL && k == 9);
  }
  CHECK(nttmul_galois_element(256, 1, 0, nullptr) == NTTMUL_EINVAL);
  printf("galois sanitizer run ok: %d plans\n", plans);
  return 0;
}
