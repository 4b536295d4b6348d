// ctlin_san.cpp — the host-only part of include/nttmul_ctlin.h under ASan / UBSan, with a main of
// its own (tests/test_ctlin_sanitizers.py): csrc/ctlin_plan.hpp ctlin_validate over csrc/basis.cpp
// (create's statuses and their order), ctlin_constants against values recomputed here naively,
// combine's statuses in the header's order, walked term by term, tensor's, and ctlin_grid, the
// word counts and the word offsets, the very functions csrc/ctlin.cpp and csrc/ctlin.hip call.
// None of them needs a device.  A launch's workgroups are walked through heap blocks of exactly
// the operands' sizes, with the batch entry and the vector formed from the workgroup and lane index
// as the kernels form them, so a lane that starts or ends outside an operand is a report; the word
// offsets are computed for shapes where they pass 2^32.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ctlin_plan.hpp"

#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      return 1;                                                   \
    }                                                             \
  } while (0)

using namespace nttmul;
using u128 = unsigned __int128;

// primes = 1 mod 2^17 (tests/basis_cases.py, tests/rnsmp_cases.py): of mixed sizes below 2^31 and
// in [2^32, 2^62), one in [2^31, 2^32)
static const uint64_t kQ31 = 2147352577ull, kQ25 = 35389441ull, kQ28 = 268042241ull;
static const uint64_t kQ60 = 1152921504606584833ull, kQ40 = 1099512938497ull,
                      kQ50 = 1125899903827969ull;
static const uint64_t kQ32 = 4293918721ull;

static int status(uint32_t n, const uint64_t *q, uint32_t L, uint32_t flags = 0, uint64_t pq = 0,
                  size_t size = sizeof(nttmul_params)) {
  nttmul_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.n = n;
  prm.q = pq;
  prm.ndev = 1;
  prm.flags = flags;
  ClPlan P;
  const int st = ctlin_validate(&prm, size, q, L, &P);
  // nttmul_galois_create's status is the same two steps with the same bounds
  BasisRequest B;
  int gal = basis_invalid(&prm, size, &q, &L, 1, 1u << 30, &B);
  if (!gal) gal = basis_unsupported(&B, 256, 65536, false);
  if (gal != st) return -99;
  if (st == NTTMUL_OK) {
    if (P.L != L || P.m.size() != L || P.n != n || (1u << P.logn) != n) return -100;
    if (P.word_bits != B.word_bits || P.flags != flags) return -101;
    ctlin_constants(&P);  // every table at its size, every value against a naive recomputation
    if (P.r1.size() != L || P.r2.size() != L) return -102;
    for (uint32_t l = 0; l < L; l++) {
      const uint64_t m = q[l];
      if (P.m[l] != m) return -103;
      u128 r = 1;
      for (int b = 0; b < P.word_bits; b++) r = r * 2 % m;
      if (P.r1[l] != (uint64_t)r || P.r1[l] >= m) return -104;
      for (int b = 0; b < P.word_bits; b++) r = r * 2 % m;         // R^2 mod q_l
      if (P.r2[l] != (uint64_t)r || P.r2[l] >= m || P.r2[l] == 0) return -105;
    }
  }
  return st;
}

static int check_create() {
  const uint64_t q32[3] = {kQ31, kQ25, kQ28}, q64[3] = {kQ60, kQ40, kQ50};
  for (uint32_t n : {256u, 4096u, 8192u, 65536u}) {
    for (uint32_t L : {1u, 2u, 3u}) {
      CHECK(status(n, q32, L) == NTTMUL_OK);
      CHECK(status(n, q64, L) == NTTMUL_OK);
    }
    CHECK(status(n, q32, 0) == NTTMUL_EINVAL);                      // limbs = 0
    CHECK(status(n, nullptr, 1) == NTTMUL_EINVAL);
    const uint64_t twice[2] = {kQ31, kQ31};
    CHECK(status(n, twice, 2) == NTTMUL_EINVAL);                    // a prime that occurs twice
    CHECK(status(n, q32, 3, 0, kQ31) == NTTMUL_EINVAL);             // params->q
    CHECK(status(n, q32, 3, 0, 0, 4) == NTTMUL_EINVAL);             // params size
    CHECK(status(n, q32, 3, NTTMUL_FLAG_CYCLIC) == NTTMUL_EUNSUPPORTED);
    const uint64_t mixed[2] = {kQ31, kQ60}, mixed2[2] = {kQ60, kQ31};
    CHECK(status(n, mixed, 2) == NTTMUL_EUNSUPPORTED);              // mixed classes
    CHECK(status(n, mixed2, 2) == NTTMUL_EUNSUPPORTED);
    CHECK(status(n, &kQ32, 1) == NTTMUL_EUNSUPPORTED);              // [2^31, 2^32)
    const uint64_t comp[2] = {kQ32, kQ31 + 2};
    CHECK(status(n, comp + 1, 1) == NTTMUL_EINVAL);                 // not prime
    // the order: every EINVAL before any EUNSUPPORTED
    CHECK(status(n, comp, 2) == NTTMUL_EINVAL);
    CHECK(status(n, q32, 3, NTTMUL_FLAG_CYCLIC, kQ31) == NTTMUL_EINVAL);
  }
  CHECK(status(128, q32, 1) == NTTMUL_EINVAL);
  CHECK(status(10000, q32, 1) == NTTMUL_EINVAL);
  CHECK(status(131072, q32, 1) == NTTMUL_EINVAL);                   // 2^18 does not divide q - 1
  // limb counts: exactly NTTMUL_RNS_MAX_LIMBS entries on the heap, so a read past the basis' own
  // count is a report
  uint64_t *many = (uint64_t *)malloc(sizeof(uint64_t) * NTTMUL_RNS_MAX_LIMBS);
  CHECK(many);
  for (uint32_t i = 0; i < NTTMUL_RNS_MAX_LIMBS; i++) many[i] = 3 + i;
  CHECK(status(256, many, NTTMUL_RNS_MAX_LIMBS + 1) == NTTMUL_EINVAL);
  CHECK(status(256, many, NTTMUL_RNS_MAX_LIMBS) == NTTMUL_EINVAL);
  free(many);
  return 0;
}

static nttmul_ctlin_term term(const void *x, const void *w, uint32_t kind, uint32_t reserved = 0) {
  nttmul_ctlin_term t;
  t.x = x;
  t.w = w;
  t.kind = kind;
  t.reserved = reserved;
  return t;
}

// combine's statuses in the header's order: a NULL context; nterms; comps; NULL terms; per term
// in index order kind, reserved, ONE with a w, SCALAR or PLAIN without one, ONE without an x; a
// NULL out with batch > 0; batch = 0 succeeds.  Each refusal is made with everything after it in
// the order wrong as well, and with everything before it right: the first one decides, and the
// array is on the heap at exactly nterms entries, so a look past it is a report
static int check_combine() {
  int one = 0;
  const void *a = &one;
  const nttmul_ctlin_term good[3] = {term(a, nullptr, NTTMUL_CTLIN_ONE),
                                     term(a, a, NTTMUL_CTLIN_SCALAR),
                                     term(nullptr, a, NTTMUL_CTLIN_PLAIN)};
  CHECK(ctlin_combine_status(true, &one, good, 3, 1, 1) == NTTMUL_OK);
  CHECK(ctlin_combine_status(true, &one, good, 3, (size_t)1 << 40, 3) == NTTMUL_OK);
  CHECK(ctlin_combine_status(true, nullptr, good, 3, 0, 2) == NTTMUL_OK);   // batch = 0
  const nttmul_ctlin_term cs = term(nullptr, a, NTTMUL_CTLIN_SCALAR);
  CHECK(ctlin_combine_status(true, &one, &cs, 1, 1, 1) == NTTMUL_OK);       // constants alone
  const int E = NTTMUL_EINVAL;
  const nttmul_ctlin_term worst = term(nullptr, nullptr, 3, 1);
  CHECK(ctlin_combine_status(false, &one, good, 3, 1, 1) == E);
  CHECK(ctlin_combine_status(false, nullptr, nullptr, 0, 0, 0) == E);
  for (uint32_t nterms : {0u, 17u, 0xFFFFFFFFu})                    // (terms is not looked at)
    CHECK(ctlin_combine_status(true, nullptr, nullptr, nterms, 1, 0) == E);
  for (uint32_t comps : {0u, 4u, 0xFFFFFFFFu}) {
    CHECK(ctlin_combine_status(true, nullptr, nullptr, 1, 1, comps) == E);
    CHECK(ctlin_combine_status(true, &one, good, 3, 0, comps) == E);        // also at batch 0
  }
  CHECK(ctlin_combine_status(true, nullptr, nullptr, 16, 1, 3) == E);       // NULL terms
  CHECK(ctlin_combine_status(true, nullptr, nullptr, 1, 0, 1) == E);
  // the per-term refusals, at every index of every count, on a heap array of exactly that count
  const nttmul_ctlin_term bad[5] = {
      term(nullptr, nullptr, 3, 1),                                 // kind (all else wrong too)
      term(nullptr, a, NTTMUL_CTLIN_ONE, 1),                        // reserved
      term(nullptr, a, NTTMUL_CTLIN_ONE),                           // ONE with a w (and no x)
      term(a, nullptr, NTTMUL_CTLIN_PLAIN),                         // PLAIN without a w
      term(nullptr, nullptr, NTTMUL_CTLIN_ONE)};                    // ONE without an x
  int walked = 0;
  for (uint32_t count : {1u, 2u, 16u})
    for (uint32_t at = 0; at < count; at++)
      for (int which = 0; which < 5; which++) {
        nttmul_ctlin_term *t = (nttmul_ctlin_term *)malloc(sizeof(nttmul_ctlin_term) * count);
        CHECK(t);
        for (uint32_t i = 0; i < count; i++) t[i] = i < at ? good[i % 3] : worst;
        t[at] = bad[which];
        // out is NULL too: the term decides
        CHECK(ctlin_combine_status(true, nullptr, t, count, 1, 1) == E);
        // the same term alone made right is accepted: it was that term
        for (uint32_t i = at; i < count; i++) t[i] = good[i % 3];
        CHECK(ctlin_combine_status(true, &one, t, count, 1, 1) == NTTMUL_OK);
        CHECK(ctlin_combine_status(true, nullptr, t, count, 1, 1) == E);    // a NULL out, last
        CHECK(ctlin_combine_status(true, nullptr, t, count, 0, 1) == NTTMUL_OK);
        free(t);
        walked++;
      }
  CHECK(walked == 5 * 19);
  const nttmul_ctlin_term sc = term(a, nullptr, NTTMUL_CTLIN_SCALAR);
  CHECK(ctlin_combine_status(true, &one, &sc, 1, 1, 1) == E);               // SCALAR without a w
  // tensor's: nttmul_ctmul_high's
  CHECK(ctlin_tensor_status(true, a, a, a, 1, 1) == NTTMUL_OK);
  CHECK(ctlin_tensor_status(true, nullptr, nullptr, nullptr, 0, 1) == NTTMUL_OK);
  CHECK(ctlin_tensor_status(false, a, a, a, 1, 1) == E);
  CHECK(ctlin_tensor_status(true, a, a, a, 1, 0) == E);
  CHECK(ctlin_tensor_status(true, nullptr, nullptr, nullptr, 0, 0) == E);
  for (int mask = 0; mask < 7; mask++)
    CHECK(ctlin_tensor_status(true, mask & 1 ? a : nullptr, mask & 2 ? a : nullptr,
                              mask & 4 ? a : nullptr, 1, 1) == E);
  return 0;
}

// The lanes of either kernel over a block of one byte per vector of a [batch][comps][L][n / vec]
// operand: every vector is taken exactly once, by the lane of its slot in every component
static int walk(size_t batch, uint32_t logn, uint32_t L, uint32_t comps, int word_bits) {
  const CtHighGrid G = ctlin_grid(batch, logn, word_bits);
  const uint32_t vec = word_bits == 32 ? 4 : 2, lgp = logn - (vec == 4 ? 2 : 1);
  const size_t pv = (size_t)1 << lgp;
  CHECK(G.vec == vec && vec * (word_bits / 8) == 16);
  CHECK(G.vectors == batch * pv && G.wgx == (G.vectors + 255) / 256 && G.ok);
  CHECK(G.tail == G.vectors % 256 && G.per == (pv < 256 ? 256 / pv : 1));
  size_t words[3];
  ctlin_combine_words(L, 1u << logn, batch, comps, words);
  CHECK(words[0] == batch * comps * L * pv * vec && words[1] == L && words[2] == L * pv * vec);
  if (!batch) {
    CHECK(G.wgx == 0);
    return 0;
  }
  uint8_t *o = (uint8_t *)calloc(words[0] / vec, 1), *w = (uint8_t *)calloc(words[2] / vec, 1);
  CHECK(o && w);
  size_t idle = 0;
  for (uint32_t l = 0; l < L; l++)
    for (size_t b = 0; b < G.wgx; b++)
      for (uint32_t t = 0; t < 256; t++) {
        const size_t g = b * 256 + t;
        if (g >= G.vectors) {
          idle++;
          continue;
        }
        const size_t p = g >> lgp, j = (g & (pv - 1)) * vec;
        CHECK(p < batch);
        for (uint32_t c = 0; c < comps; c++) {
          const size_t at = ctlin_word_offset(p, comps, c, L, l, logn) + j;
          CHECK(at % vec == 0 && at + vec <= words[0]);
          o[at / vec]++;
        }
        w[((((size_t)l) << logn) + j) / vec] = 1;                   // a plaintext's vector
      }
  for (size_t i = 0; i < words[0] / vec; i++) CHECK(o[i] == 1);
  for (size_t i = 0; i < words[2] / vec; i++) CHECK(w[i] == 1);
  CHECK(idle == (G.wgx * 256 - G.vectors) * L);
  free(o);
  free(w);
  return 0;
}

int main() {
  if (check_create() || check_combine()) return 1;
  int walks = 0;
  for (uint32_t logn : {8u, 9u, 12u, 13u, 16u})
    for (int bits : {32, 64}) {
      // batch 0, 1 and around a workgroup boundary: per entries fill one workgroup
      const size_t per = ctlin_grid(1, logn, bits).per;
      for (size_t batch : {(size_t)0, (size_t)1, per - 1, per, per + 1, 2 * per + 1, (size_t)9})
        for (uint32_t comps : {1u, 2u, 3u}) {
          if (walk(batch, logn, 3, comps, bits)) return 1;
          walks++;
        }
    }
  // the partial last workgroups, in the words of tests/ctlin_cases.py
  CHECK(ctlin_grid(1, 8, 32).per == 4 && ctlin_grid(1, 8, 32).tail == 64);
  CHECK(ctlin_grid(5, 8, 32).wgx == 2 && ctlin_grid(5, 8, 32).tail == 64);
  CHECK(ctlin_grid(5, 8, 64).wgx == 3 && ctlin_grid(5, 8, 64).tail == 128);
  CHECK(ctlin_grid(5, 9, 32).per == 2 && ctlin_grid(5, 9, 64).per == 1);
  CHECK(ctlin_grid(5, 9, 64).tail == 0 && ctlin_grid(3, 12, 32).tail == 0);
  // sizes past 2^32 words.  No memory is touched: the counts and offsets alone
  {
    const uint32_t n = 65536, L = 60;
    const size_t batch = 2048;
    size_t cw[3], tw[2];
    ctlin_combine_words(L, n, batch, 3, cw);
    ctlin_tensor_words(L, n, batch, 3, tw);
    CHECK(cw[0] == batch * 3 * 60 * 65536 && cw[0] > ((size_t)1 << 32));
    CHECK(cw[1] == 60 && cw[2] == (size_t)60 * 65536);
    CHECK(tw[0] == cw[0] && tw[1] == batch * 3 * 2 * 60 * 65536 && tw[1] > ((size_t)1 << 33));
    // the last entry's offsets as the kernels form them
    const size_t p = batch - 1, comp = (size_t)L << 16;
    CHECK(ctlin_word_offset(p, 3, 2, L, 59, 16) + n == cw[0]);
    CHECK(ctlin_word_offset(p, 3, 0, L, 59, 16) + 2 * comp + n == cw[0]);
    CHECK(ctlin_word_offset(p, 3, 0, L, 0, 16) > ((size_t)1 << 32));
    const size_t x_off = ((p * 3 * 2 * L + 59) << 16);              // pair 0, component 0
    CHECK(x_off + (size_t)2 * 2 * comp + comp + n == tw[1]);        // pair 2, component 1
    CHECK(((p * 3 * L + 59) << 16) + 2 * comp + n == tw[0]);        // d_2
    const CtHighGrid G = ctlin_grid(batch, 16, 64);
    CHECK(G.ok && G.vectors == batch * 32768 && G.wgx == batch * 128 && G.tail == 0);
    // a batch whose workgroups no longer fit a grid dimension is refused, not wrapped
    CHECK(!ctlin_grid((size_t)1 << 34, 16, 64).ok && ctlin_grid((size_t)1 << 24, 16, 32).ok);
  }
  printf("ctlin sanitizer run ok: %d walks\n", walks);
  return 0;
}
