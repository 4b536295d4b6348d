"""The identities include/nttmul_galois.h states, checked in Python integers on tests/galois_ref.py
(the reference the GPU tests compare against) and the CPU oracle, and nttmul_galois_plan (the index
arithmetic of the kernels, restated on the host) against that reference.  No GPU."""
import numpy as np
import pytest

import galois_cases as C
import galois_ref as ref
import nttmul
from oracle import oracle as O

N = (256, 1024)
MODULI = (C.BASES[0][0], C.BASES[1][0])      # one modulus per word class


def _ks(n):
    return (3, 5, n - 1, n + 1, 2 * n - 1, pow(5, 7, 2 * n))


def _forward(P, a):
    """The forward transform nttmul_forward is held to (tests/test_gpu_parity.py
    test_transforms_vs_oracle)."""
    return [int(x) for x in P.transform("mulntt_ct_std2rev", a, "mixed_powers_rev")]


def _random(rng, n, q):
    a = [int(x) for x in rng.integers(0, q, size=n, dtype=np.uint64)]
    a[int(rng.integers(n))] = 0
    a[int(rng.integers(n))] = q - 1
    return a


@pytest.mark.parametrize("q", MODULI)
@pytest.mark.parametrize("n", N)
def test_slot_j_of_the_forward_transform_is_a_at_psi_to_2_brv_j_plus_1(n, q):
    P = O.Plan(n, q)
    a = _random(np.random.default_rng(n), n, q)
    hat, E = _forward(P, a), ref.exponents(n)
    for j in (0, 1, 2, n // 2 - 1, n // 2, n - 1):
        x = pow(P.psi, E[j], q)
        assert hat[j] == sum(c * pow(x, i, q) for i, c in enumerate(a)) % q


@pytest.mark.parametrize("q", MODULI)
@pytest.mark.parametrize("n", N)
def test_forward_of_sigma_is_sigma_of_forward(n, q):
    P = O.Plan(n, q)
    a = _random(np.random.default_rng(n + 1), n, q)
    hat = _forward(P, a)
    for k in _ks(n):
        assert _forward(P, ref.coeff_one(a, k, q)) == ref.ntt_one(hat, k), k


@pytest.mark.parametrize("q", MODULI)
@pytest.mark.parametrize("n", N)
def test_sigma_composes_and_is_a_ring_homomorphism(n, q):
    P = O.Plan(n, q)
    rng = np.random.default_rng(n + 2)
    a, b = _random(rng, n, q), _random(rng, n, q)
    ab = [int(x) for x in P.product_merged(a, b)]
    hat = _forward(P, a)
    ks = _ks(n)
    for k, m in zip(ks, ks[1:] + ks[:1]):
        km = k * m % (2 * n)
        assert ref.coeff_one(ref.coeff_one(a, m, q), k, q) == ref.coeff_one(a, km, q)
        assert ref.ntt_one(ref.ntt_one(hat, m), k) == ref.ntt_one(hat, km)
        sa, sb = ref.coeff_one(a, k, q), ref.coeff_one(b, k, q)
        assert [int(x) for x in P.product_merged(sa, sb)] == ref.coeff_one(ab, k, q)
    assert ref.coeff_one(a, 1, q) == a and ref.ntt_one(hat, 1) == hat


def test_array_forms_equal_the_scalar_forms():
    n, moduli = 256, C.BASES[1]
    x = ref.random_words(np.random.default_rng(3), moduli, 2, n, np.uint64)
    for l, q in enumerate(moduli):      # the planted words: -0 and the largest negation
        assert (x[:, l, :] == 0).any(axis=1).all() and (x[:, l, :] == q - 1).any(axis=1).all()
    for k in (3, 2 * n - 1):
        c, h = ref.coeff(x, k, moduli), ref.ntt(x, k)
        assert c.dtype == h.dtype == np.uint64 and c.shape == h.shape == x.shape
        for p in range(2):
            for l, q in enumerate(moduli):
                assert [int(v) for v in c[p, l]] == ref.coeff_one(x[p, l], k, q)
                assert [int(v) for v in h[p, l]] == ref.ntt_one(x[p, l], k)


@pytest.mark.parametrize("n", C.ALL_N)
def test_plan_equals_the_reference_tables(n):
    for k in sorted({1, 3, n + 1, 2 * n - 1, pow(5, 7, 2 * n), ref.element(n, -3)}):
        src, neg, hat = nttmul.galois_plan(n, k)
        want = ref.tables(n, k)
        assert src.dtype == hat.dtype == np.uint32 and neg.dtype == np.uint8
        assert (src.tolist(), neg.tolist(), hat.tolist()) == tuple(want), (n, k)
    src, neg, hat = nttmul.galois_plan(n, 1)
    assert src.tolist() == hat.tolist() == list(range(n)) and not neg.any()


@pytest.mark.parametrize("n", C.ALL_N)
def test_ntt_src_maps_aligned_blocks_onto_aligned_blocks(n):
    """What the kernels rely on for coalescing: the slots of an aligned block of 2^m (a wave's 64,
    a workgroup slice's 256) come from one aligned block of 2^m, each of its slots once."""
    for k in (3, n - 1, 2 * n - 1, ref.element(n, 1)):
        hat = nttmul.galois_plan(n, k)[2].astype(np.int64)
        for m in (6, 8):
            blocks = (hat >> m).reshape(-1, 1 << m)
            assert (blocks == blocks[:, :1]).all(), (n, k, m)
            assert (np.sort(hat.reshape(-1, 1 << m) & ((1 << m) - 1), axis=1)
                    == np.arange(1 << m)).all()
            assert sorted(blocks[:, 0].tolist()) == list(range(n >> m))


def test_element_of_the_reference():
    for n in C.ALL_N:
        assert ref.element(n, 0) == 1 and ref.element(n, 1) == 5
        assert ref.element(n, 1) * ref.element(n, -1) % (2 * n) == 1
        assert ref.element(n, 0, True) == 2 * n - 1
        assert ref.element(n, n // 2) == 1          # 5 has order n / 2 mod 2n
