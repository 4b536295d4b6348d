"""tests/hoist_ref.py held to its definitions and to the key-switch identity, in Python integers on
the CPU oracle.  No GPU: the reference the GPU chain is compared with bit for bit
(tests/test_gpu_hoist.py) must itself stay within the bound for the seeds used."""
import numpy as np
import pytest

import bconv_ref as B
import galois_ref
import hoist_cases as C
import hoist_ref as H
import rns_cases as R


@pytest.mark.parametrize("moduli", (R.BASIS32[:2], R.BASIS64[:2]), ids=("u32", "u64"))
def test_hoist_is_the_mac_of_the_rotated_polynomial(moduli):
    """hoist(forward(a), b_hat, k)[:, r, i] = INTT(forward(sigma_k(a)) o b_hat[r][i]), with sigma_k
    applied in coefficient order by tests/galois_ref.py; k = 1 is the plain pointwise mac; and the
    result is the negacyclic product of sigma_k(a) with the polynomial b_hat transforms."""
    n, batch, terms = 256, 2, 2
    dt = np.uint32 if max(moduli) < 1 << 32 else np.uint64
    ks = (1, 5, 2 * n - 1)
    rng = np.random.default_rng(len(moduli) + int(moduli[0] % 97))
    a = B.random_words(rng, moduli, batch * terms, n, dt).reshape(batch, terms, len(moduli), n)
    b = B.random_words(rng, moduli, len(ks) * 2 * terms, n, dt).reshape(
        len(ks), 2, terms, len(moduli), n)
    a_hat, b_hat = H.forward(a, moduli), H.forward(b, moduli)
    got = H.hoist(a_hat, b_hat, ks, moduli)
    assert got.shape == (batch, len(ks), 2, len(moduli), n) and got.dtype == dt
    for r, k in enumerate(ks):
        ar = galois_ref.coeff(a.reshape(-1, len(moduli), n), k, moduli).reshape(a.shape)
        plain = H.hoist(H.forward(ar, moduli), b_hat[r:r + 1], (1,), moduli)
        assert np.array_equal(got[:, r], plain[:, 0]), k
        for l, q in enumerate(moduli):                     # and against the oracle's product
            want = sum(H.plan(n, q).product_merged(ar[0, t, l], b[r, 1, t, l]).astype(object)
                       for t in range(terms)) % q
            assert np.array_equal(got[0, r, 1, l], want.astype(dt)), (k, l)
    assert not np.array_equal(got[:, 0], got[:, 1]) and not np.array_equal(got[:, :, 0],
                                                                            got[:, :, 1])


def test_rotate_signed_is_galois_ref_on_signed_coefficients():
    n, q = 256, 12289
    rng = np.random.default_rng(1)
    s = [int(v) for v in rng.integers(-1, 2, size=n)]
    for k in C.pool(n):
        want = galois_ref.coeff_one([v % q for v in s], k, q)
        assert [v % q for v in H.rotate_signed(s, k)] == want
    assert H.rotate_signed(s, 1) == s


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,kind", C.CHAIN)
def test_the_reference_chain_stays_within_the_bound(n, kind, bits):
    """c_0 + c_1 s - sigma_k(x) sigma_k(s2) within +-(K + 1)(1 + h) per coefficient, for every
    batch entry and rotation, at the degrees, classes and seeds of the GPU test."""
    L, K, alpha = C.CHAIN_SHAPE
    ch = H.chain(n, bits)
    assert C.family(n) == kind and 2 * n - 1 in ch["ks"] and len(ch["ks"]) == C.CHAIN_ROTS
    assert ch["out"].shape == (C.CHAIN_BATCH, C.CHAIN_ROTS, 2, L, n)
    assert ch["mid"].shape == (C.CHAIN_BATCH, C.CHAIN_ROTS, 2, L + K, n)
    errs = H.chain_errors(ch)
    assert len(errs) == C.CHAIN_BATCH * C.CHAIN_ROTS
    assert max(errs) <= H.chain_bound() == 27, errs
    # the rotations' keys and results differ, so a swapped rotation or component would show
    for r in range(1, C.CHAIN_ROTS):
        assert not np.array_equal(ch["out"][:, 0], ch["out"][:, r])
    assert not np.array_equal(ch["out"][:, :, 0], ch["out"][:, :, 1])
    # and the identity is not vacuous: with a rotation's halves swapped it fails by far
    swapped = np.ascontiguousarray(ch["out"][:, :, ::-1])
    assert min(H.chain_errors(ch, swapped)) > 1 << 20
