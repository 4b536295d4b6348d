"""tests/ksntt_ref.py against the references it stands beside, at n = 256 in Python integers:
identity (A), modup from the header's formula equals forward(ks_ref.modup(mdntt_ref.inverse(.)));
identity (B), mac from its formula equals forward(hoist_ref.hoist(.)), and with one term against
an operand of ones it is galois_ref.ntt.  No GPU."""
import numpy as np
import pytest

import bconv_ref as B
import galois_ref
import hoist_ref as H
import ks_ref
import ksntt_ref as ref
import mdntt_ref

N = 256
SHAPES = ((4, 2, 2), (5, 2, 2), (3, 1, 1), (3, 2, 3))


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("L,K,alpha", SHAPES)
def test_modup_formula_equals_the_composition(L, K, alpha, bits):
    q, p = ks_ref.bases(bits, L, K)
    x_hat = B.random_words(np.random.default_rng(100 * L + 10 * K + alpha + bits), q, 2, N, _dt(bits))
    for l, m in enumerate(q):                # the ends of every limb's range
        x_hat[0, l, 0], x_hat[0, l, 1] = 0, m - 1
    got = ref.modup(x_hat, q, p, alpha)
    dn = -(-L // alpha)
    assert got.dtype == _dt(bits) and got.shape == (2, dn, L + K, N)
    assert np.array_equal(got, ref.modup_composition(x_hat, q, p, alpha))
    assert all(int(got[:, :, l].max()) < m for l, m in enumerate(q + p))
    # a digit's own limbs are the input itself; every other limb is not (random input)
    for d, D in enumerate(ks_ref.digits(L, alpha)):
        for m in range(L):
            assert np.array_equal(got[:, d, m], x_hat[:, m]) == (m in D)
    # and the inverse under it is mdntt_ref's: coefficient order back and forth
    assert np.array_equal(H.forward(mdntt_ref.inverse(x_hat, q), q), x_hat)


@pytest.mark.parametrize("bits", (32, 64))
def test_modup_worst_case_input_is_the_accumulators(bits):
    L, K, alpha = 5, 2, 2
    q, p = ks_ref.bases(bits, L, K)
    x_hat = ref.worst_x_hat(q, alpha, 1, N, _dt(bits))
    want = np.array(ks_ref.worst_case(q, alpha), dtype=object)
    assert (mdntt_ref.inverse(x_hat, q)[0].astype(object) == want[:, None]).all()
    assert np.array_equal(ref.modup(x_hat, q, p, alpha), ref.modup_composition(x_hat, q, p, alpha))


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("L,K,alpha", SHAPES)
def test_mac_formula_equals_forward_of_hoist(L, K, alpha, bits):
    q, p = ks_ref.bases(bits, L, K)
    ext, terms = q + p, -(-L // alpha)
    rng = np.random.default_rng(L + K + alpha + bits)
    ks = (1, 5, 2 * N - 1)
    a_hat = B.random_words(rng, ext * terms, 2, N, _dt(bits)).reshape(2, terms, L + K, N)
    b_hat = B.random_words(rng, ext * (terms * 2), len(ks), N, _dt(bits)).reshape(
        len(ks), 2, terms, L + K, N)
    a_hat[0, 0, :, 0] = [m - 1 for m in ext]
    b_hat[0, 0, 0, :, 0] = [m - 1 for m in ext]
    got = ref.mac(a_hat, b_hat, ks, ext)
    assert got.dtype == _dt(bits) and got.shape == (2, len(ks), 2, L + K, N)
    assert np.array_equal(got, ref.mac_composition(a_hat, b_hat, ks, ext))
    assert all(int(got[..., l, :].max()) < m for l, m in enumerate(ext))


@pytest.mark.parametrize("bits", (32, 64))
def test_mac_against_ones_is_the_slot_permutation(bits):
    q, p = ks_ref.bases(bits, 2, 1)
    ext = q + p
    a_hat = B.random_words(np.random.default_rng(bits), ext, 2, N, _dt(bits))
    ones = np.ones((1, 1, 1, 3, N), dtype=_dt(bits))
    for k in (1, 5, 2 * N - 1, 25):
        got = ref.mac(a_hat[:, None], ones, (k,), ext)[:, 0, 0]
        assert np.array_equal(got, galois_ref.ntt(a_hat, k))
