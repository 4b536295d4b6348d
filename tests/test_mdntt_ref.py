"""tests/mdntt_ref.py against itself: the composition (the oracle's per-limb transforms around
bconv_ref.moddown) agrees at n = 256 with the NTT-domain formula of include/nttmul_mdntt.h computed
independently of it, and for K = 1 with NTT(floor(X / p) mod q_l) on random big integers X.
No GPU."""
from math import prod

import numpy as np
import pytest

import bconv_ref as B
import ks_ref
import mdntt_ref as ref

N = 256


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("L,K", ((1, 1), (3, 2), (2, 5)))
def test_composition_equals_the_ntt_domain_formula(L, K, bits):
    q, p = ks_ref.bases(bits, L, K)
    x_hat = B.random_words(np.random.default_rng(L * 10 + K + bits), q + p, 2, N, _dt(bits))
    for l, m in enumerate(q + p):            # the ends of every limb's range
        x_hat[0, l, 0], x_hat[0, l, 1] = 0, m - 1
    got = ref.moddown(x_hat, q, p)
    assert got.dtype == _dt(bits) and got.shape == (2, L, N)
    assert np.array_equal(got, ref.formula(x_hat, q, p))
    assert all(int(got[:, l].max()) < m for l, m in enumerate(q))


def test_transforms_invert_each_other():
    q, p = ks_ref.bases(64, 2, 1)
    x = B.random_words(np.random.default_rng(1), q + p, 1, N, np.uint64)
    assert np.array_equal(ref.inverse(ref.forward(x, q + p), q + p), x)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("L", (1, 3))
def test_rescale_is_the_exact_floor(L, bits):
    """K = 1: out = NTT(floor(X / p) mod q_l) for the CRT value X over Q u {p}."""
    q, p = ks_ref.bases(bits, L, 1)
    ext = q + p
    X = ref.big_integers(np.random.default_rng(L + bits), N, prod(ext))
    assert X[0] == 0 and X[1] == prod(ext) - 1 and all(0 <= v < prod(ext) for v in X)
    x_hat = ref.forward(ref.residues(X, ext, _dt(bits))[None], ext)
    want = ref.forward(ref.rescale_floor(X, q, p[0]).astype(_dt(bits))[None], q)
    assert np.array_equal(ref.moddown(x_hat, q, p), want)
    # and the floor is the CRT value's: (X - X mod p) / p
    assert all((v - v % p[0]) // p[0] % q[0] == int(ref.rescale_floor(X, q, p[0])[0][i])
               for i, v in enumerate(X))
