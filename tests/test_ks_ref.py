"""tests/ks_ref.py held to the definitions of include/nttmul_ks.h, in Python integers, without a
GPU and without the library's kernels: the digit's own limbs pass through, every digit's output is
x_d + u D_d with 0 <= u < |D_d|, the worst case reaches u = |D_d| - 1, and modup, a key built from
the gadget factors, the per-limb products and moddown make a hybrid key switch (the identity
test_gpu_ks.py asserts on the device, here at n = 16)."""
from math import prod

import numpy as np
import pytest

import bconv_ref as B
import ks_ref as ref

SHAPES = ((1, 1, 1), (4, 2, 2), (5, 2, 2), (5, 3, 5), (6, 1, 1), (3, 2, 2))


def _dtype(bits):
    return np.uint32 if bits == 32 else np.uint64


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("shape", SHAPES)
def test_modup_is_the_headers_formula(bits, shape):
    L, K, alpha = shape
    q, p = ref.bases(bits, L, K)
    assert all((m - 1) % ref.STEP == 0 for m in q + p) and len(set(q + p)) == L + K
    n, batch = 8, 2
    x = B.random_words(np.random.default_rng(L * 100 + K), q, batch, n, _dtype(bits))
    up = ref.modup(x, q, p, alpha)
    D = ref.digits(L, alpha)
    assert up.shape == (batch, len(D), L + K, n) and up.dtype == x.dtype
    assert len(D) == -(-L // alpha) and sum(len(d) for d in D) == L
    ext = q + p
    for d, rng in enumerate(D):
        own = [q[i] for i in rng]
        # own limbs equal the input
        assert np.array_equal(up[:, d, rng.start:rng.stop, :], x[:, rng.start:rng.stop, :])
        for b in range(batch):
            for k in range(n):
                xd = B.crt([x[b, i, k] for i in rng], own)
                assert B.crt([up[b, d, i, k] for i in rng], own) == xd
                # one integer x_d + u D_d gives every limb of the output
                s = B.conv_sum([x[b, i, k] for i in rng], own)
                u, r = divmod(s - xd, prod(own))
                assert r == 0 and 0 <= u < len(own)
                assert [int(v) for v in up[b, d, :, k]] == [s % m for m in ext]


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("shape", SHAPES)
def test_worst_case_reaches_the_largest_multiple(bits, shape):
    L, K, alpha = shape
    q, p = ref.bases(bits, L, K)
    x = ref.worst_case(q, alpha)
    assert len(x) == L and all(0 <= v < m for v, m in zip(x, q))
    for rng in ref.digits(L, alpha):
        own = [q[i] for i in rng]
        Dd = prod(own)
        ys = [x[i] * pow(Dd // q[i], -1, q[i]) % q[i] for i in rng]
        assert ys == [m - 1 for m in own]
        s = B.conv_sum([x[i] for i in rng], own)
        assert (s - B.crt([x[i] for i in rng], own)) // Dd == len(own) - 1


@pytest.mark.parametrize("bits", (32, 64))
def test_constants_and_gadget(bits):
    for L, K, alpha in SHAPES:
        q, p = ref.bases(bits, L, K)
        inv, w, g, pinv, pw, Pinv = ref.constants(q, p, alpha)
        assert (pinv, pw, Pinv) == B.constants(p, q)
        P = prod(p)
        for d, rng in enumerate(ref.digits(L, alpha)):
            # the gadget is P on the digit's own limbs and 0 on every other limb of Q u P
            assert g[d] == [P % q[i] if i in rng else 0 for i in range(L)] + [0] * K
            Dd = prod(q[i] for i in rng)
            for i in rng:
                assert inv[i] * (Dd // q[i]) % q[i] == 1
                assert w[i] == [(Dd // q[i]) % m for m in q + p]
                assert all(w[i][m] == 0 for m in rng if m != i)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("shape", ((4, 2, 2), (5, 2, 2), (3, 1, 3), (4, 3, 1)))
def test_key_switch_identity_in_python(bits, shape):
    L, K, alpha = shape
    n, h, batch = 16, 8, 2
    q, p = ref.bases(bits, L, K)
    ext = q + p
    rng = np.random.default_rng(7 * L + K + bits)
    s, s2 = ref.ternary(rng, n, h), ref.ternary(rng, n, h)
    key = ref.keygen(rng, n, q, p, alpha, s, s2)
    x = B.random_words(rng, q, batch, n, _dtype(bits))
    up = ref.modup(x, q, p, alpha)
    c = []
    for comp in key:
        acc = np.zeros((batch, L + K, n), dtype=object)
        for b in range(batch):
            for l, m in enumerate(ext):
                acc[b, l] = sum(ref.negacyclic([int(v) for v in up[b, d, l]], comp[d, l], m)
                                for d in range(up.shape[1])) % m
        c.append(B.moddown(acc.astype(_dtype(bits)), p, q))
    bound = (K + 1) * (1 + h)
    for b in range(batch):
        assert ref.key_switch_error(x[b], c[0][b], c[1][b], q, s, s2) <= bound
