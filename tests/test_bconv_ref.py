"""The identities include/nttmul_bconv.h states, checked in Python integers on tests/bconv_ref.py
(the reference the GPU tests compare against).  No GPU."""
import random
from math import prod

import pytest

import bconv_ref as R

# (bits, L, K): 5 + 4 primes just below 2^31, 17 + 7 just below 2^62, single-prime bases
BASES = [(31, 5, 4), (62, 17, 7), (31, 1, 3), (62, 1, 1), (31, 3, 1)]


def _bases(bits, L, K):
    p = R.primes_below(1 << bits, R.STEP, L + K)
    return p[:L], p[L:]


def _inputs(rng, from_q, count=40):
    edge = [R.worst_case(from_q), [0] * len(from_q), [b - 1 for b in from_q]]
    return edge + [[rng.randrange(b) for b in from_q] for _ in range(count)]


def test_primes_below_walks_down_in_steps():
    p = R.primes_below(1 << 31, R.STEP, 6)
    assert p == sorted(p, reverse=True) and len(set(p)) == 6 and p[0] < (1 << 31)
    assert all((q - 1) % R.STEP == 0 for q in p)
    assert p[0] == 2147377153           # the largest prime = 1 mod 8192 below 2^31
    assert all(q >= (1 << 61) for q in R.primes_below(1 << 62, R.STEP, 24))


@pytest.mark.parametrize("bits,L,K", BASES)
def test_sum_is_x_plus_alpha_b(bits, L, K):
    """sum_i y_i Bh_i = x + alpha B with x the CRT value and 0 <= alpha < L."""
    from_q, to_q = _bases(bits, L, K)
    B, rng = prod(from_q), random.Random(bits * 100 + L)
    for x in _inputs(rng, from_q):
        s, v = R.conv_sum(x, from_q), R.crt(x, from_q)
        alpha, rem = divmod(s - v, B)
        assert rem == 0 and 0 <= alpha < L
        inv, _, _ = R.constants(from_q, to_q)
        ys = [xi * k % b for xi, k, b in zip(x, inv, from_q)]
        assert alpha == sum(y * (B // b) for y, b in zip(ys, from_q)) // B      # floor(sum y_i / b_i)
        assert R.convert_one(x, from_q, to_q) == [(v + alpha * B) % c for c in to_q]


@pytest.mark.parametrize("bits,L,K", BASES)
def test_moddown_is_floor_minus_alpha(bits, L, K):
    """moddown = (floor(X / B) - alpha) mod c_j; alpha = 0 and the rescale is exact for L = 1."""
    from_q, to_q = _bases(bits, L, K)
    B, C, rng = prod(from_q), prod(to_q), random.Random(bits * 100 + K)
    for _ in range(40):
        X = rng.randrange(B * C)
        x = [X % c for c in to_q] + [X % b for b in from_q]
        alpha = (R.conv_sum(x[K:], from_q) - X % B) // B
        assert 0 <= alpha < L and (L > 1 or alpha == 0)
        assert R.moddown_one(x, from_q, to_q) == [(X // B - alpha) % c for c in to_q]
    Z = rng.randrange(C)                # a multiple of B comes back exactly, for any L
    X = B * Z
    x = [X % c for c in to_q] + [0] * L
    assert R.moddown_one(x, from_q, to_q) == [Z % c for c in to_q]


@pytest.mark.parametrize("bits,L,K", BASES)
def test_worst_case_input_maximises_every_y(bits, L, K):
    """x[i] = -Bh_i mod b_i gives every y_i = b_i - 1 and alpha = L - 1."""
    from_q, to_q = _bases(bits, L, K)
    B = prod(from_q)
    x = R.worst_case(from_q)
    inv, _, _ = R.constants(from_q, to_q)
    assert [xi * k % b for xi, k, b in zip(x, inv, from_q)] == [b - 1 for b in from_q]
    assert (R.conv_sum(x, from_q) - R.crt(x, from_q)) // B == L - 1


def test_array_forms_equal_the_scalar_forms():
    import numpy as np
    from_q, to_q = _bases(62, 3, 2)
    x = R.random_words(np.random.default_rng(7), tuple(to_q) + tuple(from_q), 2, 8, np.uint64)
    conv, down = R.convert(x[:, 2:, :], from_q, to_q), R.moddown(x, from_q, to_q)
    assert conv.dtype == np.uint64 and conv.shape == (2, 2, 8) == down.shape
    for p in range(2):
        for k in range(8):
            assert list(conv[p, :, k]) == R.convert_one(list(x[p, 2:, k]), from_q, to_q)
            assert list(down[p, :, k]) == R.moddown_one(list(x[p, :, k]), from_q, to_q)


def test_unfolded_sums_overflow_where_the_cadence_tests_say():
    """The lengths tests/bconv_cases.py names: five products of the top 32-bit primes overflow 64
    bits where four fit, seventeen of the top 64-bit primes overflow 128 bits where sixteen fit."""
    for bits, acc, fits in ((31, 64, 4), (62, 128, 16)):
        p = R.primes_below(1 << bits, R.STEP, fits + 3)
        c = p[fits + 1]
        assert sum((b - 1) * (c - 1) for b in p[:fits]) < (1 << acc)
        assert sum((b - 1) * (c - 1) for b in p[:fits + 1]) >= (1 << acc)
