"""The closed form behind tests/test_gpu_saturation.py, checked on the CPU: for every member of
the family S(m, v) (tests/saturation.py) up to n = 1024 the expectation generator equals the
oracle's product, so the GPU test's expected values are themselves tested without a GPU."""
import numpy as np
import pytest

import dispatch_cases as D
import nttmul
import saturation as S
from oracle import oracle as O


def test_ones_conv_is_numpy_s_convolution():
    for ma, mb in ((1, 1), (1, 8), (8, 1), (4, 4), (3, 7), (256, 256), (512, 64)):
        want = np.convolve(np.ones(ma, np.int64), np.ones(mb, np.int64))
        got = S.ones_conv(ma, mb, 2 * max(ma, mb))
        assert np.array_equal(got[:len(want)], want) and not got[len(want):].any()


@pytest.mark.parametrize("n,q", [(n, q) for n in (256, 1024) for q in D.sat_moduli(n)])
def test_closed_form_equals_the_oracle_product(n, q):
    P = O.Plan(n, q)
    a, b, c = S.family(n, q)
    assert len(a) == 2 * len(S.sizes(n)) and S.sizes(n)[-1] == n
    for i in range(len(a)):
        assert np.array_equal(c[i], P.product_merged(a[i], b[i])), (n, q, i)
    # mixed sizes and values too: the general form the family is a diagonal of
    rng = np.random.default_rng(n)
    for ma, mb in ((1, n), (n, 1), (4, 8), (8, 4), (n // 2, n), (n, n // 4)):
        va, vb = int(rng.integers(1, q)), q - 1
        assert np.array_equal(S.product(n, q, ma, va, mb, vb),
                              P.product_merged(S.poly(n, ma, va), S.poly(n, mb, vb))), (ma, mb)


def test_case_table():
    assert {n: nttmul.find_prime(n, 31) for n in D.SAT_N} == D.SAT_P31
    assert all((q - 1) % (2 * n) == 0 for n in D.SAT_N for q in D.sat_moduli(n))
    prods = D.sat_products()
    assert (4096, D.Q31HI, 64) in prods and (8192, D.Q32, 64) in prods
    assert (1024, D.Q31HI, 64) not in prods and (65536, D.Q62, 32) not in prods
    assert len(prods) == len(set(prods))
    launched = {k for c in D.new_cases() for k in D.kernels_of(c)}
    for n, q, w in prods:
        assert set(D.product_keys(D.Case("multiply", n, q, w, D.sat_batch(n)))) <= launched
