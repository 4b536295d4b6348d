"""Why the NTT-domain libraries are held to the CPU reference on every output word
(tests/full_ref.py), on the references alone: no GPU.

The conversions (mdntt, xconv, tmd) work per coefficient between an inverse and a forward
transform.  An error at one coefficient spreads over the whole NTT-domain output, and a test's own
inverse transform brings it back to that one coefficient: the comparison on
xconv_cases.sample_indices, 66 coefficients of n, sees it only if the position is sampled.  Here
the reference output at n = 8192 gets one coefficient-domain value changed and is transformed
forward again:

* at a position outside the sample, one in each residue class modulo 64 -- the sampled comparison
  accepts the wrong output and the full comparison rejects it;
* at the first and the last coefficient, which the sample always holds -- both reject it.

And the exact arithmetic that makes the references cheap enough to run ungated is held to Python
integers: hoist_ref.mulmod's C product on 64-bit words, ksntt_ref.mac's uint64 sums."""
import numpy as np
import pytest

import bconv_ref as B
import full_ref as F
import hoist_ref as H
import ks_ref
import ksntt_ref
import mdntt_cases as MC
import tmd_cases as TC
import xconv_cases as XC

N = 8192
L, K = MC.DEGREE_SHAPE


def _inputs(library, op, bits):
    """(x_hat, q, p, t) of the library's own degree-sweep case at n = 8192, one polynomial."""
    if library == "mdntt":
        case = MC.Case(bits, N, 1, L, K)
        q, p = MC.moduli_of(case)
        dt = np.uint32 if bits == 32 else np.uint64
        return B.random_words(np.random.default_rng(N + bits), q + p, 1, N, dt), q, p, 1
    if library == "xconv":
        case = XC.Case(op, bits, N, 1, L, K, 65537)
        return (XC.seeded_input(case),) + tuple(XC.moduli_of(case)) + (case.t,)
    t = TC.plain_moduli(bits)[0]
    case = TC.Case(bits, N, 1, L, K, t)
    return (TC.seeded_input(case),) + tuple(TC.moduli_of(case)) + (t,)


def _positions(n):
    """One position outside the sample in each residue class modulo 64, the smallest."""
    sampled = set(XC.sample_indices(n))
    out = []
    for r in range(64):
        out.append(next(k for k in range(r, n, 64) if k not in sampled and 0 < k < n - 1))
    assert len({k % 64 for k in out}) == 64 and not set(out) & sampled
    return out


def test_the_sample_is_66_coefficients_whatever_the_degree():
    assert len(XC.sample_indices(256)) >= 64 and {0, 255} <= set(XC.sample_indices(256))
    for n in XC.ALL_N:
        idx = XC.sample_indices(n)
        assert {i * 64 // n for i in idx} == set(range(64)) and {0, n - 1} <= set(idx)
        assert len(idx) <= 66
    assert 100 * len(XC.sample_indices(N)) < N          # under 1 % at n = 8192


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("library,op", (("mdntt", "moddown"), ("xconv", "extend"),
                                        ("xconv", "moddown"), ("tmd", "moddown")))
def test_one_wrong_coefficient_passes_the_sample_and_fails_the_full_comparison(library, op, bits):
    x_hat, q, p, t = _inputs(library, op, bits)
    want_coef, want = F.conversion(library, op, x_hat, q, p, t)
    args = (x_hat, q, p) + (() if library == "mdntt" else (t,))
    assert want.shape == (1, L, N) and F.equal(want, F.reference(library, op, *args))
    idx = XC.sample_indices(N)
    assert F.sampled_equal(want, want_coef, q, idx) and F.equal(want, want)

    def wrong(k, l):
        """The reference output with coefficient k of limb l off by one, in the NTT domain."""
        coef = want_coef.copy()
        coef[0, l, k] = (int(coef[0, l, k]) + 1) % q[l]
        bad = want.copy()
        bad[0, l] = H.forward(coef[:, l:l + 1], (q[l],))[0, 0]
        # one coefficient spreads over the limb's whole transform
        assert np.count_nonzero(bad[0, l] != want[0, l]) > N // 2
        return bad

    for i, k in enumerate(_positions(N)):
        bad = wrong(k, i % L)
        assert F.sampled_equal(bad, want_coef, q, idx), (k, "the sample sees an unsampled position")
        assert not F.equal(bad, want), k
        assert F.mismatches(bad, want)[1][0][:2] == (0, i % L)
    for k in (0, N - 1):                                # always sampled: both comparisons see them
        bad = wrong(k, L - 1)
        assert not F.sampled_equal(bad, want_coef, q, idx), k
        assert not F.equal(bad, want), k


def test_equal_is_strict_about_shape_and_type():
    a = np.arange(12, dtype=np.uint32).reshape(1, 3, 4)
    assert F.equal(a, a.copy())
    assert not F.equal(a, a.astype(np.uint64)) and not F.equal(a, a.reshape(3, 4))
    b = a.copy()
    b[0, 2, 3] ^= 1
    assert not F.equal(a, b) and F.mismatches(a, b) == (1, [(0, 2, 3)])
    with pytest.raises(AssertionError):
        F.assert_equal(a, b, "here")


def test_no_case_is_on_the_subset_list():
    """The README names the subset cases; there are none, and the ledgers rely on it."""
    assert set(F.SUBSET) == set(F.LIBRARIES) and not any(F.SUBSET.values())
    assert not F.on_subset("ksntt", object())


@pytest.mark.parametrize("bits", (32, 64))
def test_the_c_product_is_the_python_integer_product(bits):
    q, p = ks_ref.bases(bits, 3, 2)
    rng = np.random.default_rng(bits)
    for m in q + p:
        x = rng.integers(0, m, size=4096, dtype=np.uint64)
        y = rng.integers(0, m, size=4096, dtype=np.uint64)
        x[:4], y[:4] = (0, 1, m - 1, m - 1), (m - 1, m - 1, m - 1, 1)
        want = H.mulmod_py(x, y, m)
        assert int(want[2]) == 1 and np.array_equal(H.mulmod_c(x, y, m), want)
        assert x.size >= H.MULMOD_C_WORDS and np.array_equal(H.mulmod(x, y, m), want)
        assert np.array_equal(H.mulmod(x[:64], y[:64], m), want[:64])


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n", (256, 4096))
def test_the_exact_mac_is_the_python_integer_mac(n, bits):
    """n = 4096: a batch of three passes MULMOD_C_WORDS, the C product's path on 64-bit words."""
    q, p = ks_ref.bases(bits, 2, 1)
    ext, rng = q + p, np.random.default_rng(n + bits)
    dt = np.uint32 if bits == 32 else np.uint64
    batch, terms, comps, ks = 3, 3, 2, (5, 2 * n - 1)
    a = B.random_words(rng, ext * terms, batch, n, dt).reshape(batch, terms, len(ext), n)
    b = B.random_words(rng, ext * (terms * comps), len(ks), n, dt).reshape(
        len(ks), comps, terms, len(ext), n)
    top = np.array([m - 1 for m in ext], dtype=dt)[:, None]
    a[0], b[0] = top, top                               # the largest products and sums
    got = ksntt_ref.mac(a, b, ks, ext)
    assert got.dtype == dt and np.array_equal(got, ksntt_ref.mac_python(a, b, ks, ext))
    assert (got[0, 0] == terms).all()
