"""tests/galois_sweep.py held to what it claims, without a GPU: S(n) reaches every 2-adic valuation
of k - 1 and of k + 1 an odd k < 2n can have, at every n; the call lists hold S(n) exactly;
derived_perm, built on the oracle's forward transform, equals the mirror of galois_slot's formula
(tests/galois_ref.py) for every k of S(n) at n = 256 and 512, so that the data-derived table and
the formula's mirror agree before a kernel is judged by either; the library's host plan returns
k^-1 mod 2n; and every automorphism kernel the ledgers name is launched by a row of the sweep or
carries a stated exemption."""
import re

import numpy as np
import pytest

import galois_cases
import galois_ref
import galois_sweep as W
import hoist_cases
import hoist_ref as H
import ksntt_cases
import lintrans_cases
import nttmul
import rnsmp_cases


@pytest.mark.parametrize("n", W.ALL_N)
def test_sweep_reaches_every_valuation(n):
    ks = W.S(n)
    logn = n.bit_length() - 1
    assert len(set(ks)) == len(ks) and all(k % 2 == 1 and 0 < k < 2 * n for k in ks)
    want = set(range(1, logn + 2))
    assert {W.valuation(k - 1, n) for k in ks} == want
    assert {W.valuation(k + 1, n) for k in ks} == want
    structured = set()
    for j in range(1, logn + 1):
        structured |= {(1 << j) + 1, (1 << j) - 1, 2 * n - (1 << j) + 1, 2 * n - (1 << j) - 1}
    assert structured <= set(ks)
    if n == 256:
        assert ks == tuple(range(1, 512, 2))
    else:
        assert len(structured) < len(ks) <= len(structured) + W.DRAWN, "the drawn elements add"


@pytest.mark.parametrize("n", W.ALL_N)
def test_lists_hold_the_sweep_exactly(n):
    ls = W.lists(n)
    assert sum(len(l) for l in ls) == len(W.S(n))
    assert sorted(k for l in ls for k in l) == list(W.S(n))
    assert all(1 <= len(l) <= W.LIST for l in ls)
    (home,) = [l for l in ls if 1 in l]
    assert len(home) > 2 and home[0] != 1 and home[-1] != 1
    assert W.lists(n, 1) == [(k,) for k in W.S(n)]


@pytest.mark.parametrize("q", (rnsmp_cases.BASIS32[0], rnsmp_cases.BASIS64[0]))
@pytest.mark.parametrize("n", (256, 512))
def test_derived_perm_equals_the_formulas_mirror(n, q):
    dt = np.uint32 if q < 1 << 31 else np.uint64
    x = np.zeros((1, 1, n), dtype=dt)
    x[0, 0, 1] = 1
    fwd_x = H.forward(x, (q,))[0, 0]
    ks = W.S(n)
    imgs = np.stack([W.monomial_image(n, k, (q,), dt) for k in ks])
    for i, k in enumerate(ks):
        assert np.array_equal(imgs[i], galois_ref.coeff(x, k, (q,))[0])      # sigma_k(x), twice
    fwd = H.forward(imgs, (q,))
    for i, k in enumerate(ks):
        src = W.derived_perm(fwd_x, fwd[i, 0])
        assert np.array_equal(src, galois_ref.np_tables(n, k)[2]), k
    assert np.array_equal(W.derived_perm(fwd_x, fwd_x), np.arange(n))
    with pytest.raises(AssertionError):
        W.derived_perm(fwd_x, np.roll(fwd_x, 1) + np.arange(n, dtype=dt) % 2)


@pytest.mark.parametrize("n", W.ALL_N)
def test_the_librarys_plan_inverts_every_element(n):
    for k in W.S(n):
        src, neg, hat = nttmul.galois_plan(n, k)
        kinv = pow(k, -1, 2 * n)
        # coefficient j of sigma_k(a) is +-a[j k^-1 mod n], negated when j k^-1 mod 2n >= n
        for j in (1, 2, n // 2 + 1, n - 1):
            e = j * kinv % (2 * n)
            assert (int(src[j]), int(neg[j])) == (e % n, int(e >= n)), (k, j)
        assert int(src[1]) + n * int(neg[1]) == kinv
        assert sorted(hat.tolist()) == list(range(n))


def test_every_automorphism_kernel_has_a_row_or_an_exemption():
    named = set()
    for C in (galois_cases, hoist_cases, ksntt_cases, lintrans_cases):
        for case in C.all_cases():
            named |= {k for k in C.kernels_of(case) if k.startswith(W.PREFIXES)}
    assert named, "the mirrors name the automorphism kernels"
    swept = {k for row in W.rows() for k in W.kernels_of(row)}
    assert swept <= named, "the sweep launches only kernels the ledgers already name"
    exempt = set()
    for key in sorted(named - swept):
        reasons = [why for pattern, why in W.SWEEP_EXEMPT if re.search(pattern, key)]
        assert len(reasons) == 1 and reasons[0], f"{key}: no sweep row and no exemption"
        exempt.add(key)
    assert all(not re.search(p, k) for p, _ in W.SWEEP_EXEMPT for k in swept)
    # the one exemption: a component count of 1, whose gather code is the other count's
    assert exempt and all(re.sub(r",1>$", ",2>", k) in swept or
                          re.sub(r",1,([01])>$", r",2,\1>", k) in swept for k in exempt)
    assert {r.op for r in W.rows()} == set(W.OPS)
    assert len(W.rows()) == 2 * sum(map(len, W.OPS.values()))
