"""tests/xconv_ref.py held to independent statements of the same things, without a GPU: big
integers through their residues, the K = 1 rounding, mdntt_ref's floor form (round - floor in
[0, K]), the table identities of nttmul_xconv_plan's constants, in_band in exact fractions; the
derivation of the chain bound (the rounded ModDown switches keys within less than (1 + h) / 2, the
floor form on the same data does not); and that no seeded input of the GPU tests has a coefficient
inside the guard band."""
from fractions import Fraction
from math import prod

import numpy as np
import pytest

import bconv_ref as B
import hoist_cases
import hoist_ref as H
import ks_ref
import mdntt_ref
import xconv_cases as C
import xconv_ref as ref

N = 256
EPS1 = Fraction(1, 1 << C.BAND_LOG2)


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


@pytest.mark.parametrize("t", (1, 65537, 1032193))
@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("L,K", ((1, 1), (3, 2), (2, 5)))
def test_both_operations_on_big_integers(L, K, bits, t):
    """X in [0, Q P) through its residues: moddown is round(t X / P), extend of the P part the
    centred residue of t X mod P, both modulo each q_l."""
    q, p = ks_ref.bases(bits, L, K)
    Q, P = prod(q), prod(p)
    rng = np.random.default_rng(L + 10 * K + bits + t)
    X = mdntt_ref.big_integers(rng, N, Q * P)
    x = mdntt_ref.residues(X, q + p, _dt(bits))[None]
    down = ref.moddown_coeff(x, q, p, t)[0].astype(object)
    up = ref.extend_coeff(x[:, L:], q, p, t)[0].astype(object)
    for k, v in enumerate(X):
        r = Fraction(t * v, P)
        near = r.numerator // r.denominator + (r - r.numerator // r.denominator > Fraction(1, 2))
        assert abs(Fraction(near) - r) < Fraction(1, 2)                 # P odd: never a tie
        c = t * v - near * P
        assert -(P - 1) // 2 <= c <= (P - 1) // 2 and (c - t * v) % P == 0
        for l, m in enumerate(q):
            assert down[l, k] == near % m and up[l, k] == c % m
    assert np.array_equal(down, ref.moddown_values(X, q, p, t))


@pytest.mark.parametrize("bits", (32, 64))
def test_the_rounded_rescale(bits):
    """t = 1, K = 1: round(X / p)."""
    q, p = ks_ref.bases(bits, 3, 1)
    rng = np.random.default_rng(bits)
    X = mdntt_ref.big_integers(rng, N, prod(q) * p[0])
    x = mdntt_ref.residues(X, q + p, _dt(bits))[None]
    want = [[((2 * v + p[0]) // (2 * p[0])) % m for v in X] for m in q]
    assert ref.moddown_coeff(x, q, p)[0].astype(object).tolist() == want
    assert all(abs(Fraction(2 * v + p[0], 2 * p[0]).__floor__() * p[0] - v) * 2 < p[0] for v in X)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("L,K", ((3, 2), (4, 1), (2, 5)))
def test_round_minus_floor_lies_in_0_to_K(L, K, bits):
    """Against bconv_ref.moddown (what nttmul_mdntt_moddown computes): per coefficient the rounded
    result exceeds the floor form's by [frac(phi) >= 1/2] + alpha, in 0 .. K."""
    q, p = ks_ref.bases(bits, L, K)
    rng = np.random.default_rng(L * K + bits)
    x = B.random_words(rng, q + p, 2, N, _dt(bits))
    exact = ref.moddown_coeff(x, q, p).astype(object)
    floor = B.moddown(x, p, q).astype(object)
    y = ref.y_of(x[:, L:], p)
    seen = set()
    for b in range(2):
        for k in range(N):
            phi = ref.phi(y[b, :, k], p)
            alpha = phi.numerator // phi.denominator
            d = alpha + int(phi - alpha >= Fraction(1, 2))
            assert 0 <= d <= K
            seen.add(d)
            for l, m in enumerate(q):
                assert exact[b, l, k] == (floor[b, l, k] + d) % m
    assert len(seen) > 1


@pytest.mark.parametrize("t", (1, 65537))
@pytest.mark.parametrize("bits", (32, 64))
def test_the_plan_constants_are_the_tables_of_the_identities(bits, t):
    """Per limb the result is (x_l - r_l') (t P^-1), r_l' formed with the weights Ph_j t^-1 and one
    more term a (-P t^-1); extend's with Ph_j and a (-P)."""
    L, K = 3, 2
    q, p = ks_ref.bases(bits, L, K)
    P = prod(p)
    yscale, w_ext, w_md, v = ref.plan(q, p, t)
    assert len(w_ext) == len(w_md) == K + 1
    rng = np.random.default_rng(bits + t)
    x = B.random_words(rng, q + p, 1, N, _dt(bits))
    down = ref.moddown_coeff(x, q, p, t)[0].astype(object)
    up = ref.extend_coeff(x[:, L:], q, p, t)[0].astype(object)
    for k in range(N):
        y = [int(x[0, L + j, k]) * yscale[j] % m for j, m in enumerate(p)]
        assert y == [int(u) for u in ref.y_of(x[:, L:], p, t)[0, :, k]]
        phi = ref.phi(y, p)
        a = (phi + Fraction(1, 2)).__floor__()
        assert 0 <= a <= K
        for l, m in enumerate(q):
            r_ext = (sum(yj * w_ext[j][l] for j, yj in enumerate(y)) + a * w_ext[K][l]) % m
            r_md = (sum(yj * w_md[j][l] for j, yj in enumerate(y)) + a * w_md[K][l]) % m
            assert up[l, k] == r_ext
            assert down[l, k] == (int(x[0, l, k]) - r_md) * v[l] % m
    for l, m in enumerate(q):
        assert v[l] == t * pow(P, -1, m) % m and w_ext[K][l] == -P % m


def test_in_band_in_exact_fractions():
    """in_band by fractions.Fraction on constructed coefficients, and the whole-array count held
    to it."""
    for bits, K in ((32, 1), (32, 2), (64, 1), (64, 5)):
        q, p = ks_ref.bases(bits, 1, K)
        P = prod(p)
        eps = K * EPS1
        w = int(eps * P)
        vals = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2, (P - 1) // 2 - w - 1,
                (P + 1) // 2 + w + 1, (P - 1) // 2 - w // 2, (P + 1) // 2 + max(0, w - 1)]
        xp = np.array([[[T % m for T in vals] for m in p]], dtype=object)
        y = ref.y_of(xp, p)
        want = [abs(Fraction(T, P) - Fraction(1, 2)) <= eps for T in vals]
        got = [ref.in_band(y[0, :, k], p, eps) for k in range(len(vals))]
        assert got == want
        assert not any(want[:3]) and not want[5] and not want[6]
        assert want[3] == want[4] == (2 * eps * P >= 1)
        assert ref.count_in_band(xp, p, 1, eps) == sum(want)
        for k in range(len(vals)):
            assert ref.count_in_band(xp[:, :, k:k + 1], p, 1, eps) == int(want[k])


@pytest.mark.parametrize("bits", (32, 64))
def test_the_rounded_chain_is_within_half_of_1_plus_h(bits):
    """The derivation of the chain bound on hoist_ref.chain's mid: the rounded ModDown's error per
    component is at most 1/2, so c_0 + c_1 s - sigma_k(x) sigma_k(s_2) stays strictly below
    (1 + h) / 2; the floor form on the same data (the chain's own out) exceeds that, so the GPU
    chain test can only pass with the rounded form."""
    ch = H.chain(N, bits)
    q, p = ch["q"], ch["p"]
    mid = ch["mid"]
    out = ref.moddown_coeff(mid.reshape(-1, len(q) + len(p), N), q, p).reshape(ch["out"].shape)
    h = hoist_cases.CHAIN_H
    rounded, floored = H.chain_errors(ch, out), H.chain_errors(ch)
    assert 2 * max(rounded) < 1 + h, rounded
    assert 2 * max(floored) >= 1 + h, floored
    assert max(floored) <= H.chain_bound()
    assert ref.count_in_band(mid.reshape(-1, len(q) + len(p), N)[:, len(q):], p, 1,
                             len(p) * EPS1) == 0


def test_no_seeded_gpu_input_has_a_coefficient_inside_the_band():
    """Every seeded input of tests/test_gpu_xconv.py, through the oracle's inverse transform of
    its P part: zero in-band coefficients, so that no GPU assertion is conditional on the data."""
    seen = 0
    for case, x in C.seeded_gpu_inputs():
        q, p = C.moduli_of(case)
        xp = x if case.op == "extend" else x[:, case.L:]
        coef = np.empty_like(xp)
        for b in range(xp.shape[0]):
            for j, m in enumerate(p):
                coef[b, j] = H.inverse_one(xp[b, j].astype(np.uint64), case.n, m)
        assert ref.count_in_band(coef, p, case.t, case.K * EPS1) == 0, case
        seen += 1
    assert seen >= len(C.parity_cases()) + len(C.subbatch_cases()) + 4 + 8 + len(C.bases_cases())
