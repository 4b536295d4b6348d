"""tests/tmd_ref.py held to the statements of include/nttmul_tmd.h, without a GPU, on every basis
of tests/basis_cases.py and on ks_ref.bases, with t = 3, 65537 and the largest odd t below the
class bound: d = X (mod P) and d = 0 (mod t); P out = X (mod t); |X / P - out| <= K + (t + 1) / 2;
out = the floor form - u; the table identities of nttmul_tmd_plan's constants; and the derivation
of the chain bound the GPU test asserts."""
from fractions import Fraction
from math import prod

import numpy as np
import pytest

import basis_cases as BC
import bconv_ref as B
import hoist_cases
import hoist_ref as H
import ks_ref
import mdntt_ref
import tmd_cases as C
import tmd_ref as ref
from xconv_ref import _crt

N = 48
SHAPES = ((1, 1), (3, 2), (2, 5))
BASES = [(prof, BC.bits_of(prof)) for prof in BC.PROFILES] + [("top", 32), ("top", 64)]


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _basis(prof, bits, L, K):
    return ks_ref.bases(bits, L, K) if prof == "top" else BC.basis(prof, L, K)


@pytest.mark.parametrize("which", range(3))
@pytest.mark.parametrize("L,K", SHAPES)
@pytest.mark.parametrize("prof,bits", BASES)
def test_the_definition_on_big_integers(prof, bits, L, K, which):
    q, p = _basis(prof, bits, L, K)
    t = C.plain_moduli(bits)[which]
    Q, P = prod(q), prod(p)
    rng = np.random.default_rng(L + 10 * K + bits + which)
    X = mdntt_ref.big_integers(rng, N, Q * P)
    x = mdntt_ref.residues(X, q + p, _dt(bits))[None]
    Xr, S, u, d = ref.parts(x, q, p, t)
    out = ref.values(x, q, p, t)[0]
    floor = B.moddown(x, p, q)[0].astype(object)
    got = ref.moddown_coeff(x, q, p, t)[0].astype(object)
    half = (t - 1) // 2
    for k, v in enumerate(X):
        assert Xr[0, k] == v
        assert 0 <= S[0, k] - v % P < K * P and (S[0, k] - v) % P == 0     # [X]_P + alpha P
        assert -half <= u[0, k] <= half
        assert (d[0, k] - v) % P == 0 and d[0, k] % t == 0
        assert (P * int(out[k]) - v) % t == 0
        assert abs(Fraction(v, P) - int(out[k])) <= ref.bound(K, t)
        for l, m in enumerate(q):
            assert got[l, k] == int(out[k]) % m == (int(floor[l, k]) - int(u[0, k])) % m
    assert np.array_equal(ref.u_coeff(x, q, p, t)[0].astype(object),
                          np.array([[int(v) % m for v in u[0]] for m in q], dtype=object))


@pytest.mark.parametrize("bits", (32, 64))
def test_the_rescale_keeps_the_message(bits):
    """K = 1: X = m + t e (mod Q p) with m in Z_t comes out as [p^-1 m]_t + t e'."""
    q, p = ks_ref.bases(bits, 3, 1)
    t = 65537
    rng = np.random.default_rng(bits)
    QP = prod(q) * p[0]
    m = [int(v) for v in rng.integers(0, t, size=N)]
    e = [int(v) for v in rng.integers(-(1 << 40), 1 << 40, size=N)]
    X = [(a + t * b) % QP for a, b in zip(m, e)]
    x = mdntt_ref.residues(X, q + p, _dt(bits))[None]
    out = ref.values(x, q, p, t)[0]
    mf = ref.plan(q, p, t)[4]
    for k in range(N):
        # X itself, not its residue: m + t e may be negative, then X = m + t e + Q p and Q p is
        # not 0 modulo t.  The decryption takes the centred residue modulo Q first
        c = (int(out[k]) + prod(q) // 2) % prod(q) - prod(q) // 2
        assert c % t == mf * m[k] % t, k


@pytest.mark.parametrize("t", (3, 65537))
@pytest.mark.parametrize("bits", (32, 64))
def test_the_plan_constants_are_the_tables_of_the_identities(bits, t):
    """Per limb the result is (x_l - r_l) P^-1 with r_l = sum_j y_j w_j + |u| w_K or w_{K + 1}."""
    L, K = 3, 2
    q, p = ks_ref.bases(bits, L, K)
    P = prod(p)
    yscale, g, w, v, mf = ref.plan(q, p, t)
    assert len(w) == K + 2 and mf * P % t == 1
    rng = np.random.default_rng(bits + t)
    x = B.random_words(rng, q + p, 1, N, _dt(bits))
    want = ref.moddown_coeff(x, q, p, t)[0].astype(object)
    for k in range(N):
        y = [int(x[0, L + j, k]) * yscale[j] % m for j, m in enumerate(p)]
        vv = sum(yj * gj for yj, gj in zip(y, g)) % t
        neg = vv > (t - 1) // 2
        mag = t - vv if neg else vv
        assert mag <= (t - 1) // 2
        for l, m in enumerate(q):
            r = (sum(yj * w[j][l] for j, yj in enumerate(y)) + mag * w[K + neg][l]) % m
            assert want[l, k] == (int(x[0, l, k]) - r) * v[l] % m


@pytest.mark.parametrize("t", C.CHAIN_T)
@pytest.mark.parametrize("bits", (32, 64))
def test_the_chain_keeps_the_error_a_multiple_of_t(bits, t):
    """The derivation of the chain test on hoist_ref.chain's mid at n = 256: with zero-noise keys
    mid_0 + mid_1 s = P sigma(x) sigma(s2) exactly, so d_0 + d_1 s is a multiple of P and of t,
    e = -(d_0 + d_1 s) / P is a multiple of t bounded by (K + (t + 1) / 2)(1 + h); the floor
    form's e on the same data is not a multiple of t."""
    ch = H.chain(256, bits)
    q, p = ch["q"], ch["p"]
    L, K = len(q), len(p)
    flat = ch["mid"].reshape(-1, L + K, 256)
    out = ref.moddown_coeff(flat, q, p, t).reshape(ch["out"].shape)
    h = hoist_cases.CHAIN_H
    es = C.chain_error_polys(ch, out)
    assert all(int(v) % t == 0 for e in es for v in e)
    assert max(abs(int(v)) for e in es for v in e) <= ref.bound(K, t) * (1 + h)
    floor = C.chain_error_polys(ch, ch["out"])
    assert any(int(v) % t for e in floor for v in e)
