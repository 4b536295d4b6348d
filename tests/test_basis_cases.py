"""tests/basis_cases.py held to its own definitions, and the Python-integer references held to
theirs on its bases before any kernel is compared with them (tests/test_gpu_bases.py).  No GPU.

The literals: every one is prime (nttmul.is_prime, the library's host Miller-Rabin), = 1 mod 2^17,
inside its word class, and the prime its anchor defines, recomputed by the walk; Q and P of every
profile are disjoint and of one class.  The references, at n = 256 and L, K <= 4: ks_ref.modup
raises to x_d + u D_d with 0 <= u < |D_d|; ks_ref.worst_case reaches u = |D_d| - 1;
mdntt_ref.moddown equals mdntt_ref.formula, and rescale_floor for K = 1; bconv_ref's sums are the
CRT value plus alpha B with 0 <= alpha < L; the zero-noise key switch of ks_ref.keygen stays inside
the bound its derivation gives (tests/test_gpu_ks.py: (K + 1)(1 + h), whatever the limbs' sizes)."""
from math import prod

import numpy as np
import pytest

import basis_cases as BC
import bconv_ref as B
import ks_ref
import mdntt_ref
import nttmul

N = 256
PROFILES = tuple(BC.PROFILES)
SHAPES = ((4, 2, 2), (3, 2, 2), (4, 4, 1))           # (L, K, alpha), L, K <= 4


def _dt(profile):
    return np.uint32 if BC.bits_of(profile) == 32 else np.uint64


def test_every_literal_is_the_prime_its_anchor_defines():
    for anchor, primes in BC.ANCHORS.items():
        assert len(primes) == BC.PER_ANCHOR
        assert all(nttmul.is_prime(v) for v in primes), anchor
        assert all(v % BC.STEP == 1 for v in primes), anchor
        assert primes == BC.walk(anchor, BC.PER_ANCHOR, nttmul.is_prime), anchor
    used = {a for _, first, qc, pc in BC.PROFILES.values()
            for a in ((first,) if first else ()) + qc + pc}
    assert used == set(BC.ANCHORS)


@pytest.mark.parametrize("profile", PROFILES)
def test_profiles_are_disjoint_and_of_one_class(profile):
    L, K = BC.MAX_SHAPE
    K = min(K, BC.MAX_LIMBS - L)
    q, p = BC.basis(profile, L, K)
    lo, hi = BC.CLASS[BC.bits_of(profile)]
    assert (len(q), len(p)) == (L, K) and len(set(q + p)) == L + K
    assert all(lo <= v < hi for v in q + p)
    assert all(nttmul.is_prime(v) and v % BC.STEP == 1 for v in q + p)
    for l in range(1, L + 1):                        # a smaller shape is a prefix of Q, and of P
        for k in range(1, min(BC.MAX_SHAPE[1], BC.MAX_LIMBS - l) + 1):
            ql, pk = BC.basis(profile, l, k)
            assert ql == q[:l] and len(set(ql + pk)) == l + k
            assert all(lo <= v < hi for v in pk)
            if profile != "bottom64":
                assert pk[:K] == p[:k]
    assert BC.basis("bottom64", 2, 2)[1] == BC.ANCHORS[("up", 32)][2:4]


def test_profiles_are_what_the_table_says():
    A = BC.ANCHORS
    q, p = BC.basis("chain64", 5, 2)
    assert q == (A[("down", 60)][0], A[("up", 40)][0], A[("down", 50)][0], A[("up", 45)][0],
                 A[("up", 33)][0])
    assert p == (A[("down", 62)][0], A[("down", 61)][0]) and min(p) > max(q)
    q, p = BC.basis("chain64_rev", 4, 2)
    assert q == A[("down", 62)][:4] and p == A[("up", 32)][:2] and max(p) < min(q)
    q, p = BC.basis("chain32", 5, 2)
    assert q == (A[("down", 31)][0], A[("up", 25)][0], A[("down", 28)][0], A[("up", 0)][0],
                 A[("up", 25)][1])
    assert p == (A[("down", 31)][1], A[("down", 30)][0])
    q, p = BC.basis("chain32_rev", 4, 2)
    assert q == A[("down", 31)][:4] and p == A[("up", 0)][:2] and max(p) < min(q)
    q, p = BC.basis("bottom64", 4, 2)
    assert q + p == A[("up", 32)][:6] and q[0] - (1 << 32) < 1 << 23
    for profile in ("chain64", "chain32"):           # the order is the table's, not sorted
        q, _ = BC.basis(profile, 4, 2)
        assert list(q) != sorted(q) and list(q) != sorted(q, reverse=True)


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("shape", SHAPES)
def test_modup_raises_to_x_plus_u_D(shape, profile):
    L, K, alpha = shape
    q, p = BC.basis(profile, L, K)
    ext = q + p
    x = B.random_words(np.random.default_rng(L * 100 + K), q, 1, N, _dt(profile))
    x[0, :, 0] = ks_ref.worst_case(q, alpha)
    up = ks_ref.modup(x, q, p, alpha)
    for d, D in enumerate(ks_ref.digits(L, alpha)):
        own = [q[i] for i in D]
        assert np.array_equal(up[:, d, D.start:D.stop, :], x[:, D.start:D.stop, :])
        for k in range(N):
            xd = B.crt([x[0, i, k] for i in D], own)
            raised = B.crt([up[0, d, m, k] for m in range(L + K)], ext)
            u, r = divmod(raised - xd, prod(own))
            assert r == 0 and 0 <= u < len(own), (d, k, u)
            assert k or u == len(own) - 1            # the worst case reaches the largest u


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("L,K", ((1, 1), (4, 2), (2, 4)))
def test_moddown_equals_the_formula_and_the_floor(L, K, profile):
    q, p = BC.basis(profile, L, K)
    x_hat = B.random_words(np.random.default_rng(L * 10 + K), q + p, 1, N, _dt(profile))
    for l, m in enumerate(q + p):
        x_hat[0, l, 0], x_hat[0, l, 1] = 0, m - 1
    got = mdntt_ref.moddown(x_hat, q, p)
    assert np.array_equal(got, mdntt_ref.formula(x_hat, q, p))
    assert all(int(got[:, l].max()) < m for l, m in enumerate(q))
    if K == 1:
        ext = q + p
        X = mdntt_ref.big_integers(np.random.default_rng(L), N, prod(ext))
        x_hat = mdntt_ref.forward(mdntt_ref.residues(X, ext, _dt(profile))[None], ext)
        want = mdntt_ref.rescale_floor(X, q, p[0]).astype(_dt(profile))[None]
        assert np.array_equal(mdntt_ref.moddown(x_hat, q, p), mdntt_ref.forward(want, q))


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("L,K", ((1, 4), (3, 2), (4, 3)))
def test_conversion_sums_are_the_crt_value_plus_alpha_B(L, K, profile):
    to_q, from_q = BC.basis(profile, K, L)           # from P's end of the table into Q's
    x = B.random_words(np.random.default_rng(L + 10 * K), from_q, 1, N, _dt(profile))
    x[0, :, 0] = B.worst_case(from_q)
    s = B.conv_sums(x, from_q)
    got = B.convert(x, from_q, to_q)
    Bp = prod(from_q)
    for k in range(N):
        a, r = divmod(int(s[0, k]) - B.crt(x[0, :, k], from_q), Bp)
        assert r == 0 and 0 <= a < L and (k or a == L - 1)
        assert [int(v) for v in got[0, :, k]] == [int(s[0, k]) % c for c in to_q]
    both = np.concatenate([B.random_words(np.random.default_rng(K), to_q, 1, N, _dt(profile)), x],
                          axis=1)
    down = B.moddown(both, from_q, to_q)
    for k in (0, 1, N - 1):
        assert [int(v) for v in down[0, :, k]] == B.moddown_one(both[0, :, k], from_q, to_q)


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("shape", ((4, 2, 2), (3, 2, 1)))
def test_zero_noise_key_switch_stays_inside_its_bound(shape, profile):
    """Products through the oracle's transforms (hoist_ref), so that n = 256 stays quick."""
    import hoist_ref as H
    L, K, alpha = shape
    h = 8
    q, p = BC.basis(profile, L, K)
    ext, dt = q + p, _dt(profile)
    rng = np.random.default_rng(7 * L + K)
    s, s2 = ks_ref.ternary(rng, N, h), ks_ref.ternary(rng, N, h)
    key = [c.astype(dt) for c in ks_ref.keygen(rng, N, q, p, alpha, s, s2)]
    x = B.random_words(rng, q, 1, N, dt)
    up_hat = H.forward(ks_ref.modup(x, q, p, alpha), ext)          # [1, dnum, L + K, n]
    out = []
    for comp in key:
        mid = H.hoist(up_hat, H.forward(comp, ext)[None, None], (1,), ext)[:, 0, 0]
        out.append(B.moddown(mid, p, q))
    err = ks_ref.key_switch_error(x[0], out[0][0], out[1][0], q, s, s2)
    assert err <= (K + 1) * (1 + h), err
