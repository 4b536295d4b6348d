"""tests/lintrans_ref.py against the references it stands beside, at n = 256 in Python integers:
with one rotation, no weights and no c_0 it is ksntt_ref's mac; the unweighted call is the weighted
call with all-ones weights; it is linear in w_hat; and the chain modup -> apply -> moddown returns
the linear transform of the ciphertext within ModDown's rounding, whatever the number of rotations.
No GPU."""
import numpy as np
import pytest

import bconv_ref as B
import galois_ref
import hoist_cases as HC
import hoist_ref as H
import ks_ref
import ksntt_ref
import lintrans_ref as ref

N = 256
SHAPES = ((4, 2, 2), (3, 1, 1))


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _operands(bits, L, K, terms, comps, ks, batch=2, seed=0):
    q, p = ks_ref.bases(bits, L, K)
    ext, rots = q + p, len(ks)
    rng = np.random.default_rng(1000 * L + 100 * K + 10 * terms + comps + bits + seed)
    a = B.random_words(rng, ext * terms, batch, N, _dt(bits)).reshape(batch, terms, L + K, N)
    b = B.random_words(rng, ext * (terms * comps), rots, N, _dt(bits)).reshape(
        rots, comps, terms, L + K, N)
    w = B.random_words(rng, ext, rots, N, _dt(bits))
    c0 = B.random_words(rng, q, batch, N, _dt(bits))
    a[0, 0, :, 0] = [m - 1 for m in ext]           # the ends of every limb's range
    b[0, 0, 0, :, 0] = [m - 1 for m in ext]
    w[0, :, 0] = [m - 1 for m in ext]
    c0[0, :, 0] = [m - 1 for m in q]
    return q, p, a, b, w, c0


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("L,K,alpha", SHAPES)
def test_one_rotation_unweighted_is_the_key_mac(L, K, alpha, bits):
    terms = -(-L // alpha)
    for k in (1, 5, 2 * N - 1):
        q, p, a, b, _, _ = _operands(bits, L, K, terms, 2, (k,))
        got = ref.apply(a, b, (k,), q, p)
        assert got.dtype == _dt(bits) and got.shape == (2, 2, L + K, N)
        assert np.array_equal(got, ksntt_ref.mac(a, b, (k,), q + p)[:, 0])


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("c0_on", (False, True))
def test_unweighted_is_weighted_by_ones(c0_on, bits):
    ks = (5, 25, 5)
    q, p, a, b, _, c0 = _operands(bits, 3, 2, 2, 2, ks)
    ones = np.ones((len(ks), 5, N), dtype=_dt(bits))
    z = c0 if c0_on else None
    got = ref.apply(a, b, ks, q, p, None, z)
    assert np.array_equal(got, ref.apply(a, b, ks, q, p, ones, z))
    assert all(int(got[..., l, :].max()) < m for l, m in enumerate(q + p))
    # the sum over the rotations of the per-rotation macs, plus P sigma(c0) on component 0 of Q
    want = ksntt_ref.mac(a, b, ks, q + p).astype(object).sum(axis=1)
    if c0_on:
        for r, k in enumerate(ks):
            rot = galois_ref.ntt(c0, k).astype(object)
            for l, m in enumerate(q):
                want[:, 0, l] += rot[:, l] * ref.p_mod(q, p)[l]
    for l, m in enumerate(q + p):
        assert (got[:, :, l].astype(object) == want[:, :, l] % m).all()


@pytest.mark.parametrize("bits", (32, 64))
def test_linear_in_the_weights(bits):
    ks = (1, 5, 2 * N - 1)
    q, p, a, b, w1, c0 = _operands(bits, 3, 1, 3, 1, ks)
    _, _, _, _, w2, _ = _operands(bits, 3, 1, 3, 1, ks, seed=1)
    ext = q + p
    wsum = np.stack([((w1[:, l].astype(object) + w2[:, l].astype(object)) % m).astype(_dt(bits))
                     for l, m in enumerate(ext)], axis=1)
    g1, g2, gs = (ref.apply(a, b, ks, q, p, w, c0) for w in (w1, w2, wsum))
    for l, m in enumerate(ext):
        assert (gs[:, :, l].astype(object) ==
                (g1[:, :, l].astype(object) + g2[:, :, l].astype(object)) % m).all()
    # a weight of zero removes its rotation
    w0 = w1.copy()
    w0[1:] = 0
    assert np.array_equal(ref.apply(a, b, ks, q, p, w0, c0),
                          ref.apply(a[:, :], b[:1], ks[:1], q, p, w0[:1], c0))


@pytest.mark.parametrize("bits", (32, 64))
def test_chain_is_the_linear_transform_within_one_moddown(bits):
    """modup -> apply (weights and c_0) -> moddown on hoist_ref.chain's zero-noise keys.  With
    X_i = c_hat component i as an integer mod QP, X_0 + X_1 s = P T mod QP exactly, T = sum_r w_r
    sigma_{k_r}(c0 + x s2): the key is noiseless and ModUp's overflow u D_d meets the gadget
    P (Q / D_d) t as a multiple of QP.  B.moddown returns (X_i - r_i) / P with r_i = X_i mod P's
    conversion representative in [0, K P), so c0' + c1' s - T = -(r_0 + r_1 s) / P, at most
    K + K h in magnitude: inside hoist_ref.chain_bound() = (K + 1)(1 + h), which therefore holds
    unchanged, and does not grow with the number of rotations or the size of the weights."""
    ch = ref.chain(N, bits)
    assert len(ch["ks"]) == HC.CHAIN_ROTS and ch["mid_lt"].shape[1] == 2
    errs = ref.chain_errors(ch)
    print("lintrans chain errors", bits, errs, "bound", H.chain_bound())
    assert max(errs) <= H.chain_bound()
    assert ch["out_lt"].shape == (ch["x"].shape[0], 2, len(ch["q"]), N)
