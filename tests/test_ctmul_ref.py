"""tests/ctmul_ref.py against the references it stands beside, at n = 256 in Python integers: the
inverse of high(forward(a), forward(b)) is the negacyclic product per limb; relin without tensor
terms is ksntt_ref's mac and lintrans_ref's apply with P c_0; it is symmetric in x and y and
additive over the pairs; and the chain high -> modup -> relin -> moddown decrypts to the product
within one ModDown's rounding, whatever `pairs` is.  No GPU."""
import numpy as np
import pytest

import bconv_ref as B
import ctmul_ref as ref
import hoist_cases as HC
import hoist_ref as H
import ks_ref
import ksntt_ref
import lintrans_ref

N = 256


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _pairs(bits, L, K, pairs, batch=2, seed=0):
    q, p = ks_ref.bases(bits, L, K)
    rng = np.random.default_rng(100 * L + 10 * K + pairs + bits + seed)
    x = B.random_words(rng, q * (2 * pairs), batch, N, _dt(bits)).reshape(batch, pairs, 2, L, N)
    y = B.random_words(rng, q * (2 * pairs), batch, N, _dt(bits)).reshape(batch, pairs, 2, L, N)
    x[0, 0, :, :, 0] = y[0, 0, :, :, 0] = [m - 1 for m in q]      # the ends of every limb's range
    return q, p, x, y


def _key_operands(bits, q, p, terms, batch=2, seed=0):
    ext = q + p
    rng = np.random.default_rng(7 * terms + bits + seed)
    up = B.random_words(rng, ext * terms, batch, N, _dt(bits)).reshape(batch, terms, len(ext), N)
    key = B.random_words(rng, ext * terms, 2, N, _dt(bits)).reshape(2, terms, len(ext), N)
    up[0, 0, :, 0] = key[0, 0, :, 0] = [m - 1 for m in ext]
    return up, key


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("pairs", (1, 3))
def test_high_is_the_negacyclic_product_per_limb(pairs, bits):
    """inverse(high(forward(a), forward(b))) = sum_s a_s[1] b_s[1] mod (x^n + 1, q_l), with sparse
    a so that ks_ref.negacyclic stays cheap."""
    q, p, x, y = _pairs(bits, 3, 1, pairs, batch=1)
    a = np.zeros_like(x)
    rng = np.random.default_rng(bits + pairs)
    for s in range(pairs):
        for i in range(2):
            for l, m in enumerate(q):
                for j in rng.choice(N, size=4, replace=False):
                    a[0, s, i, l, int(j)] = int(rng.integers(1, m))
    a[0, 0, 1, :, N - 1] = [m - 1 for m in q]
    d2 = ref.coefficients(ref.high(H.forward(a, q), H.forward(y, q), q), q)
    assert d2.dtype == _dt(bits) and d2.shape == (1, 3, N)
    for l, m in enumerate(q):
        want = sum(ks_ref.negacyclic([int(v) for v in a[0, s, 1, l]], y[0, s, 1, l], m)
                   for s in range(pairs)) % m
        assert (d2[0, l].astype(object) == want).all()


@pytest.mark.parametrize("bits", (32, 64))
def test_relin_is_the_key_mac_plus_p_times_the_tensor_terms(bits):
    q, p, x, y = _pairs(bits, 3, 2, 2)
    up, key = _key_operands(bits, q, p, 2)
    ext = q + p
    got = ref.relin(up, key, x, y, q, p)
    assert got.dtype == _dt(bits) and got.shape == (2, 2, 5, N)
    assert all(int(got[..., l, :].max()) < m for l, m in enumerate(ext))
    mac = ksntt_ref.mac(up, key[None], (1,), ext)[:, 0]
    assert np.array_equal(got[:, :, 3:], mac[:, :, 3:])              # the limbs of P: no tensor term
    e0, e1, d2 = ref.tensor(x, y, q)
    pq = ref.p_mod(q, p)
    for l, m in enumerate(q):
        for i, e in enumerate((e0, e1)):
            want = (mac[:, i, l].astype(object) + pq[l] * e[:, l].astype(object)) % m
            assert (got[:, i, l].astype(object) == want).all()
    # component 0 is lintrans_ref's apply with c0_hat = e_0, k = {1}, no weights
    lt = lintrans_ref.apply(up, key[None], (1,), q, p, None, e0)
    assert np.array_equal(lt[:, 0], got[:, 0])
    assert np.array_equal(ref.high(x, y, q), d2)


@pytest.mark.parametrize("bits", (32, 64))
def test_symmetric_in_its_pairs_and_additive_over_them(bits):
    q, p, x, y = _pairs(bits, 2, 1, 2)
    up, key = _key_operands(bits, q, p, 1)
    both = ref.relin(up, key, x, y, q, p)
    assert np.array_equal(both, ref.relin(up, key, y, x, q, p))
    assert np.array_equal(ref.high(x, y, q), ref.high(y, x, q))
    zero = np.zeros_like(key)
    parts = [ref.relin(up, zero, x[:, s:s + 1], y[:, s:s + 1], q, p) for s in range(2)]
    whole = ref.relin(up, zero, x, y, q, p)
    assert not whole[:, :, 2:].any()
    for l, m in enumerate(q):
        assert (whole[:, :, l].astype(object) ==
                (parts[0][:, :, l].astype(object) + parts[1][:, :, l].astype(object)) % m).all()
    # the square
    sq = ref.relin(up, key, x, x, q, p)
    e0, e1, _ = ref.tensor(x, x, q)
    for l, m in enumerate(q):
        twice = 2 * sum(x[:, s, 0, l].astype(object) * x[:, s, 1, l].astype(object)
                        for s in range(2)) % m
        assert (e1[:, l].astype(object) == twice).all()
    mac = ksntt_ref.mac(up, key[None], (1,), q + p)[:, 0]
    assert np.array_equal(sq, ref.add_scaled(mac, e0, e1, q, p))


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("pairs", (1, 3))
def test_the_reference_chain_decrypts(pairs, bits):
    """high -> modup -> relin -> moddown on a zero-noise key for s s -> s.  With Y_i = c_hat
    component i as an integer mod QP, Y_0 + Y_1 s = P (d0 + d1 s + d2 s s) mod QP exactly: the key
    is noiseless and ModUp's overflow u D_d meets the gadget P (Q / D_d) as a multiple of QP.
    B.moddown returns (Y_i - r_i) / P with 0 <= r_i < (K + 1) P, so the error is at most
    (K + 1)(1 + h) in magnitude: one key switch's rounding, whatever `pairs` is."""
    ch = ref.chain(N, bits, pairs)
    L, K, alpha = HC.CHAIN_SHAPE
    assert ch["mid"].shape == (HC.CHAIN_BATCH, 2, L + K, N) and ch["x"].shape[1] == pairs
    assert ch["up_hat"].shape == (HC.CHAIN_BATCH, -(-L // alpha), L + K, N)
    assert sum(1 for v in ch["s"] if v) == HC.CHAIN_H
    # s s as signed integers is the negacyclic square
    m = ch["q"][0]
    assert (ks_ref.negacyclic(ch["s"], [v % m for v in ch["s"]], m) ==
            np.array([v % m for v in ch["ss"]], dtype=object)).all()
    # the d_i are the negacyclic products of the coefficient-order inputs (limb 0, entry 0)
    x, y = ch["x"][0, :, :, 0], ch["y"][0, :, :, 0]
    want = sum(ks_ref.negacyclic([int(v) for v in x[s, 1]], y[s, 1], m) for s in range(pairs)) % m
    assert (ch["d"][2][0, 0].astype(object) == want).all()
    errs = ref.chain_errors(ch, ch["out"], ch["d"])
    print("ctmul chain errors", bits, pairs, errs, "bound", ref.chain_bound())
    assert max(errs) <= ref.chain_bound() == (K + 1) * (1 + HC.CHAIN_H)
