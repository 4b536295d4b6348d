"""tests/ctlin_ref.py without a GPU, on the mixed-size bases of tests/basis_cases.py: the array
references against the word-by-word definitions of include/nttmul_ctlin.h, tensor's d_2, d_0 and
d_1 against tests/ctmul_ref.py's high, e_0 and e_1, and the two identities the GPU chains rest on,
with schoolbook negacyclic products mod Q in Python integers at n = 256."""
import numpy as np
import pytest

import bconv_ref as B
import ctlin_cases as C
import ctlin_ref as ref
import ctmul_ref

SMALL_N = 8                                  # the definitions walk word by word


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _terms(rng, q, shape, spec, dt):
    """Seeded operands of a term spec of tests/ctlin_cases.py: [(x, w, kind), ..]."""
    batch, comps, L, n = shape
    count = 1 + max([i for _, i in spec if i is not None], default=-1)
    xs = [B.random_words(rng, q * comps, batch, n, dt).reshape(shape) for _ in range(count)]
    out = []
    for kind, i in spec:
        w = None
        if kind == C.SCALAR:
            w = np.array([int(rng.integers(0, m, dtype=np.uint64)) for m in q], dtype=dt)
        elif kind == C.PLAIN:
            w = B.random_words(rng, q, 1, n, dt)[0]
        out.append((None if i is None else xs[i], w, C.KIND_CODE[kind]))
    return out


@pytest.mark.parametrize("bits", (32, 64))
def test_the_bases_are_mixed_and_unsorted(bits):
    q = C.moduli_of(bits)
    lo, hi = (2, 1 << 31) if bits == 32 else (1 << 32, 1 << 62)
    assert len(q) == C.L == 3 and all(lo <= m < hi for m in q)
    assert list(q) != sorted(q) and list(q) != sorted(q, reverse=True)
    assert max(q).bit_length() - min(q).bit_length() >= 5
    assert not set(C.special_of(bits)) & set(q)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("row", range(len(C.ROWS)))
def test_combine_equals_the_definition(row, bits):
    q, dt = C.moduli_of(bits), _dt(bits)
    _, comps, spec = C.ROWS[row]
    shape = (2, comps, C.L, SMALL_N)
    terms = _terms(np.random.default_rng(row + bits), q, shape, spec, dt)
    got = ref.combine(terms, q, shape, dt)
    assert got.dtype == dt
    assert (got.astype(object) == ref.definition_combine(terms, q, shape)).all()
    for l, m in enumerate(q):
        assert (got[:, :, l].astype(object) < m).all()


@pytest.mark.parametrize("bits", (32, 64))
def test_combine_at_the_top_of_the_range(bits):
    """Every word q_l - 1: 16 PLAIN terms sum to 16, 16 ONE terms to -16, a scalar q_l - 1 negates."""
    q, dt = C.moduli_of(bits), _dt(bits)
    shape = (1, 3, C.L, SMALL_N)
    top = np.broadcast_to(np.array([m - 1 for m in q], dtype=dt)[:, None], shape).copy()
    for kind, want in ((ref.PLAIN, 16), (ref.ONE, -16)):
        terms = [(top, top[0, 0] if kind == ref.PLAIN else None, kind)] * 16
        got = ref.combine(terms, q, shape, dt)
        assert (got.astype(object) == ref.definition_combine(terms, q, shape)).all()
        for l, m in enumerate(q):
            assert (got[:, :, l] == want % m).all()
    neg = ref.combine([(top, top[0, 0, :, 0], ref.SCALAR)], q, shape, dt)
    assert (neg == 1).all()


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("pairs,square", ((1, False), (3, False), (2, True)))
def test_tensor_equals_the_definition_and_ctmul_ref(pairs, square, bits):
    q, dt = C.moduli_of(bits), _dt(bits)
    rng = np.random.default_rng(pairs + bits)
    shape = (2, pairs, 2, C.L, SMALL_N)
    x = B.random_words(rng, q * (2 * pairs), 2, SMALL_N, dt).reshape(shape)
    y = x if square else B.random_words(rng, q * (2 * pairs), 2, SMALL_N, dt).reshape(shape)
    got = ref.tensor(x, y, q)
    assert got.dtype == dt and got.shape == (2, 3, C.L, SMALL_N)
    assert (got.astype(object) == ref.definition_tensor(x, y, q)).all()
    e0, e1, d2 = ctmul_ref.tensor(x, y, q)
    assert np.array_equal(got[:, 2], ctmul_ref.high(x, y, q)) and np.array_equal(got[:, 2], d2)
    assert np.array_equal(got[:, 0], e0) and np.array_equal(got[:, 1], e1)


@pytest.mark.parametrize("bits", (32, 64))
def test_the_identities_of_the_chains(bits):
    """For c_0 = m - c_1 s: pt c_0 + (pt c_1) s = pt m, and for two such ciphertexts
    d_0 + d_1 s + d_2 s^2 = m_1 m_2, both exactly mod Q."""
    q = C.moduli_of(bits)
    ch = ref.chain_setup(bits, q, 2, 5 + bits)
    Q, s, n = ch["Q"], ch["s"], ref.CHAIN_N
    assert n == C.CHAIN_N == 256 and len(s) == n and sum(map(abs, s)) == ref.CHAIN_H
    cts = [[ref.lift(ch["cts"][i, c], q) for c in (0, 1)] for i in (0, 1)]
    for (c0, c1), m in zip(cts, ch["msgs"]):                        # zero noise
        assert ref.decrypt([c0, c1], s, Q) == m
    rng = np.random.default_rng(bits)
    pt = [ref.uniform(rng, Q) for _ in range(n)]
    (a0, a1), (b0, b1) = cts
    m1, m2 = ch["msgs"]
    assert ref.decrypt([ref.negacyclic(pt, a0, Q), ref.negacyclic(pt, a1, Q)], s, Q) == \
        ref.negacyclic(pt, m1, Q)
    d0 = ref.negacyclic(a0, b0, Q)
    d1 = [(u + v) % Q for u, v in zip(ref.negacyclic(a0, b1, Q), ref.negacyclic(a1, b0, Q))]
    d2 = ref.negacyclic(a1, b1, Q)
    assert ref.decrypt([d0, d1, d2], s, Q) == ref.negacyclic(m1, m2, Q)


def test_the_composition_needs_no_library_at_import():
    import inspect
    src = inspect.getsource(ref)
    assert "import nttmul" not in src and "import torch" not in src
