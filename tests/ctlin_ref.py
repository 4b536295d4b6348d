"""Python-integer reference of include/nttmul_ctlin.h, from the header's formulas.  definition_* are
the definitions word by word in plain Python integers; combine and tensor are the same sums on
whole arrays (numpy uint64 on 32-bit words, object arrays on 64-bit words), which
tests/test_ctlin_ref.py holds to the definitions.  And the zero-noise ciphertexts of the chain
tests.  No GPU, but for composition(), which runs the calls of the contexts it is handed.

A term is (x, w, kind) as nttmul.ctlin_one / ctlin_scalar / ctlin_plain / ctlin_const_scalar /
ctlin_const_plain make it: x [batch, comps, L, n] or None, w None, [L] or [L, n]."""
from math import prod

import numpy as np

import bconv_ref as B
import ks_ref
from ctmul_ref import _m, _wide, limb_products

ONE, SCALAR, PLAIN = 0, 1, 2


def _scalar(v, m):
    """v as the scalar that keeps the arrays of limb m in their type."""
    return np.uint64(int(v)) if m < (1 << 32) else int(v)


def definition_combine(terms, q, shape):
    """out[p][c][l][j] = (sum_i W_i[l][j] X_i[p][c][l][j]) mod q_l, one word at a time."""
    batch, comps, L, n = shape
    assert L == len(q)
    out = np.empty(shape, dtype=object)
    for p in range(batch):
        for c in range(comps):
            for l in range(L):
                for j in range(n):
                    acc = 0
                    for x, w, kind in terms:
                        X = int(x[p][c][l][j]) if x is not None else int(c == 0)
                        W = 1 if kind == ONE else int(w[l]) if kind == SCALAR else int(w[l][j])
                        acc += W * X
                    out[p, c, l, j] = acc % q[l]
    return out


def definition_tensor(x_hat, y_hat, q):
    """d_0 = sum_s x[s][0] y[s][0], d_1 = sum_s (x[s][0] y[s][1] + x[s][1] y[s][0]),
    d_2 = sum_s x[s][1] y[s][1], one word at a time: [batch, 3, L, n]."""
    batch, pairs, _, L, n = np.shape(x_hat)
    out = np.empty((batch, 3, L, n), dtype=object)
    for p in range(batch):
        for l in range(L):
            for j in range(n):
                x = [[int(x_hat[p][s][i][l][j]) for i in (0, 1)] for s in range(pairs)]
                y = [[int(y_hat[p][s][i][l][j]) for i in (0, 1)] for s in range(pairs)]
                out[p, 0, l, j] = sum(a[0] * b[0] for a, b in zip(x, y)) % q[l]
                out[p, 1, l, j] = sum(a[0] * b[1] + a[1] * b[0] for a, b in zip(x, y)) % q[l]
                out[p, 2, l, j] = sum(a[1] * b[1] for a, b in zip(x, y)) % q[l]
    return out


def combine(terms, q, shape, dtype):
    """The definition on whole arrays; returns [batch, comps, L, n] of `dtype`."""
    batch, comps, L, n = shape
    assert L == len(q)
    out = np.empty(shape, dtype=dtype)
    for l, m in enumerate(q):
        acc = _wide(np.zeros((batch, comps, n), dtype=np.uint64), m)
        for x, w, kind in terms:
            if x is None:                                           # X = [c = 0]
                X = _wide(np.zeros((batch, comps, n), dtype=np.uint64), m)
                X[:, 0] += _wide(np.ones(n, dtype=np.uint64), m)
            else:
                X = _wide(np.asarray(x)[:, :, l], m)
            if kind == ONE:
                assert w is None and x is not None
                W = _scalar(1, m)
            elif kind == SCALAR:
                W = _scalar(w[l], m)
            else:
                assert kind == PLAIN
                W = _wide(np.asarray(w)[l], m)
            acc = (acc + X * W % _m(m)) % _m(m)
        out[:, :, l] = acc
    return out


def tensor(x_hat, y_hat, q):
    """[batch, pairs, 2, L, n] twice -> [batch, 3, L, n] in x_hat's dtype."""
    x_hat, y_hat = np.asarray(x_hat), np.asarray(y_hat)
    batch, pairs, two, L, n = x_hat.shape
    assert two == 2 and L == len(q) and y_hat.shape == x_hat.shape
    out = np.empty((batch, 3, L, n), dtype=x_hat.dtype)
    for l, m in enumerate(q):
        d = [_wide(np.zeros((batch, n), dtype=np.uint64), m) for _ in range(3)]
        for s in range(pairs):
            x0, x1 = _wide(x_hat[:, s, 0, l], m), _wide(x_hat[:, s, 1, l], m)
            y0, y1 = _wide(y_hat[:, s, 0, l], m), _wide(y_hat[:, s, 1, l], m)
            d[0] = (d[0] + x0 * y0 % _m(m)) % _m(m)
            d[1] = (d[1] + x0 * y1 % _m(m) + x1 * y0 % _m(m)) % _m(m)
            d[2] = (d[2] + x1 * y1 % _m(m)) % _m(m)
        for i in range(3):
            out[:, i, l] = d[i]
    return out


# ---------------------------------------------------------------------------------------------
# The composition a caller runs without the library (the reference where Python integers do not
# reach): one plain context per limb for the products, host modular additions
# ---------------------------------------------------------------------------------------------

def _add_mod(a, b, q):
    """a + b per limb mod q_l for canonical [.., L, n] arrays, dtype kept."""
    out = np.empty_like(a)
    for l, m in enumerate(q):
        out[..., l, :] = (_wide(a[..., l, :], m) + _wide(b[..., l, :], m)) % _m(m)
    return out


def composition(plain, terms, q, shape, dtype):
    """combine from per-limb pointwise products (plain: one nttmul.Context per limb) and host
    additions: a SCALAR is a product with the constant in every slot."""
    batch, comps, L, n = shape
    acc = np.zeros(shape, dtype=dtype)
    for x, w, kind in terms:
        if kind == SCALAR:
            w = np.repeat(np.asarray(w, dtype=dtype)[:, None], n, axis=1)
        if x is None:
            t = np.zeros(shape, dtype=dtype)
            t[:, 0] = np.asarray(w, dtype=dtype)
        elif kind == ONE:
            t = np.asarray(x)
        else:
            t = limb_products(plain, np.asarray(x),
                              np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=dtype),
                                                                   shape)))
        acc = _add_mod(acc, t, q)
    return acc


def tensor_composition(plain, x_hat, y_hat, q):
    """tensor from ctmul_ref.tensor_composition's products and additions: [batch, 3, L, n]."""
    from ctmul_ref import tensor_composition as parts
    return np.stack(parts(plain, x_hat, y_hat, q), axis=1)


# ---------------------------------------------------------------------------------------------
# Zero-noise ciphertexts over Q, in coefficient order, for the chains
# ---------------------------------------------------------------------------------------------

CHAIN_N = 256
CHAIN_H = 16                                 # the secret's Hamming weight


def residues(poly, q, dtype):
    """A polynomial of integers mod Q -> its limbs [L, n]."""
    return np.array([[int(v) % m for v in poly] for m in q], dtype=dtype)


def lift(limbs, q):
    """[L, n] canonical residues -> the n integers in [0, Q)."""
    limbs = np.asarray(limbs)
    return [B.crt(limbs[:, j], q) for j in range(limbs.shape[1])]


def negacyclic(a, b, Q):
    """a b mod (x^n + 1, Q), schoolbook in Python integers: a list."""
    return [int(v) for v in ks_ref.negacyclic([int(v) for v in a], np.array(b, dtype=object), Q)]


def uniform(rng, Q):
    """A seeded integer in [0, Q) (Q < 2^192: the bias is below 2^-64)."""
    assert Q < 1 << 192
    return int.from_bytes(rng.bytes(32), "little") % Q


def encrypt(rng, msg, s, Q):
    """(c_0, c_1) with c_1 uniform and c_0 = msg - c_1 s mod Q exactly: no noise."""
    n = len(msg)
    c1 = [uniform(rng, Q) for _ in range(n)]
    c1s = negacyclic(s, c1, Q)
    return [(int(v) - u) % Q for v, u in zip(msg, c1s)], c1


def decrypt(comps, s, Q):
    """c_0 + c_1 s + c_2 s^2 .. mod Q for the components given, lists of integers."""
    acc, power = [0] * len(s), None
    for c in comps:
        term = c if power is None else negacyclic(power, c, Q)
        acc = [(a + int(t)) % Q for a, t in zip(acc, term)]
        power = list(s) if power is None else negacyclic(s, power, Q)
    return acc


def chain_setup(bits, q, count, seed):
    """Q, a ternary secret, `count` random messages mod Q and their zero-noise ciphertexts as
    coefficient-order limbs [count, 2, L, n]."""
    Q = prod(q)
    dt = np.uint32 if bits == 32 else np.uint64
    rng = np.random.default_rng(seed)
    s = ks_ref.ternary(rng, CHAIN_N, CHAIN_H)
    msgs = [[uniform(rng, Q) for _ in range(CHAIN_N)] for _ in range(count)]
    cts = np.stack([np.stack([residues(c, q, dt) for c in encrypt(rng, m, s, Q)]) for m in msgs])
    return dict(Q=Q, s=s, msgs=msgs, cts=cts, dtype=dt)
