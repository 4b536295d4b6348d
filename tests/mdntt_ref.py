"""Python-integer reference of include/nttmul_mdntt.h: ModDown on NTT-domain limbs as the
composition it replaces -- the oracle's per-limb inverse transforms (tests/hoist_ref.py, the CPU
loops the library's transforms are held to), bconv_ref.moddown with from = P and to = Q, the
oracle's forward transforms over Q -- and, computed independently of it, the NTT-domain formula of
the header and the exact rescale.  No GPU."""
from math import prod

import numpy as np

import bconv_ref as B
import hoist_ref as H


def inverse(x_hat, moduli):
    """[batch, M, n] bit-reversed transforms -> canonical coefficients, dtype kept."""
    x_hat = np.asarray(x_hat)
    out = np.empty_like(x_hat)
    n = x_hat.shape[-1]
    for p in range(x_hat.shape[0]):
        for l, q in enumerate(moduli):
            out[p, l] = H.inverse_one(x_hat[p, l].astype(np.uint64), n, q)
    return out


forward = H.forward


def moddown(x_hat, q, p):
    """[batch, L + K, n] (limbs of q, then of p, NTT order) -> [batch, L, n] NTT order, dtype
    kept: forward_Q(moddown(inverse_{Q u P}(x_hat)))."""
    x_hat = np.asarray(x_hat)
    assert x_hat.ndim == 3 and x_hat.shape[1] == len(q) + len(p)
    x = inverse(x_hat, tuple(q) + tuple(p))
    return forward(B.moddown(x, p, q), q)


def formula(x_hat, q, p):
    """The header's formula, with nothing taken from bconv_ref: only the K limbs of P are
    transformed back, the conversion sum is formed in Python integers, transformed forward under
    each q_l and subtracted in the NTT domain."""
    x_hat = np.asarray(x_hat)
    L, K, n = len(q), len(p), x_hat.shape[-1]
    P = prod(p)
    out = np.empty((x_hat.shape[0], L, n), dtype=x_hat.dtype)
    for b in range(x_hat.shape[0]):
        s = np.zeros(n, dtype=object)
        for j, pj in enumerate(p):
            Ph = P // pj
            y = H.inverse_one(x_hat[b, L + j].astype(np.uint64), n, pj).astype(object)
            s += (y * pow(Ph, -1, pj) % pj) * Ph
        for l, ql in enumerate(q):
            r = np.array([int(v) % ql for v in s], dtype=x_hat.dtype)
            r_hat = H.forward(r[None, None, :], (ql,))[0, 0].astype(object)
            out[b, l] = ((x_hat[b, l].astype(object) - r_hat) * pow(P, -1, ql) % ql).astype(
                x_hat.dtype)
    return out


def residues(X, moduli, dtype):
    """[len(moduli), n] canonical residues of the n Python integers X."""
    return np.array([[int(v) % m for v in X] for m in moduli], dtype=dtype)


def big_integers(rng, n, bound):
    """n seeded Python integers in [0, bound), the first two at the ends of the range."""
    words = -(-bound.bit_length() // 32) + 1
    X = [int.from_bytes(rng.bytes(4 * words), "little") % bound for _ in range(n)]
    X[0], X[1] = 0, bound - 1
    return X


def rescale_floor(X, q, p):
    """[L, n] object array: floor(X / p) mod q_l per coefficient, coefficient order."""
    return np.array([[(int(v) // p) % ql for v in X] for ql in q], dtype=object)
