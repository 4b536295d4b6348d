"""Python-integer reference of include/nttmul_tmd.h, straight from the definition: the CRT value X
of the residues, the uncorrected sum S, v = -S P^-1 mod t, its centred representative u,
d = S + u P and (X - d) / P.  Coefficient-order functions work on canonical residues; the
NTT-order one wraps them in the oracle's transforms (tests/hoist_ref.py).  No GPU."""
from math import prod

import numpy as np

import hoist_ref as H
from xconv_ref import _crt, _inverse

T_BOUND = {32: 1 << 31, 64: 1 << 62}          # csrc/tmd_plan.hpp tmd_t_bound


def t_max(bits):
    """The largest odd t below the class bound."""
    return T_BOUND[bits] - 1


def y_of(xp, p):
    """y_j = [x]_{p_j} Ph_j^-1 mod p_j for the residues xp [.., K, n] over p: object array."""
    xp = np.asarray(xp).astype(object)
    P = prod(p)
    out = np.empty_like(xp)
    for j, m in enumerate(p):
        out[..., j, :] = xp[..., j, :] * pow(P // m, -1, m) % m
    return out


def parts(x, q, p, t):
    """Of [batch, L + K, n] residues over q + p: object arrays [batch, n] X (the CRT value over
    Q u P), S (the uncorrected sum), u (the centred correction) and d = S + u P."""
    x = np.asarray(x)
    L, P = len(q), prod(p)
    X = _crt(x, tuple(q) + tuple(p))
    y = y_of(x[:, L:], p)
    S = sum(y[:, j, :] * (P // m) for j, m in enumerate(p))
    u = u_of(x[:, L:], p, t)
    return X, S, u, S + u * P


def u_of(xp, p, t):
    """[.., n] object array: the centred u of the residues xp [.., K, n] over p."""
    y = y_of(xp, p)
    v = sum(y[..., j, :] * (-pow(m, -1, t) % t) for j, m in enumerate(p)) % t
    return v - t * np.asarray(v > (t - 1) // 2).astype(int).astype(object)


def values(x, q, p, t):
    """[batch, n] object array of the signed integers (X - d) / P."""
    X, _, _, d = parts(x, q, p, t)
    P = prod(p)
    assert not np.any((X - d) % P)
    return (X - d) // P


def moddown_coeff(x, q, p, t):
    """[batch, L + K, n] residues over q + p -> [batch, L, n]: (X - d) / P mod q_l.  dtype kept."""
    x = np.asarray(x)
    r = values(x, q, p, t)
    return np.stack([r % m for m in q], axis=1).astype(x.dtype)


def u_coeff(x, q, p, t):
    """[batch, L, n]: u mod q_l, dtype kept."""
    x = np.asarray(x)
    u = parts(x, q, p, t)[2]
    return np.stack([u % m for m in q], axis=1).astype(x.dtype)


def moddown(x_hat, q, p, t):
    """NTT order in, NTT order out: forward_Q(moddown_coeff(inverse_{Q u P}(x_hat)))."""
    return H.forward(moddown_coeff(_inverse(x_hat, tuple(q) + tuple(p)), q, p, t), q)


def plan(q, p, t):
    """(yscale, g, w, v, msg_factor) of nttmul_tmd_plan in Python integers."""
    P = prod(p)
    yscale = [pow(P // m, -1, m) for m in p]
    g = [-pow(m, -1, t) % t for m in p]
    w = [[(P // m) % c for c in q] for m in p] + [[P % c for c in q], [-P % c for c in q]]
    v = [pow(P, -1, c) for c in q]
    return yscale, g, w, v, pow(P, -1, t)


def bound(K, t):
    """|X / P - out| <= K + (t + 1) / 2."""
    return K + (t + 1) // 2
