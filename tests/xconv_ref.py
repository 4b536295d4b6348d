"""Python-integer reference of include/nttmul_xconv.h, straight from the definitions: the CRT
value of the residues, its centred representative modulo P, and round(t X / P) as
(2 t X + P) // (2 P).  Coefficient-order functions work on canonical residues; the NTT-order ones
wrap them in the oracle's transforms (tests/hoist_ref.py).  in_band decides the header's guard band
in exact fractions.  No GPU."""
from fractions import Fraction
from math import prod

import numpy as np

import hoist_ref as H


def _crt(x, moduli):
    """[batch, len(moduli), n] residues -> object array [batch, n] of the values in [0, M)."""
    x = np.asarray(x).astype(object)
    M = prod(moduli)
    return sum(x[:, i, :] * (pow(M // m, -1, m) * (M // m)) for i, m in enumerate(moduli)) % M


def centred(v, P):
    """The representative of v mod P in [-(P - 1) / 2, (P - 1) / 2] (P odd), elementwise."""
    r = v % P
    return r - P * np.asarray(r > P // 2).astype(int).astype(object)


def extend_coeff(x, q, p, t=1):
    """[batch, K, n] residues over p -> [batch, L, n] over q: the centred representative of
    t * CRT(x) mod P, reduced modulo each q_l.  dtype kept."""
    x = np.asarray(x)
    c = centred(_crt(x, p) * t, prod(p))
    return np.stack([c % m for m in q], axis=1).astype(x.dtype)


def moddown_coeff(x, q, p, t=1):
    """[batch, L + K, n] residues over q + p -> [batch, L, n]: round(t X / P) mod q_l for the CRT
    value X over Q u P.  dtype kept."""
    x = np.asarray(x)
    P = prod(p)
    X = _crt(x, tuple(q) + tuple(p))
    r = (2 * t * X + P) // (2 * P)
    return np.stack([r % m for m in q], axis=1).astype(x.dtype)


def moddown_values(X, q, p, t=1):
    """[L, n] object array: round(t X / P) mod q_l for the n Python integers X."""
    P = prod(p)
    return np.array([[((2 * t * int(v) + P) // (2 * P)) % m for v in X] for m in q], dtype=object)


def _inverse(x_hat, moduli):
    x_hat = np.asarray(x_hat)
    out = np.empty_like(x_hat)
    for b in range(x_hat.shape[0]):
        for l, m in enumerate(moduli):
            out[b, l] = H.inverse_one(x_hat[b, l].astype(np.uint64), x_hat.shape[-1], m)
    return out


def extend(p_hat, q, p, t=1):
    """NTT order in, NTT order out: forward_Q(extend_coeff(inverse_P(p_hat)))."""
    return H.forward(extend_coeff(_inverse(p_hat, p), q, p, t), q)


def moddown(x_hat, q, p, t=1):
    """NTT order in, NTT order out: forward_Q(moddown_coeff(inverse_{Q u P}(x_hat)))."""
    return H.forward(moddown_coeff(_inverse(x_hat, tuple(q) + tuple(p)), q, p, t), q)


def y_of(xp, p, t=1):
    """y_j = [t x]_{p_j} Ph_j^-1 mod p_j for the residues xp [.., K, n] over p: object array."""
    xp = np.asarray(xp).astype(object)
    P = prod(p)
    out = np.empty_like(xp)
    for j, m in enumerate(p):
        out[..., j, :] = xp[..., j, :] * (t * pow(P // m, -1, m) % m) % m
    return out


def phi(y, p):
    """The exact phi = sum_j y_j / p_j of one coefficient's y."""
    return sum(Fraction(int(v), m) for v, m in zip(y, p))


def in_band(y, p, eps):
    """|frac(phi) - 1/2| <= eps for one coefficient's y (a sequence of K integers)."""
    f = phi(y, p)
    return abs(f - (f.numerator // f.denominator) - Fraction(1, 2)) <= eps


def count_in_band(xp, p, t, eps):
    """The coefficients of the residues xp [.., K, n] over p (coefficient order) whose phi lies
    inside the band, in whole-array integer arithmetic: frac(phi) = (S mod P) / P with
    S = sum_j y_j Ph_j, so the coefficient is inside iff |2 (S mod P) - P| <= 2 eps P.
    tests/test_xconv_ref.py holds it to in_band."""
    y = y_of(xp, p, t)
    P = prod(p)
    S = sum(y[..., j, :] * (P // m) for j, m in enumerate(p)) % P
    eps = Fraction(eps)
    d = abs(2 * S - P) * eps.denominator
    return int(np.count_nonzero(np.asarray(d <= 2 * eps.numerator * P).astype(bool)))


def plan(q, p, t=1):
    """(yscale, w_ext, w_md, v) of nttmul_xconv_plan in Python integers."""
    P, K = prod(p), len(p)
    yscale = [t * pow(P // m, -1, m) % m for m in p]
    w_ext = [[(P // m) % c for c in q] for m in p] + [[-P % c for c in q]]
    w_md = [[w_ext[j][l] * pow(t, -1, c) % c for l, c in enumerate(q)] for j in range(K + 1)]
    v = [t * pow(P, -1, c) % c for c in q]
    return yscale, w_ext, w_md, v
