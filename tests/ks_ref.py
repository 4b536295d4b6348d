"""Python-integer reference of include/nttmul_ks.h: the digit ModUp formula of the header, the
key generator's gadget factors and the plain constants of nttmul_ks_plan, and the helpers the ks
tests share.  ModDown is bconv_ref.moddown with from = P and to = Q.  No GPU."""
from math import prod

import numpy as np

import bconv_ref as B

STEP = 2 * 65536         # primes with 2 * 65536 | q - 1 serve every n <= 65536
TOP = {32: 1 << 31, 64: 1 << 62}


def bases(bits, L, K):
    """Disjoint Q (L primes) and P (K primes) of the class at the top of its range, for every n:
    the first L primes = 1 mod 2^17 below the class's top, then the next K."""
    p = B.primes_below(TOP[bits], STEP, L + K)
    return tuple(p[:L]), tuple(p[L:])


def digits(L, digit_limbs):
    """The digits D_d as ranges of limbs of Q: dnum = ceil(L / digit_limbs), the last may be
    shorter."""
    assert 1 <= digit_limbs <= L
    return [range(lo, min(lo + digit_limbs, L)) for lo in range(0, L, digit_limbs)]


def modup(x, q, p, digit_limbs):
    """[batch, L, n] -> [batch, dnum, L + K, n], dtype kept: for every digit the integer sum over
    i in D_d of y_i Dh_i (bconv_ref.conv_sums over the digit's limbs), reduced mod every modulus
    of q + p."""
    x = np.asarray(x)
    ext = tuple(q) + tuple(p)
    assert x.ndim == 3 and x.shape[1] == len(q)
    out = []
    for D in digits(len(q), digit_limbs):
        s = B.conv_sums(x[:, D.start:D.stop, :], [q[i] for i in D])
        out.append(np.stack([s % m for m in ext], axis=1))
    return np.stack(out, axis=1).astype(x.dtype)


def gadget(q, p, digit_limbs):
    """[dnum][L + K]: P (Q / D_d) ((Q / D_d)^-1 mod D_d) mod every modulus of q + p, the factor a
    key generator multiplies s' by in digit d."""
    Q, P = prod(q), prod(p)
    out = []
    for D in digits(len(q), digit_limbs):
        Dd = prod(q[i] for i in D)
        Qd = Q // Dd
        g = P * Qd * (pow(Qd, -1, Dd) if Dd > 1 else 0)
        out.append([g % m for m in tuple(q) + tuple(p)])
    return out


def constants(q, p, digit_limbs):
    """(inv, w, gadget, pinv, pw, Pinv) of nttmul_ks_plan: inv[i] = Dh_i^-1 mod q_i,
    w[i][m] = Dh_i mod m-th modulus of q + p, the gadget factors, and bconv_ref.constants(p, q)."""
    ext = tuple(q) + tuple(p)
    inv, w = [0] * len(q), [None] * len(q)
    for D in digits(len(q), digit_limbs):
        Dd = prod(q[i] for i in D)
        for i in D:
            inv[i] = pow(Dd // q[i], -1, q[i])
            w[i] = [(Dd // q[i]) % m for m in ext]
    pinv, pw, Pinv = B.constants(p, q)
    return inv, w, gadget(q, p, digit_limbs), pinv, pw, Pinv


def worst_case(q, digit_limbs):
    """x[i] = -Dh_i mod q_i: every y_i = q_i - 1 and u = |D_d| - 1 in every digit, the
    accumulator's worst case."""
    out = []
    for D in digits(len(q), digit_limbs):
        out += B.worst_case([q[i] for i in D])
    return out


# ---------------------------------------------------------------------------------------------
# The hybrid key switch modup and moddown serve, in Python integers (test_ks_ref.py at n = 16,
# test_gpu_ks.py's chain on the device)
# ---------------------------------------------------------------------------------------------

def negacyclic(a, b, m):
    """a b mod (x^n + 1, m) as an object array: a a sequence of n Python integers (signed, the
    cost is per non-zero coefficient), b array-like of n integers."""
    b = np.asarray(b).astype(object)
    n = len(b)
    assert len(a) == n
    out = np.zeros(n, dtype=object)
    for i, ai in enumerate(a):
        if ai:
            out += int(ai) * np.concatenate((-b[n - i:], b[:n - i]))     # x^i b
    return out % m


def ternary(rng, n, h):
    """A ternary polynomial of Hamming weight h, as a list of signed integers."""
    s = [0] * n
    for i in rng.choice(n, size=h, replace=False):
        s[int(i)] = int(rng.choice((-1, 1)))
    return s


def keygen(rng, n, q, p, digit_limbs, s, s2):
    """The zero-noise key that switches s2 to s, over q + p: per digit d and limb m, a_d uniform
    and b_d = -a_d s + gadget_d s2.  Returns the components (b, a), each an object array
    [dnum, L + K, n] of canonical residues."""
    ext = tuple(q) + tuple(p)
    g = gadget(q, p, digit_limbs)
    a = np.empty((len(g), len(ext), n), dtype=object)
    b = np.empty_like(a)
    for d, gd in enumerate(g):
        for l, m in enumerate(ext):
            a[d, l] = [int(v) for v in rng.integers(0, m, size=n, dtype=np.uint64)]
            b[d, l] = (gd[l] * np.array(s2, dtype=object) - negacyclic(s, a[d, l], m)) % m
    return b, a


def key_switch_error(x, c0, c1, q, s, s2):
    """The largest |coefficient| of c0 + c1 s - x s2 mod q_i, centered, over the limbs of Q;
    x, c0, c1: [L, n]."""
    worst = 0
    for i, m in enumerate(q):
        e = np.asarray(c0[i]).astype(object) + negacyclic(s, c1[i], m) - negacyclic(s2, x[i], m)
        e %= m
        worst = max(worst, max(int(min(v, m - v)) for v in e))
    return worst
