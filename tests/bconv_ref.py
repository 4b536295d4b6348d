"""Python-integer reference of include/nttmul_bconv.h: the two formulas of the header, the plain
constants of nttmul_bconv_plan, and the helpers the bconv tests share.  No GPU; nttmul.is_prime is
the library's host Miller-Rabin."""
from math import prod

import numpy as np

import nttmul

STEP = 2 * 4096          # primes with 2 * 4096 | q - 1 serve every n <= 4096


def primes_below(top, step, count):
    """The first `count` primes q = 1 mod step below top, walking down in steps of `step`."""
    assert step % STEP == 0
    q, out = (top - 2) // step * step + 1, []
    while len(out) < count:
        assert q > 2
        if nttmul.is_prime(q):
            out.append(q)
        q -= step
    return out


def constants(from_q, to_q):
    """(inv, w, binv) of nttmul_bconv_plan: inv[i] = Bh_i^-1 mod b_i, w[i][j] = Bh_i mod c_j,
    binv[j] = B^-1 mod c_j."""
    B = prod(from_q)
    inv = [pow(B // b, -1, b) for b in from_q]
    w = [[(B // b) % c for c in to_q] for b in from_q]
    binv = [pow(B, -1, c) for c in to_q]
    return inv, w, binv


def conv_sum(x, from_q):
    """The integer sum over i of y_i Bh_i for one coefficient's residues x[i]."""
    B = prod(from_q)
    return sum((int(xi) * pow(B // b, -1, b) % b) * (B // b) for xi, b in zip(x, from_q))


def convert_one(x, from_q, to_q):
    s = conv_sum(x, from_q)
    return [s % c for c in to_q]


def moddown_one(x, from_q, to_q):
    """x: residues in the order c_0 .. c_{K-1}, b_0 .. b_{L-1}."""
    K, B = len(to_q), prod(from_q)
    conv = convert_one(x[K:], from_q, to_q)
    return [(int(x[j]) - conv[j]) * pow(B, -1, c) % c for j, c in enumerate(to_q)]


def _objects(x):
    return np.asarray(x).astype(object)


def conv_sums(x, from_q):
    """conv_sum for every coefficient of x [batch, L, n], as an object array [batch, n]."""
    x = _objects(x)
    assert x.ndim == 3 and x.shape[1] == len(from_q)
    B = prod(from_q)
    inv, _, _ = constants(from_q, ())
    return sum((x[:, i, :] * inv[i] % b) * (B // b) for i, b in enumerate(from_q))


def convert(x, from_q, to_q):
    """[batch, L, n] -> [batch, K, n], dtype kept."""
    s = conv_sums(x, from_q)
    return np.stack([s % c for c in to_q], axis=1).astype(np.asarray(x).dtype)


def moddown(x, from_q, to_q):
    """[batch, K + L, n] (limbs of to_q, then of from_q) -> [batch, K, n], dtype kept."""
    K = len(to_q)
    assert np.asarray(x).shape[1] == K + len(from_q)
    s, xo, B = conv_sums(np.asarray(x)[:, K:, :], from_q), _objects(x), prod(from_q)
    return np.stack([(xo[:, j, :] - s) * pow(B, -1, c) % c for j, c in enumerate(to_q)],
                    axis=1).astype(np.asarray(x).dtype)


def crt(x, moduli):
    """The value in [0, prod(moduli)) with residues x."""
    M = prod(moduli)
    return sum(int(xi) * pow(M // m, -1, m) % m * (M // m) for xi, m in zip(x, moduli)) % M


def worst_case(from_q):
    """x[i] = -Bh_i mod b_i: every y_i = b_i - 1 and alpha = L - 1, the accumulator's worst case."""
    B = prod(from_q)
    return [(-(B // b)) % b for b in from_q]


def random_words(rng, moduli, batch, n, dtype):
    """Seeded canonical words [batch, len(moduli), n]: limb l below moduli[l]."""
    out = np.empty((batch, len(moduli), n), dtype=dtype)
    for l, q in enumerate(moduli):
        out[:, l, :] = rng.integers(0, q, size=(batch, n), dtype=np.uint64).astype(dtype)
    return out
