"""Inputs that saturate a stage boundary, and their products in closed form.

Both transforms peel x^n + 1 into factors x^m - z, so a polynomial of degree < m is its own
residue in every block once the stages have left blocks of m coefficients.  S(m, v), the first m
coefficients v and the rest 0, therefore puts v in every position at that boundary: S(m, q - 1)
in both operands of a fused product with m = 2^D makes every base block all q - 1 (its last
output sums B (q - 1)^2 exactly, the worst case of the basemul folds), and S(1, q - 1) makes the
whole NTT-domain operand q - 1.

The product needs no oracle: S(ma, va) S(mb, vb) = va vb (conv[:n] - conv[n:]) mod q with
conv = ones(ma) * ones(mb).  Plain numpy and Python integers; no GPU, no library."""
import numpy as np


def sizes(n):
    """m = 1, 2, 4, ..., n."""
    return [1 << k for k in range(n.bit_length())]


def poly(n, m, v):
    x = np.zeros(n, dtype=np.uint64)
    x[:m] = v
    return x


def ones_conv(ma, mb, length):
    """np.convolve(ones(ma), ones(mb)) padded to `length`, without the quadratic work:
    conv[k] = #{(i, j): i + j = k, i < ma, j < mb}."""
    k = np.arange(length, dtype=np.int64)
    return np.maximum(0, np.minimum(k, ma - 1) - np.maximum(0, k - mb + 1) + 1)


def product(n, q, ma, va, mb, vb):
    """S(ma, va) S(mb, vb) mod (x^n + 1, q)."""
    conv = ones_conv(ma, mb, 2 * n)
    d = (conv[:n] - conv[n:]).astype(object)
    return ((va * vb % q) * d % q).astype(np.uint64)


def family(n, q):
    """The (a, b, expected product) rows of one launch: every (m, m) pair with
    (va, vb) in {(q - 1, q - 1), (q - 1, 1)}."""
    a, b, c = [], [], []
    for m in sizes(n):
        for va, vb in ((q - 1, q - 1), (q - 1, 1)):
            a.append(poly(n, m, va))
            b.append(poly(n, m, vb))
            c.append(product(n, q, m, va, m, vb))
    return np.stack(a), np.stack(b), np.stack(c)
