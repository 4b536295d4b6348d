"""The automorphism sigma_k : a(x) -> a(x^k) mod (x^n + 1) of include/nttmul_galois.h in Python
integers, from its definitions; the reference tests/test_gpu_galois.py compares the kernels with.
Plain arithmetic, no GPU, no library.

Coefficient order.  x^i goes to x^(i k) and x^n = -1: coefficient i lands at e = i k mod 2n, at
index e when e < n, negated at index e - n otherwise (a scatter; k odd makes it a bijection).

NTT order.  Slot j of the project's forward transform holds a(psi^E(j)), E(j) = 2 brv(j) + 1, brv
reversing log2 n bits (tests/test_galois_ref.py holds this against the oracle).  sigma_k(a) at
psi^E(j) is a((psi^E(j))^k) = a(psi^(k E(j) mod 2n)): the slot whose exponent is k E(j) mod 2n.
The source slot is looked up by exponent, not computed by a closed formula."""
from functools import lru_cache

import numpy as np


def brv(x: int, bits: int) -> int:
    return int(format(x, f"0{bits}b")[::-1], 2) if bits else 0


def exponents(n: int) -> list:
    """E(j) for every slot j."""
    bits = n.bit_length() - 1
    return [2 * brv(j, bits) + 1 for j in range(n)]


@lru_cache(maxsize=None)
def tables(n: int, k: int):
    """(coeff_src, coeff_neg, ntt_src) as lists: out[j] = (-in if coeff_neg[j] else in)[coeff_src[j]]
    in coefficient order, out_hat[j] = in_hat[ntt_src[j]] in NTT order."""
    assert n >= 2 and n & (n - 1) == 0 and k % 2 == 1 and 0 < k < 2 * n
    src, neg = [None] * n, [None] * n
    for i in range(n):
        e = i * k % (2 * n)
        j = e if e < n else e - n
        assert src[j] is None
        src[j], neg[j] = i, int(e >= n)
    E = exponents(n)
    slot_of = {e: j for j, e in enumerate(E)}
    assert len(slot_of) == n
    hat = [slot_of[k * e % (2 * n)] for e in E]
    return src, neg, hat


def np_tables(n: int, k: int):
    src, neg, hat = tables(n, k)
    return (np.array(src, dtype=np.int64), np.array(neg, dtype=bool), np.array(hat, dtype=np.int64))


def coeff_one(a, k: int, q: int) -> list:
    """sigma_k of one polynomial (a list of n integers in [0, q)), straight from the scatter."""
    n = len(a)
    out = [None] * n
    for i, x in enumerate(a):
        e = i * k % (2 * n)
        if e < n:
            out[e] = int(x)
        else:
            out[e - n] = (q - int(x)) % q
    return out


def ntt_one(a_hat, k: int) -> list:
    _, _, hat = tables(len(a_hat), k)
    return [int(a_hat[s]) for s in hat]


def coeff(x: np.ndarray, k: int, moduli) -> np.ndarray:
    """x [batch, limbs, n] canonical -> sigma_k per limb, canonical (-0 = 0)."""
    src, neg, _ = np_tables(x.shape[-1], k)
    out = np.empty_like(x)
    for l, q in enumerate(moduli):
        g = x[:, l, :][:, src].astype(np.uint64)
        minus = np.where(g == 0, np.uint64(0), np.uint64(q) - g)
        out[:, l, :] = np.where(neg[None, :], minus, g).astype(x.dtype)
    return out


def ntt(x_hat: np.ndarray, k: int) -> np.ndarray:
    """x_hat [batch, limbs, n] bit-reversed transforms -> sigma_k, a permutation of the slots."""
    _, _, hat = np_tables(x_hat.shape[-1], k)
    return np.ascontiguousarray(x_hat[..., hat])


def element(n: int, step: int, conjugate: bool = False) -> int:
    """5^step mod 2n (negative steps: the inverse of 5), times 2n - 1 when conjugate."""
    m = 2 * n
    k = pow(5, step, m) if step >= 0 else pow(pow(5, -1, m), -step, m)
    return k * (m - 1) % m if conjugate else k


def random_words(rng, moduli, batch: int, n: int, dtype) -> np.ndarray:
    """[batch, limbs, n] words uniform below their limb's modulus, with 0 and q_l - 1 planted in
    every limb of every polynomial (-0 and the largest negation)."""
    x = np.empty((batch, len(moduli), n), dtype=dtype)
    for l, q in enumerate(moduli):
        x[:, l, :] = rng.integers(0, q, size=(batch, n), dtype=np.uint64).astype(dtype)
        for p in range(batch):
            i, j = rng.choice(n, size=2, replace=False)
            x[p, l, i], x[p, l, j] = 0, q - 1
    return x
