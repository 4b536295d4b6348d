"""The Galois elements tests/test_gpu_galois_sweep.py runs, the rows of that sweep, and the slot
permutation of sigma_k read off a transform's data: plain data and arithmetic, no GPU, no library.

Which bits of a slot index sigma_k moves is decided by the 2-adic valuations of k - 1 and k + 1, so
S(n) holds, for every j = 1 .. log2 n, the four elements 2^j + 1, 2^j - 1, 2n - 2^j + 1 and
2n - 2^j - 1, and 16 more drawn by a seeded generator: every valuation an odd k < 2n can have
(tests/test_galois_sweep.py).  At n = 256 it is all 256 odd k.

derived_perm does not know galois_slot's formula (csrc/galois_dev.hpp) nor its mirror
(tests/galois_ref.py).  The forward transform of the monomial x holds psi^E(j) in slot j, n
pairwise distinct words; sigma_k(x) = x^k = +-x^(k mod n) transforms to (psi^E(j))^k, which is the
word of x's transform in the slot sigma_k reads slot j from.  Matching equal words gives src."""
from collections import namedtuple

import numpy as np

import galois_cases
import hoist_cases
import ksntt_cases
import lintrans_cases

SEED, DRAWN, LIST = 20240, 16, 16
ALL_N = galois_cases.ALL_N
FULL_N = 256                                   # every odd k


def S(n):
    """The elements run at n, ascending."""
    assert n in ALL_N
    if n == FULL_N:
        return tuple(range(1, 2 * n, 2))
    m, ks = 2 * n, set()
    for j in range(1, n.bit_length()):
        ks |= {(1 << j) + 1, (1 << j) - 1, m - (1 << j) + 1, m - (1 << j) - 1}
    rng = np.random.default_rng(SEED + n)
    ks |= {2 * int(v) + 1 for v in rng.integers(0, n, size=DRAWN)}
    assert all(k % 2 == 1 and 0 < k < m for k in ks)
    return tuple(sorted(ks))


def lists(n, size=LIST):
    """S(n) cut into call lists of at most `size`.  The identity stands in the middle of its list,
    not first: a call whose first element is 1 must not be taken for the plain mac."""
    ks = S(n)
    out = [list(ks[i:i + size]) for i in range(0, len(ks), size)]
    for ls in out:
        if 1 in ls and len(ls) > 1:
            ls.remove(1)
            ls.insert(len(ls) // 2 + 1, 1)
    return [tuple(ls) for ls in out]


def valuation(v, n):
    """v2 of v mod 2n, with 0 counted as 2n: 1 .. log2 n + 1 for an even v."""
    v %= 2 * n
    v = v or 2 * n
    return (v & -v).bit_length() - 1


def monomial_image(n, k, moduli, dtype):
    """sigma_k(x) = x^k mod (x^n + 1) from the definition, [limbs, n]: coefficient k is 1 for
    k < n, coefficient k - n is -1 = q_l - 1 otherwise."""
    out = np.zeros((len(moduli), n), dtype=dtype)
    for l, q in enumerate(moduli):
        out[l, k % n] = 1 if k < n else q - 1
    return out


def derived_perm(fwd_x, fwd_xk):
    """src with fwd_xk[j] == fwd_x[src[j]]: fwd_x the forward transform of x under one modulus,
    fwd_xk that of sigma_k(x) under the same."""
    fwd_x, fwd_xk = np.asarray(fwd_x), np.asarray(fwd_xk)
    assert fwd_x.ndim == 1 and fwd_x.shape == fwd_xk.shape
    order = np.argsort(fwd_x, kind="stable")
    ranked = fwd_x[order]
    assert bool((ranked[1:] != ranked[:-1]).all()), "the words psi^E(j) are pairwise distinct"
    src = order[np.minimum(np.searchsorted(ranked, fwd_xk), len(ranked) - 1)]
    assert np.array_equal(fwd_x[src], fwd_xk), "sigma_k(x) transforms to a permutation of x's words"
    assert np.array_equal(np.sort(src), np.arange(len(src)))
    return src.astype(np.int64)


# ---------------------------------------------------------------------------------------------
# The rows of the sweep: (operation, word bits, n) and the kernels each launches, by the mirrors
# ---------------------------------------------------------------------------------------------

LIMBS, BATCH, TERMS, COMPS = 2, 5, 2, 2
COEFF_N = (256, 4096, 16384, 32768, 65536)     # every staging form of k_galois_coeff, both classes
NTT_N = (256, 4096, 8192, 65536)
HOIST_N = hoist_cases.ALL_N                    # Gr::off differs per log n, multi-pass per n
MAC_N = (256, 512, 4096, 8192, 65536)
OPS = {"coeff": COEFF_N, "ntt": NTT_N, "ntt_many": NTT_N, "hoist": HOIST_N, "ksntt_mac": MAC_N,
       "lintrans_one": MAC_N, "lintrans_sum": MAC_N}
PREFIXES = ("k_galois_", "k_rns_hoist", "k_rnsmp_hoist", "k_ksntt_mac", "k_lintrans")

Row = namedtuple("Row", "op bits n")


def rows():
    return [Row(op, bits, n) for op, ns in OPS.items() for bits in (32, 64) for n in ns]


def moduli(bits):
    """rnsmp_cases.BASIS32 / BASIS64, cut to two limbs."""
    import rnsmp_cases
    return (rnsmp_cases.BASIS32 if bits == 32 else rnsmp_cases.BASIS64)[:LIMBS]


def kernels_of(row):
    """The automorphism kernels a row launches (the identity reference calls launch the same)."""
    m = moduli(row.bits)
    if row.op in ("coeff", "ntt", "ntt_many"):
        return [galois_cases.kernel_name(row.op, row.n, m)]
    if row.op == "hoist":
        return [hoist_cases.hoist_kernel(row.n, m, COMPS)]
    if row.op == "ksntt_mac":
        return ksntt_cases.sequence("mac", row.n, row.bits, COMPS)
    # one rotation per call with weights and c0; sixteen with neither
    return [lintrans_cases.kernel_name(row.bits, COMPS, row.op == "lintrans_one")]


# Kernels of the ledgers the sweep does not launch: (regular expression over the kernel key, reason)
SWEEP_EXEMPT = (
    (r"^k_(rns_hoist|rnsmp_hoist|ksntt_mac)<.*,1>$|^k_lintrans<\w+,\w+,1,[01]>$",
     "one component: the gather of a lane's sources is written once and does not depend on the "
     "component count, which only sets how many b_hat operands meet the gathered words"),
)
