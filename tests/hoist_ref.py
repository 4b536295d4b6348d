"""Python-integer reference of include/nttmul_hoist.h and of the hoisted key switch it serves:
hoist_ntt from its definition (the NTT-order table of tests/galois_ref.py, products and sums in
Python integers or exact 64-bit arithmetic, the oracle's inverse transform), and the chain
modup -> forward -> hoist_ntt -> moddown on tests/ks_ref.py and bconv_ref.py.  No GPU; the
transforms are the CPU oracle's loops the library's forward and inverse are held to
(tests/test_gpu_parity.py test_transforms_vs_oracle)."""
from functools import lru_cache

import numpy as np

import bconv_ref as B
import galois_ref
import hoist_cases as C
import ks_ref
from oracle import oracle as O


@lru_cache(maxsize=None)
def plan(n, q):
    return O.Plan(n, q)


def mulmod(x, y, q):
    """x * y mod q for canonical uint64 arrays."""
    if q < (1 << 32):               # the product of two residues fits 64 bits
        return x * y % np.uint64(q)
    if x.size >= MULMOD_C_WORDS:    # the oracle's 128-bit product, one C loop over all words
        x, y = np.broadcast_arrays(x, y)
        return mulmod_c(x, y, q)
    return mulmod_py(x, y, q)


MULMOD_C_WORDS = 2048               # below: Python integers, cheap at the small degrees


def mulmod_py(x, y, q):
    """x * y mod q in Python integers, whatever q."""
    return ((x.astype(object) * y.astype(object)) % q).astype(np.uint64)


def mulmod_c(x, y, q):
    """x * y mod q by the oracle's pointwise product (oracle/nttmul_oracle.c orc_mul_batch: one
    unsigned 128-bit product and remainder per word), for canonical arrays of one shape.
    tests/test_full_ref.py holds it to mulmod_py."""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    y = np.ascontiguousarray(y, dtype=np.uint64)
    assert x.shape == y.shape
    out = np.empty_like(x)
    u64p = O._u64p
    O.lib().orc_mul_batch(out.ctypes.data_as(u64p), x.ctypes.data_as(u64p),
                          y.ctypes.data_as(u64p), x.size, q)
    return out


def forward(x, moduli):
    """[.., L, n] canonical coefficients -> the bit-reversed canonical transforms, dtype kept."""
    x = np.asarray(x)
    out = np.empty_like(x)
    flat, oflat = x.reshape(-1, len(moduli), x.shape[-1]), out.reshape(-1, len(moduli), x.shape[-1])
    for l, q in enumerate(moduli):
        P = plan(x.shape[-1], q)
        for p in range(flat.shape[0]):
            oflat[p, l] = P.transform("mulntt_ct_std2rev", flat[p, l], "mixed_powers_rev")
    return out


def inverse_one(x_hat, n, q):
    """One bit-reversed transform (uint64 [n]) -> canonical coefficients, scaled by n^-1."""
    P = plan(n, q)
    y = P.transform("nttmul_gs_rev2std", x_hat, "inv_mixed_powers_rev")
    return mulmod(y, np.full(n, pow(n, -1, q), dtype=np.uint64), q)


def hoist(a_hat, b_hat, ks, moduli):
    """c[p][r][i][l] = INTT_l(sum_t a_hat[p][t][l][src_{k_r}(j)] b_hat[r][i][t][l][j]) for a_hat
    [batch, terms, L, n] and b_hat [rots, comps, terms, L, n]; returns [batch, rots, comps, L, n]
    in a_hat's dtype."""
    a_hat, b_hat = np.asarray(a_hat), np.asarray(b_hat)
    batch, terms, L, n = a_hat.shape
    rots, comps = b_hat.shape[:2]
    assert b_hat.shape == (rots, comps, terms, L, n) and rots == len(ks) and L == len(moduli)
    out = np.empty((batch, rots, comps, L, n), dtype=a_hat.dtype)
    for r, k in enumerate(ks):
        src = galois_ref.np_tables(n, int(k))[2]
        ar = a_hat[..., src].astype(np.uint64)                     # sigma_k in NTT order
        for l, q in enumerate(moduli):
            for p in range(batch):
                for i in range(comps):
                    assert q < 1 << 63                             # acc + product < 2q < 2^64
                    acc = np.zeros(n, dtype=np.uint64)
                    for t in range(terms):
                        acc = (acc + mulmod(ar[p, t, l], b_hat[r, i, t, l].astype(np.uint64), q)) \
                            % np.uint64(q)
                    out[p, r, i, l] = inverse_one(acc, n, q)
    return out


def rotate_signed(s, k):
    """sigma_k of a polynomial with signed integer coefficients (a list): x^i -> x^(i k), x^n = -1."""
    n = len(s)
    out = [0] * n
    for i, v in enumerate(s):
        e = i * k % (2 * n)
        if e < n:
            out[e] = int(v)
        else:
            out[e - n] = -int(v)
    return out


@lru_cache(maxsize=None)
def chain(n, bits, bases=None):
    """The hoisted key switch of tests/hoist_cases.py CHAIN at (n, bits), every stage in Python
    integers on seeded inputs: x [batch, L, n] is the c_1 part of ciphertexts under s2; for each
    rotation k_r a zero-noise key switches sigma_k(s2) to s.  Returns a dict of the inputs (q, p,
    alpha, ks, s, s2, x, key [rots, 2, dnum, L + K, n]) and of every stage: up = modup(x), up_hat
    and key_hat = forward, mid = hoist_ntt [batch, rots, 2, L + K, n], out = moddown
    [batch, rots, 2, L, n].  bases: (q, p) of the shape's L and K limbs in place of
    ks_ref.bases(bits, L, K)."""
    L, K, alpha = C.CHAIN_SHAPE
    batch, h, rots = C.CHAIN_BATCH, C.CHAIN_H, C.CHAIN_ROTS
    dt = np.uint32 if bits == 32 else np.uint64
    q, p = ks_ref.bases(bits, L, K) if bases is None else bases
    assert (len(q), len(p)) == (L, K)
    ext, dn = q + p, -(-L // alpha)
    ks = C.draw(n, rots, 1)                                        # 5, 25, 2n - 1
    rng = np.random.default_rng(n + bits)
    s, s2 = ks_ref.ternary(rng, n, h), ks_ref.ternary(rng, n, h)
    key = np.stack([np.stack([c.astype(dt) for c in
                              ks_ref.keygen(rng, n, q, p, alpha, s, rotate_signed(s2, k))])
                    for k in ks])
    x = B.random_words(rng, q, batch, n, dt)
    up = ks_ref.modup(x, q, p, alpha)
    assert up.shape == (batch, dn, L + K, n) and key.shape == (rots, 2, dn, L + K, n)
    up_hat, key_hat = forward(up, ext), forward(key, ext)
    mid = hoist(up_hat, key_hat, ks, ext)
    out = B.moddown(mid.reshape(-1, L + K, n), p, q).reshape(batch, rots, 2, L, n)
    return dict(q=q, p=p, alpha=alpha, ks=ks, s=s, s2=s2, x=x, key=key, up=up, up_hat=up_hat,
                key_hat=key_hat, mid=mid, out=out)


def chain_errors(ch, out=None):
    """The largest |coefficient| of c_0 + c_1 s - sigma_k(x) sigma_k(s2), centered, per (batch
    entry, rotation), for the chain's own out or another [batch, rots, 2, L, n]."""
    out = ch["out"] if out is None else out
    errs = []
    for b in range(out.shape[0]):
        for r, k in enumerate(ch["ks"]):
            xr = galois_ref.coeff(ch["x"][b:b + 1], k, ch["q"])[0]
            errs.append(ks_ref.key_switch_error(xr, out[b, r, 0], out[b, r, 1], ch["q"], ch["s"],
                                                rotate_signed(ch["s2"], k)))
    return errs


def chain_bound():
    """+-(K + 1)(1 + h): tests/test_gpu_ks.py's bound, from moddown's rounding alone (sigma_k is a
    signed permutation of the coefficients and adds nothing)."""
    return (C.CHAIN_SHAPE[1] + 1) * (1 + C.CHAIN_H)
