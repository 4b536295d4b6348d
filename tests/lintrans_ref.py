"""Python-integer reference of include/nttmul_lintrans.h, from the header's formula: the slot table
of tests/galois_ref.py, products and sums in Python integers (hoist_ref.mulmod for one product),
no transform.  And the linear transform it serves, modup -> apply -> moddown, on the seeded keys of
hoist_ref.chain.  No GPU, but for composition(), which runs the calls of the context it is handed."""
from functools import lru_cache
from math import prod

import numpy as np

import bconv_ref as B
import galois_ref
import hoist_ref as H
import ks_ref

CHAIN_WEIGHT_H = 3          # non-zero coefficients of a chain weight polynomial
CHAIN_WEIGHT_MAX = 4        # their magnitudes are 1 .. CHAIN_WEIGHT_MAX


def p_mod(q, p):
    """P mod q_l for every limb of Q."""
    return [prod(p) % m for m in q]


def apply(a_hat, b_hat, ks, q, p, w_hat=None, c0_hat=None):
    """c_hat[p][i][l][j] = (sum_r w_hat[r][l][j] (sum_t a_hat[p][t][l][src_{k_r}(j)]
    b_hat[r][i][t][l][j] + [i = 0, l < L] (P mod q_l) c0_hat[p][l][src_{k_r}(j)])) mod m_l for
    a_hat [batch, terms, M, n], b_hat [rots, comps, terms, M, n], w_hat [rots, M, n] or None (all
    ones), c0_hat [batch, L, n] or None (dropped); returns [batch, comps, M, n] in a_hat's dtype."""
    a_hat, b_hat = np.asarray(a_hat), np.asarray(b_hat)
    ext, L = tuple(q) + tuple(p), len(q)
    batch, terms, M, n = a_hat.shape
    rots, comps = b_hat.shape[:2]
    assert b_hat.shape == (rots, comps, terms, M, n) and rots == len(ks) and M == len(ext)
    assert w_hat is None or np.asarray(w_hat).shape == (rots, M, n)
    assert c0_hat is None or np.asarray(c0_hat).shape == (batch, L, n)
    pq = p_mod(q, p)
    out = np.empty((batch, comps, M, n), dtype=a_hat.dtype)
    srcs = [galois_ref.np_tables(n, int(k))[2] for k in ks]
    for l, m in enumerate(ext):
        for pp in range(batch):
            for i in range(comps):
                acc = np.zeros(n, dtype=np.uint64)
                for r, src in enumerate(srcs):
                    inner = np.zeros(n, dtype=np.uint64)
                    for t in range(terms):
                        inner = (inner + H.mulmod(a_hat[pp, t, l][src].astype(np.uint64),
                                                  b_hat[r, i, t, l].astype(np.uint64), m)) % np.uint64(m)
                    if c0_hat is not None and i == 0 and l < L:
                        z = np.asarray(c0_hat)[pp, l][src].astype(np.uint64)
                        inner = (inner + H.mulmod(z, np.full(n, pq[l], dtype=np.uint64), m)) % np.uint64(m)
                    if w_hat is not None:
                        inner = H.mulmod(inner, np.asarray(w_hat)[r, l].astype(np.uint64), m)
                    acc = (acc + inner) % np.uint64(m)
                out[pp, i, l] = acc.astype(a_hat.dtype)
    return out


def composition(kn, a, b, ks, q, p, w=None, c0=None):
    """apply as the composition of existing calls on the device (kn: an nttmul.NttKeySwitch over
    q, p; its host forms) and one host addition: the reference at the degrees Python integers do
    not reach."""
    ext, L = q + p, len(q)
    batch, terms, M, n = a.shape
    rots, comps = b.shape[:2]
    dt = a.dtype
    ones = np.ones((rots, M, n), dtype=dt)
    wt = ones if w is None else w
    m = kn.mac(a, b, ks)                                            # [batch, rots, comps, M, n]
    m = np.ascontiguousarray(m.transpose(0, 2, 1, 3, 4)).reshape(batch * comps, rots, M, n)
    out = kn.mac(m, wt[None, None], (1,)).reshape(batch, comps, M, n)
    if c0 is not None:
        pad = np.zeros((batch, 1, M, n), dtype=dt)
        pad[:, 0, :L] = c0
        wp = np.zeros((rots, M, n), dtype=dt)
        for l, (mod, pq) in enumerate(zip(q, p_mod(q, p))):
            wp[:, l] = H.mulmod(wt[:, l].astype(np.uint64), np.full(n, pq, dtype=np.uint64),
                                mod).astype(dt)
        z = kn.mac(pad, wp[:, None, None], ks)[:, :, 0]              # [batch, rots, M, n]
        zs = kn.mac(z, ones[None, None], (1,)).reshape(batch, M, n)
        for l, mod in enumerate(ext):
            s = out[:, 0, l].astype(np.uint64) + zs[:, l].astype(np.uint64)
            out[:, 0, l] = (s % np.uint64(mod)).astype(dt)
    return out


def signed_weights(rng, n, rots):
    """`rots` small signed polynomials (lists), CHAIN_WEIGHT_H coefficients of magnitude 1 ..
    CHAIN_WEIGHT_MAX each."""
    ws = []
    for _ in range(rots):
        w = [0] * n
        for i in rng.choice(n, size=CHAIN_WEIGHT_H, replace=False):
            w[int(i)] = int(rng.integers(1, CHAIN_WEIGHT_MAX + 1)) * int(rng.choice((-1, 1)))
        ws.append(w)
    return ws


def weights_hat(ws, moduli, n, dtype):
    """The forward transforms of signed polynomials over `moduli`: [rots, M, n]."""
    w = np.array([[[v % m for v in poly] for m in moduli] for poly in ws], dtype=dtype)
    return H.forward(w, tuple(moduli))


@lru_cache(maxsize=None)
def chain(n, bits, bases=None):
    """The linear transform sum_r w_r sigma_{k_r}(.) of the ciphertexts (c0, x) under s2 of
    hoist_ref.chain(n, bits), with its keys: a seeded c0 [batch, L, n], seeded weights, and every
    stage in Python integers.  Returns hoist_ref.chain's dict extended by c0, c0_hat, ws (signed
    lists), w_hat [rots, L + K, n], mid_lt = apply [batch, 2, L + K, n] (NTT order) and out_lt =
    moddown of its inverse [batch, 2, L, n] (coefficient order).  bases: as hoist_ref.chain's."""
    ch = dict(H.chain(n, bits, bases))
    q, p = ch["q"], ch["p"]
    ext, L = q + p, len(q)
    dt = ch["x"].dtype
    rng = np.random.default_rng(7 * n + bits)
    batch, rots = ch["x"].shape[0], len(ch["ks"])
    c0 = B.random_words(rng, q, batch, n, dt)
    ws = signed_weights(rng, n, rots)
    w_hat = weights_hat(ws, ext, n, dt)
    c0_hat = H.forward(c0, q)
    mid = apply(ch["up_hat"], ch["key_hat"], ch["ks"], q, p, w_hat, c0_hat)
    flat = mid.reshape(-1, len(ext), n)
    coeff = np.stack([np.stack([H.inverse_one(flat[u, l].astype(np.uint64), n, m).astype(dt)
                                for l, m in enumerate(ext)]) for u in range(flat.shape[0])])
    out = B.moddown(coeff, p, q).reshape(batch, 2, L, n)
    ch.update(c0=c0, c0_hat=c0_hat, ws=ws, w_hat=w_hat, mid_lt=mid, out_lt=out)
    return ch


def chain_errors(ch, out=None):
    """The largest |coefficient| of c0' + c1' s - sum_r w_r sigma_{k_r}(c0 + x s2), centered, over
    the limbs of Q, per batch entry, for the chain's own out_lt or another [batch, 2, L, n] in
    coefficient order."""
    out = ch["out_lt"] if out is None else out
    q, s, s2 = ch["q"], ch["s"], ch["s2"]
    errs = []
    for b in range(out.shape[0]):
        worst = 0
        for i, m in enumerate(q):
            msg = (ch["c0"][b, i].astype(object) + ks_ref.negacyclic(s2, ch["x"][b, i], m)) % m
            want = np.zeros(len(msg), dtype=object)
            for w, k in zip(ch["ws"], ch["ks"]):
                rot = galois_ref.coeff_one(list(msg), int(k), m)
                want += ks_ref.negacyclic(w, rot, m)
            e = (out[b, 0, i].astype(object) + ks_ref.negacyclic(s, out[b, 1, i], m) - want) % m
            worst = max(worst, max(int(min(v, m - v)) for v in e))
        errs.append(worst)
    return errs
