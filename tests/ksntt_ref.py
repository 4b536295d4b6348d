"""Python-integer reference of include/nttmul_ksntt.h, from the header's formulas: modup (only the
L limbs of Q are transformed back, the digit sums are formed in Python integers and transformed
forward under every modulus that is not the digit's own, the own limbs are copies) and mac (the
slot table of tests/galois_ref.py, products and sums in Python integers, no transform).  The
compositions they replace are spelled out beside them on ks_ref, mdntt_ref and hoist_ref.  No GPU."""
from math import prod

import numpy as np

import galois_ref
import hoist_ref as H
import ks_ref
import mdntt_ref


def modup(x_hat, q, p, alpha):
    """[batch, L, n] NTT order -> [batch, dnum, L + K, n] NTT order, dtype kept."""
    x_hat = np.asarray(x_hat)
    q, p = tuple(q), tuple(p)
    ext, L, n = q + p, len(q), x_hat.shape[-1]
    assert x_hat.ndim == 3 and x_hat.shape[1] == L
    digs = ks_ref.digits(L, alpha)
    out = np.empty((x_hat.shape[0], len(digs), len(ext), n), dtype=x_hat.dtype)
    for b in range(x_hat.shape[0]):
        for d, D in enumerate(digs):
            Dd = prod(q[i] for i in D)
            s = np.zeros(n, dtype=object)
            for i in D:
                Dh = Dd // q[i]
                y = H.inverse_one(x_hat[b, i].astype(np.uint64), n, q[i]).astype(object)
                s += (y * pow(Dh, -1, q[i]) % q[i]) * Dh
            for m, mod in enumerate(ext):
                if m in D:
                    out[b, d, m] = x_hat[b, m]                     # a copy, no arithmetic
                    continue
                r = np.array([int(v) % mod for v in s], dtype=x_hat.dtype)
                out[b, d, m] = H.forward(r[None, None, :], (mod,))[0, 0]
    return out


def modup_composition(x_hat, q, p, alpha):
    """forward_{Q u P}(ks_modup(inverse_Q(x_hat))): identity (A)'s right-hand side."""
    q, p = tuple(q), tuple(p)
    return H.forward(ks_ref.modup(mdntt_ref.inverse(x_hat, q), q, p, alpha), q + p)


def mac(a_hat, b_hat, ks, moduli):
    """c_hat[p][r][i][l][j] = (sum_t a_hat[p][t][l][src_{k_r}(j)] b_hat[r][i][t][l][j]) mod m_l for
    a_hat [batch, terms, M, n] and b_hat [rots, comps, terms, M, n]; returns
    [batch, rots, comps, M, n] in a_hat's dtype."""
    a_hat, b_hat = np.asarray(a_hat), np.asarray(b_hat)
    batch, terms, M, n = a_hat.shape
    rots, comps = b_hat.shape[:2]
    assert b_hat.shape == (rots, comps, terms, M, n) and rots == len(ks) and M == len(moduli)
    out = np.empty((batch, rots, comps, M, n), dtype=a_hat.dtype)
    for r, k in enumerate(ks):
        src = galois_ref.np_tables(n, int(k))[2]
        ar = a_hat[..., src].astype(np.uint64)
        for l, m in enumerate(moduli):
            if m >= 1 << 63:                                       # acc + product may pass 2^64
                out[:, r, :, l] = mac_python(a_hat[:, :, l:l + 1], b_hat[r:r + 1, :, :, l:l + 1],
                                             (k,), (m,))[:, 0, :, 0]
                continue
            for i in range(comps):
                acc = np.zeros((batch, n), dtype=np.uint64)
                for t in range(terms):                             # every batch entry at once
                    bt = np.broadcast_to(b_hat[r, i, t, l].astype(np.uint64), (batch, n))
                    acc = (acc + H.mulmod(np.ascontiguousarray(ar[:, t, l]), bt, m)) % np.uint64(m)
                out[:, r, i, l] = acc.astype(a_hat.dtype)
    return out


def mac_python(a_hat, b_hat, ks, moduli):
    """mac with every product and sum in Python integers (object arrays): what mac's exact 64-bit
    arithmetic is held to (tests/test_ksntt_ref.py)."""
    a_hat, b_hat = np.asarray(a_hat), np.asarray(b_hat)
    batch, terms, M, n = a_hat.shape
    rots, comps = b_hat.shape[:2]
    out = np.empty((batch, rots, comps, M, n), dtype=a_hat.dtype)
    for r, k in enumerate(ks):
        src = galois_ref.np_tables(n, int(k))[2]
        ar = a_hat[..., src].astype(object)
        for l, m in enumerate(moduli):
            bl = b_hat[r, :, :, l].astype(object)                  # [comps, terms, n]
            for pp in range(batch):
                for i in range(comps):
                    out[pp, r, i, l] = ((ar[pp, :, l] * bl[i]).sum(axis=0) % m).astype(a_hat.dtype)
    return out


def mac_composition(a_hat, b_hat, ks, moduli):
    """forward(hoist_ntt(a_hat, b_hat, k)): identity (B)'s right-hand side."""
    return H.forward(H.hoist(a_hat, b_hat, ks, moduli), tuple(moduli))


def worst_x_hat(q, alpha, batch, n, dtype):
    """x_hat whose coefficient-order digits are ks_ref.worst_case in every coefficient: every
    y_i = q_i - 1 in the conversion sums."""
    x = np.empty((batch, len(q), n), dtype=dtype)
    for i, v in enumerate(ks_ref.worst_case(q, alpha)):
        x[:, i, :] = v
    return H.forward(x, tuple(q))
