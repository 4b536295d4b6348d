"""Integer reference of include/nttmul_ctmul.h, from the header's formulas: exact products and
sums (numpy uint64 on 32-bit words; on 64-bit words hoist_ref.mulmod -- the oracle's 128-bit C
product on whole polynomials, Python integers on short arrays -- and sums that account for the
wrap), no transform.  And the multiplication it serves, high -> modup -> relin -> moddown, on a seeded
zero-noise relinearisation key.  No GPU, but for composition(), which runs the calls of the
contexts it is handed."""
from functools import lru_cache
from math import prod

import numpy as np

import bconv_ref as B
import hoist_cases as HC
import hoist_ref as H
import ks_ref


def p_mod(q, p):
    """P mod q_l for every limb of Q."""
    return [prod(p) % m for m in q]


def _wide(x, m):
    """A canonical array in the integers the products of residues mod m fit: uint64 below 2^32,
    Python integers above."""
    return np.asarray(x).astype(np.uint64 if m < (1 << 32) else object)


def _m(m):
    """m as the scalar that keeps _wide's arrays in their type."""
    return np.uint64(m) if m < (1 << 32) else m


def _mulmod(x, y, m):
    """x y mod m for canonical arrays that broadcast, exact, as uint64: the 64-bit product below
    2^32, hoist_ref.mulmod above (the oracle's 128-bit C product on whole polynomials, Python
    integers on short arrays)."""
    x, y = np.broadcast_arrays(np.asarray(x).astype(np.uint64), np.asarray(y).astype(np.uint64))
    return H.mulmod(x, y, m)


def _addmod(a, b, m):
    """a + b mod m for canonical uint64 arrays and any m < 2^64: the sum wraps exactly when it is
    below a."""
    s = a + b
    return np.where((s < a) | (s >= np.uint64(m)), s - np.uint64(m), s)


def _dot(xs, ys, m):
    """sum over the leading axis of xs[s] ys[s] mod m: [pairs, .., n] -> [.., n], uint64."""
    acc = None
    for x, y in zip(xs, ys):
        t = _mulmod(x, y, m)
        acc = t if acc is None else _addmod(acc, t, m)
    return acc


def tensor(x_hat, y_hat, q):
    """(e_0, e_1, d2) of the header, each [batch, L, n] in x_hat's dtype, for x_hat and y_hat
    [batch, pairs, 2, L, n]."""
    x_hat, y_hat = np.asarray(x_hat), np.asarray(y_hat)
    batch, pairs, two, L, n = x_hat.shape
    assert two == 2 and L == len(q) and y_hat.shape == x_hat.shape
    out = [np.empty((batch, L, n), dtype=x_hat.dtype) for _ in range(3)]
    for l, m in enumerate(q):
        # [pairs, batch, n]: the pairs lead, _dot sums over them
        x0, x1, y0, y1 = (np.moveaxis(v[:, :, i, l], 1, 0) for v in (x_hat, y_hat) for i in (0, 1))
        out[0][:, l] = _dot(x0, y0, m)
        out[1][:, l] = _addmod(_dot(x0, y1, m), _dot(x1, y0, m), m)
        out[2][:, l] = _dot(x1, y1, m)
    return out


def high(x_hat, y_hat, q):
    """d2_hat[p][l][j] = (sum_s x_hat[p][s][1][l][j] y_hat[p][s][1][l][j]) mod q_l."""
    return tensor(x_hat, y_hat, q)[2]


def add_scaled(key_sum, e0, e1, q, p):
    """key_sum [batch, 2, M, n] + (P mod q_l) e_i on the limbs of Q, mod m_l, dtype kept."""
    out = np.array(key_sum)
    for l, (m, pq) in enumerate(zip(q, p_mod(q, p))):
        for i, e in enumerate((e0, e1)):
            scaled = _mulmod(e[:, l], np.uint64(pq), m)
            out[:, i, l] = _addmod(np.asarray(key_sum[:, i, l]).astype(np.uint64), scaled, m)
    return out


def relin(up_hat, key_hat, x_hat, y_hat, q, p):
    """c_hat[p][i][l][j] = (sum_t up_hat[p][t][l][j] key_hat[i][t][l][j]
    + [l < L] (P mod q_l) e_i[p][l][j]) mod m_l for up_hat [batch, terms, M, n], key_hat
    [2, terms, M, n]; returns [batch, 2, M, n] in up_hat's dtype."""
    up_hat, key_hat = np.asarray(up_hat), np.asarray(key_hat)
    ext = tuple(q) + tuple(p)
    batch, terms, M, n = up_hat.shape
    assert key_hat.shape == (2, terms, M, n) and M == len(ext)
    ks = np.empty((batch, 2, M, n), dtype=up_hat.dtype)
    for l, m in enumerate(ext):
        for i in range(2):
            ks[:, i, l] = _dot(np.moveaxis(up_hat[:, :, l], 1, 0), key_hat[i, :, l][:, None], m)
    e0, e1, _ = tensor(x_hat, y_hat, q)
    return add_scaled(ks, e0, e1, q, p)


# ---------------------------------------------------------------------------------------------
# The device composition of existing calls (the reference where Python integers do not reach)
# ---------------------------------------------------------------------------------------------

def limb_products(plain, a, b):
    """a o b per limb with the library's own pointwise product: a, b [.., L, n], plain: one
    nttmul.Context per limb of Q."""
    out = np.empty_like(a)
    for l, ctx in enumerate(plain):
        out[..., l, :] = ctx.pointwise(np.ascontiguousarray(a[..., l, :]),
                                       np.ascontiguousarray(b[..., l, :]), dtype=a.dtype.type)
    return out


def _sum_mod(terms, q):
    """The modular sum over axis 1 of [batch, k, L, n], on the host."""
    out = np.empty(terms.shape[:1] + terms.shape[2:], dtype=terms.dtype)
    for l, m in enumerate(q):
        acc = _wide(np.zeros(out[:, l].shape, dtype=np.uint64), m)
        for s in range(terms.shape[1]):
            acc = (acc + _wide(terms[:, s, l], m)) % _m(m)
        out[:, l] = acc
    return out


def tensor_composition(plain, x_hat, y_hat, q):
    """tensor() from the per-limb pointwise products of the plain contexts and host additions."""
    x0, x1, y0, y1 = x_hat[:, :, 0], x_hat[:, :, 1], y_hat[:, :, 0], y_hat[:, :, 1]
    e0 = _sum_mod(limb_products(plain, x0, y0), q)
    cross = np.concatenate((limb_products(plain, x0, y1), limb_products(plain, x1, y0)), axis=1)
    return e0, _sum_mod(cross, q), _sum_mod(limb_products(plain, x1, y1), q)


def composition(kn, plain, up_hat, key_hat, x_hat, y_hat, q, p):
    """relin as the composition it replaces: kn.mac (an nttmul.NttKeySwitch over q, p) with
    k = (1,) for the key sum, the per-limb pointwise products for the tensor terms, host modular
    additions."""
    ks = kn.mac(up_hat, key_hat[None], (1,))[:, 0]                  # [batch, 2, M, n]
    e0, e1, _ = tensor_composition(plain, x_hat, y_hat, q)
    return add_scaled(ks, e0, e1, q, p)


# ---------------------------------------------------------------------------------------------
# The multiplication end to end
# ---------------------------------------------------------------------------------------------

def chain_bound():
    """+-(K + 1)(1 + h) per limb, centred.  With a zero-noise key c_hat[0] + c_hat[1] s =
    P (d0 + d1 s + d2 s^2) mod QP exactly; ModDown's output is (Y_i - r_i) / P with
    0 <= r_i < (K + 1) P, the rounding of one key switch, whatever `pairs` is."""
    return (HC.CHAIN_SHAPE[1] + 1) * (1 + HC.CHAIN_H)


def chain_inputs(n, bits, pairs=1, batch=None, bases=None):
    """Seeded inputs of the multiplication on hoist_cases.CHAIN_SHAPE: q, p, alpha, a ternary s of
    weight CHAIN_H, ss = s s as signed integers, the zero-noise key (b, a) [2, dnum, L + K, n] that
    switches s s to s, and random words x, y [batch, pairs, 2, L, n] over Q (coefficient order).  bases: (q, p) of the
    shape's L and K limbs in place of ks_ref.bases(bits, L, K)."""
    L, K, alpha = HC.CHAIN_SHAPE
    batch = HC.CHAIN_BATCH if batch is None else batch
    dt = np.uint32 if bits == 32 else np.uint64
    q, p = ks_ref.bases(bits, L, K) if bases is None else bases
    assert (len(q), len(p)) == (L, K)
    rng = np.random.default_rng(3 * n + bits + pairs)
    s = ks_ref.ternary(rng, n, HC.CHAIN_H)
    ss = signed_square(s)
    key = np.stack([c.astype(dt) for c in ks_ref.keygen(rng, n, q, p, alpha, s, ss)])
    x = B.random_words(rng, q * (2 * pairs), batch, n, dt).reshape(batch, pairs, 2, L, n)
    y = B.random_words(rng, q * (2 * pairs), batch, n, dt).reshape(batch, pairs, 2, L, n)
    return dict(q=q, p=p, alpha=alpha, s=s, ss=ss, key=key, x=x, y=y)


def signed_square(s):
    """s s mod x^n + 1 over the integers, a list of signed integers."""
    n = len(s)
    out = [0] * n
    nz = [(i, v) for i, v in enumerate(s) if v]
    for i, a in nz:
        for j, b in nz:
            if i + j < n:
                out[i + j] += a * b
            else:
                out[i + j - n] -= a * b
    return out


@lru_cache(maxsize=None)
def chain(n, bits, pairs=1, bases=None):
    """The multiplication in Python integers at small n: chain_inputs plus x_hat, y_hat, key_hat,
    d2_hat = high, up_hat = forward(modup(inverse(d2_hat))), mid = relin [batch, 2, L + K, n]
    (NTT order), out = moddown of its inverse [batch, 2, L, n] (coefficient order), and
    d = (d0, d1, d2) [3, batch, L, n], the inverse of the pointwise products (coefficient
    order)."""
    ch = chain_inputs(n, bits, pairs, bases=bases)
    q, p = ch["q"], ch["p"]
    ext, L = q + p, len(q)
    dt = ch["x"].dtype
    batch = ch["x"].shape[0]
    x_hat, y_hat, key_hat = H.forward(ch["x"], q), H.forward(ch["y"], q), H.forward(ch["key"], ext)
    e0, e1, d2_hat = tensor(x_hat, y_hat, q)
    d = np.stack([coefficients(e, q) for e in (e0, e1, d2_hat)])
    up_hat = H.forward(ks_ref.modup(d[2], q, p, ch["alpha"]), ext)
    mid = relin(up_hat, key_hat, x_hat, y_hat, q, p)
    out = B.moddown(coefficients(mid.reshape(-1, len(ext), n), ext), p, q).reshape(batch, 2, L, n)
    ch.update(x_hat=x_hat, y_hat=y_hat, key_hat=key_hat, d2_hat=d2_hat, d=d, up_hat=up_hat,
              mid=mid, out=out)
    return ch


def coefficients(x_hat, moduli):
    """[batch, M, n] transforms -> canonical coefficients, dtype kept (the oracle's inverse)."""
    return np.stack([np.stack([H.inverse_one(x_hat[u, l].astype(np.uint64), x_hat.shape[-1],
                                             m).astype(x_hat.dtype)
                               for l, m in enumerate(moduli)]) for u in range(x_hat.shape[0])])


def chain_errors(ch, out, d):
    """The largest |coefficient| of c0' + c1' s - (d0 + d1 s + d2 s^2), centred, over the limbs of
    Q, per batch entry: out [batch, 2, L, n] and d [3, batch, L, n] in coefficient order."""
    q, s, ss = ch["q"], ch["s"], ch["ss"]
    errs = []
    for b in range(out.shape[0]):
        worst = 0
        for i, m in enumerate(q):
            want = (d[0][b, i].astype(object) + ks_ref.negacyclic(s, d[1][b, i], m)
                    + ks_ref.negacyclic(ss, d[2][b, i], m))
            e = (out[b, 0, i].astype(object) + ks_ref.negacyclic(s, out[b, 1, i], m) - want) % m
            worst = max(worst, max(int(min(v, m - v)) for v in e))
        errs.append(worst)
    return errs
