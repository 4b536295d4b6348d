"""The limb-aware libraries on bases of mixed limb sizes (tests/basis_cases.py): a modulus at the
bottom of the 64-bit class, RNS chains whose limbs run from 33 to 62 bits (from 20 to 31 on 32-bit
words) in an order that is not sorted, and the reversed chains whose P lies below every q.  The
other case tables take their 64-bit moduli from the top of the class, all within a few multiples
of 2^17 of each other; here a canonical word of a large limb meets the arithmetic of a small one
and the other way round, in every kernel that moves words between limbs, and every per-pair host
constant (Bh_i mod c_j, P^-1, 2^64 mod c of a 33-bit c) is built for limbs of different sizes.

Every operation is compared bit for bit, every output preset to the sentinel, on seeded canonical
inputs, with the references the other GPU tests of the library use: Python integers at n = 256
(bconv_ref, ks_ref, mdntt_ref, ksntt_ref, lintrans_ref, ctmul_ref), and at n = 8192, the first
multi-pass n (bconv: 4096, its limit), Python integers where they reach (bconv, ks, ksntt) and
otherwise the device composition of calls held on their own (mdntt, lintrans, ctmul).  The
multi-pass limb kernels are held limb by limb to plain contexts of (n, q_l), the product to the
oracle as well.  The shapes are (L, K, alpha) = (4, 2, 2) and (3, 2, 2), whose last digit has one
limb, and for the digit calls (4, 2, 1), where every digit is one small or one large limb; the
batch is 5: one whole workgroup of four units and a partial one.

Worst-case fills (every y_i = b_i - 1 under every target modulus; every word at its own modulus
- 1) run on the chains and the reversed chains with the summed limb count on both sides of the
fold cadence.  The three chains -- key switch, linear transform, ciphertext product -- run at
n = 256 on chain64 and chain32 with zero-noise keys of ks_ref.keygen on the profile's bases and
are held to the bound hoist_ref.chain_bound() / ctmul_ref.chain_bound() derive, which does not
depend on the limbs' sizes.  NTTMUL_FLAG_VALIDATE: the smallest limb's modulus in that limb is
NTTMUL_ERANGE, the same value in the largest limb is accepted."""
import numpy as np
import pytest

import basis_cases as BC
import bconv_ref as B
import ctmul_ref
import galois_ref
import hoist_cases as HC
import hoist_ref as H
import ks_ref
import ksntt_ref
import lintrans_ref
import mdntt_ref
import nttmul
from oracle import oracle as O

pytestmark = pytest.mark.gpu

BATCH = 5
SHAPES = ((4, 2, 2), (3, 2, 2))
DIGIT_SHAPES = SHAPES + ((4, 2, 1),)           # ks and ksntt: dnum = L
SMALL_N, BIG_N, BCONV_N = 256, 8192, 4096
PROFILES = tuple(BC.PROFILES)
MP_PROFILES = ("chain64", "bottom64", "chain32")
MP_OPS = ("multiply", "forward", "inverse", "mac_ntt", "macn_ntt", "hoist_ntt")
FILL_N = (256, 4096)
FILL_COUNTS = {64: (3, 4, 5), 32: (1, 2, 3)}   # both sides of the fold cadence of 4 and of 2
FILLS = ("worst", "top")
FILL_OPS = ("convert", "ks_modup", "mdntt_moddown", "ksntt_modup")
CHAIN_PROFILES = ("chain64", "chain32")
VALIDATE_OPS = ("ks", "mdntt", "ksntt", "lintrans", "ctmul")
TERMS, COMPS, PAIRS = 3, 2, (1, 3)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _to_dev(torch, x, bits):
    x = np.ascontiguousarray(x, dtype=_dt(bits))
    return torch.from_numpy(x.view(np.int32 if bits == 32 else np.int64).reshape(-1)).cuda()


def _run(torch, bits, shape, call, *operands):
    """call(out, *device operands) with out preset to the sentinel; returns out [shape] and checks
    that no operand changed."""
    out = torch.full((int(np.prod(shape)),), -1, dtype=torch.int32 if bits == 32 else torch.int64,
                     device="cuda")
    dev = [None if x is None else _to_dev(torch, x, bits) for x in operands]
    call(out, *dev)
    torch.cuda.synchronize()
    for x, d in zip(operands, dev):
        assert x is None or np.array_equal(d.cpu().numpy().view(_dt(bits)).reshape(x.shape), x)
    return out.cpu().numpy().view(_dt(bits)).reshape(shape)


def _seed(profile, *key):
    return np.random.default_rng([PROFILES.index(profile)] + [int(k) for k in key])


def _hoist_ctx(n):
    return nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext


def _cases(ns, shapes=SHAPES, profiles=PROFILES):
    return [pytest.param(p, n, s, id=f"{p}-n{n}-{'.'.join(map(str, s))}")
            for p in profiles for n in ns for s in shapes]


# ---------------------------------------------------------------------------------------------
# The device calls
# ---------------------------------------------------------------------------------------------

def _bconv(torch, n, from_q, to_q, op, x):
    bits = 8 * x.dtype.itemsize
    with nttmul.BaseConverter(n, from_q, to_q) as conv:
        assert (conv.from_limbs, conv.to_limbs, conv.word_bits) == (len(from_q), len(to_q), bits)
        return _run(torch, bits, (x.shape[0], len(to_q), n),
                    lambda out, dx: getattr(conv, f"{op}_device")(out, dx, x.shape[0]), x)


def _ks(torch, n, q, p, alpha, op, x, validate=False):
    bits, batch = 8 * x.dtype.itemsize, x.shape[0]
    with nttmul.KeySwitchBasis(n, q, p, alpha, validate=validate) as ks:
        assert (ks.q_limbs, ks.p_limbs, ks.word_bits) == (len(q), len(p), bits)
        shape = (batch, ks.digits, len(q) + len(p), n) if op == "modup" else (batch, len(q), n)
        return _run(torch, bits, shape,
                    lambda out, dx: getattr(ks, f"{op}_device")(out, dx, batch), x)


def _mdntt(torch, n, q, p, x_hat, validate=False):
    bits, batch = 8 * x_hat.dtype.itemsize, x_hat.shape[0]
    with nttmul.NttModDown(n, q, p, validate=validate) as md:
        assert (md.q_limbs, md.p_limbs, md.word_bits) == (len(q), len(p), bits)
        return _run(torch, bits, (batch, len(q), n),
                    lambda out, dx: md.moddown_device(out, dx, batch), x_hat)


def _ksntt_modup(torch, n, q, p, alpha, x_hat, validate=False):
    bits, batch = 8 * x_hat.dtype.itemsize, x_hat.shape[0]
    with nttmul.NttKeySwitch(n, q, p, alpha, validate=validate) as kn:
        assert (kn.q_limbs, kn.p_limbs, kn.word_bits) == (len(q), len(p), bits)
        return _run(torch, bits, (batch, kn.digits, kn.limbs, n),
                    lambda out, dx: kn.modup_device(out, dx, batch), x_hat)


def _ksntt_mac(torch, kn, a, b, ks):
    (batch, terms), (rots, comps) = a.shape[:2], b.shape[:2]
    return _run(torch, kn.word_bits, (batch, rots, comps, kn.limbs, kn.n),
                lambda out, da, db: kn.mac_device(out, da, db, ks, batch, terms, comps), a, b)


def _lintrans(torch, lt, a, b, ks, w, c0):
    (batch, terms), comps = a.shape[:2], b.shape[1]
    return _run(torch, lt.word_bits, (batch, comps, lt.limbs, lt.n),
                lambda out, da, db, dw, dz: lt.apply_device(out, da, db, ks, batch, terms, comps,
                                                            w_hat=dw, c0_hat=dz), a, b, w, c0)


def _ct_high(torch, ct, x, y):
    batch, pairs = x.shape[:2]
    return _run(torch, ct.word_bits, (batch, ct.q_limbs, ct.n),
                lambda out, dx, dy: ct.high_device(out, dx, dy, batch, pairs), x, y)


def _ct_relin(torch, ct, up, key, x, y):
    (batch, pairs), terms = x.shape[:2], up.shape[1]
    return _run(torch, ct.word_bits, (batch, 2, ct.limbs, ct.n),
                lambda out, du, dk, dx, dy: ct.relin_device(out, du, dk, dx, dy, batch, pairs,
                                                            terms), up, key, x, y)


def _compose_moddown(n, q, p, x_hat):
    """forward_Q(ks_moddown(inverse_{Q u P}(x_hat))) with the library's own transforms."""
    Ctx = _hoist_ctx(n)
    with Ctx(n, q + p) as ext, Ctx(n, q) as low, nttmul.KeySwitchBasis(n, q, p, 1) as ks:
        return low.forward(ks.moddown(ext.inverse(x_hat)))


def _compose_modup(n, q, p, alpha, x_hat):
    """forward_{Q u P}(ks_modup(inverse_Q(x_hat))) with the library's own transforms."""
    Ctx = _hoist_ctx(n)
    with Ctx(n, q + p) as ext, Ctx(n, q) as low, nttmul.KeySwitchBasis(n, q, p, alpha) as ks:
        up = ks.modup(low.inverse(x_hat))
        return ext.forward(up.reshape(-1, len(q) + len(p), n)).reshape(up.shape)


class _Plain:
    """One plain context per modulus."""

    def __init__(self, n, moduli):
        self.ctx = [nttmul.Context(n, m) for m in moduli]

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        for c in self.ctx:
            c.close()


# ---------------------------------------------------------------------------------------------
# One test per operation, over the profiles of its word class
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", ("convert", "moddown"))
@pytest.mark.parametrize("profile,n,shape", _cases((SMALL_N, BCONV_N)))
def test_bconv(profile, n, shape, op, torch_cuda):
    """convert Q -> P and moddown from P into Q, against bconv_ref at both n."""
    L, K, _ = shape
    q, p = BC.basis(profile, L, K)
    dt = _dt(BC.bits_of(profile))
    if op == "convert":
        x = B.random_words(_seed(profile, n, L, 0), q, BATCH, n, dt)
        x[0, :, 0] = B.worst_case(q)
        assert np.array_equal(_bconv(torch_cuda, n, q, p, op, x), B.convert(x, q, p))
    else:
        x = B.random_words(_seed(profile, n, L, 1), q + p, BATCH, n, dt)
        x[0, L:, 0] = B.worst_case(p)
        assert np.array_equal(_bconv(torch_cuda, n, p, q, op, x), B.moddown(x, p, q))


@pytest.mark.parametrize("op", ("modup", "moddown"))
@pytest.mark.parametrize("profile,n,shape", _cases((SMALL_N, BIG_N), DIGIT_SHAPES))
def test_ks(profile, n, shape, op, torch_cuda):
    L, K, alpha = shape
    q, p = BC.basis(profile, L, K)
    dt = _dt(BC.bits_of(profile))
    if op == "modup":
        x = B.random_words(_seed(profile, n, L, alpha, 2), q, BATCH, n, dt)
        x[0, :, 0] = ks_ref.worst_case(q, alpha)
        got = _ks(torch_cuda, n, q, p, alpha, op, x)
        assert np.array_equal(got, ks_ref.modup(x, q, p, alpha))
        for d, D in enumerate(ks_ref.digits(L, alpha)):           # own limbs, bit for bit
            assert np.array_equal(got[:, d, D.start:D.stop], x[:, D.start:D.stop])
    else:
        x = B.random_words(_seed(profile, n, L, alpha, 3), q + p, BATCH, n, dt)
        x[0, L:, 0] = B.worst_case(p)
        assert np.array_equal(_ks(torch_cuda, n, q, p, alpha, op, x), B.moddown(x, p, q))


def _sum_mod(rows, m):
    acc = rows[0].astype(object)
    for r in rows[1:]:
        acc = acc + r.astype(object)
    return acc % m


@pytest.mark.parametrize("op", MP_OPS)
@pytest.mark.parametrize("profile", MP_PROFILES)
def test_multi_pass_limb_kernels(profile, op, torch_cuda):
    """n = 8192 over the six limbs of Q u P in the table's order: limb l of every call equals a
    plain context of (n, q_l); the product equals the oracle's too."""
    torch, n, (L, K, _) = torch_cuda, BIG_N, SHAPES[0]
    bits = BC.bits_of(profile)
    m = sum(BC.basis(profile, L, K), ())
    M, dt, rng = len(m), _dt(bits), _seed(profile, MP_OPS.index(op), 4)
    ks = (5, 2 * n - 1)
    a = B.random_words(rng, m * TERMS, BATCH, n, dt).reshape(BATCH, TERMS, M, n)
    b = B.random_words(rng, m * (TERMS * COMPS * len(ks)), 1, n, dt).reshape(
        len(ks), COMPS, TERMS, M, n)
    for l, q in enumerate(m):                                      # the ends of every limb's range
        a[0, 0, l, :2] = (0, q - 1)
        b[0, 0, 0, l, :2] = (q - 1, q - 1)
    with nttmul.RnsMpHoistContext(n, m) as ctx, _Plain(n, m) as plain:
        assert (ctx.limbs, ctx.word_bits) == (M, bits)

        def per_limb(fn, *xs):
            """fn of the plain contexts on [.., M, n] operands, limb by limb."""
            lead = xs[0].shape[:-2]
            out = np.empty(lead + (M, n), dtype=dt)
            for l in range(M):
                args = [np.ascontiguousarray(x[..., l, :]).reshape(-1, n) for x in xs]
                out[..., l, :] = getattr(plain[l], fn)(*args, dtype=dt).reshape(lead + (n,))
            return out

        def sums(x, y):
            """sum_t x[.., t, l] y[.., t, l] mod (x^n + 1, q_l) by plain products: [.., M, n]."""
            prods = per_limb("multiply", x, y)
            out = np.empty(prods.shape[:-3] + (M, n), dtype=dt)
            for l, q in enumerate(m):
                out[..., l, :] = _sum_mod([prods[..., t, l, :] for t in range(TERMS)], q).astype(dt)
            return out

        a0, b0 = a[:, 0], np.ascontiguousarray(np.broadcast_to(b[0, 0, 0], (BATCH, M, n)))
        if op == "multiply":
            got = _run(torch, bits, (BATCH, M, n),
                       lambda out, x, y: ctx.multiply_device(out, x, y, BATCH), a0, b0)
            assert np.array_equal(got, per_limb("multiply", a0, b0))
            for l, q in enumerate(m):
                P = O.Plan(n, q)
                for i in range(BATCH):
                    want = P.product_merged(a0[i, l].astype(np.uint64), b0[i, l].astype(np.uint64))
                    assert np.array_equal(got[i, l].astype(np.uint64), want), (l, i)
        elif op in ("forward", "inverse"):
            got = _run(torch, bits, (BATCH, M, n),
                       lambda out, x: getattr(ctx, f"{op}_device")(out, x, BATCH), a0)
            assert np.array_equal(got, per_limb(op, a0))
        elif op == "mac_ntt":
            b_sh = b[0, 0]                                         # shared: [terms, M, n]
            b_hat = per_limb("forward", b_sh)
            got = _run(torch, bits, (BATCH, M, n),
                       lambda out, x, y: ctx.mac_ntt_device(out, x, y, BATCH, TERMS, shared=True),
                       a, b_hat)
            assert np.array_equal(got, sums(a, np.broadcast_to(b_sh, a.shape)))
        elif op == "macn_ntt":
            b_hat = per_limb("forward", b[0])                      # [comps, terms, M, n]
            got = _run(torch, bits, (BATCH, COMPS, M, n),
                       lambda out, x, y: ctx.macn_ntt_device(out, x, y, BATCH, TERMS, COMPS,
                                                             shared=True), a, b_hat)
            for i in range(COMPS):
                assert np.array_equal(got[:, i], sums(a, np.broadcast_to(b[0, i], a.shape))), i
        else:
            a_hat, b_hat = per_limb("forward", a), per_limb("forward", b)
            got = _run(torch, bits, (BATCH, len(ks), COMPS, M, n),
                       lambda out, x, y: ctx.hoist_ntt_device(out, x, y, ks, BATCH, TERMS, COMPS),
                       a_hat, b_hat)
            for r, k in enumerate(ks):
                ar = galois_ref.coeff(a.reshape(-1, M, n), k, m).reshape(a.shape)
                for i in range(COMPS):
                    want = sums(ar, np.broadcast_to(b[r, i], a.shape))
                    assert np.array_equal(got[:, r, i], want), (k, i)


@pytest.mark.parametrize("profile,n,shape", _cases((SMALL_N, BIG_N)))
def test_mdntt_moddown(profile, n, shape, torch_cuda):
    L, K, _ = shape
    q, p = BC.basis(profile, L, K)
    x = B.random_words(_seed(profile, n, L, 5), q + p, BATCH, n, _dt(BC.bits_of(profile)))
    for l, mod in enumerate(q + p):
        x[0, l, :2] = (0, mod - 1)
    got = _mdntt(torch_cuda, n, q, p, x)
    if n == SMALL_N:
        assert np.array_equal(got, mdntt_ref.moddown(x, q, p))
    else:
        assert np.array_equal(got, _compose_moddown(n, q, p, x))


@pytest.mark.parametrize("profile,n,shape", _cases((SMALL_N, BIG_N), DIGIT_SHAPES))
def test_ksntt_modup(profile, n, shape, torch_cuda):
    L, K, alpha = shape
    q, p = BC.basis(profile, L, K)
    x = B.random_words(_seed(profile, n, L, alpha, 6), q, BATCH, n, _dt(BC.bits_of(profile)))
    got = _ksntt_modup(torch_cuda, n, q, p, alpha, x)
    want = ksntt_ref.modup(x, q, p, alpha) if n == SMALL_N else \
        ksntt_ref.modup_composition(x, q, p, alpha)
    assert np.array_equal(got, want)
    for d, D in enumerate(ks_ref.digits(L, alpha)):               # the own limbs are copies
        assert np.array_equal(got[:, d, D.start:D.stop], x[:, D.start:D.stop])


def _mac_operands(profile, n, shape, ks, salt):
    L, K, _ = shape
    q, p = BC.basis(profile, L, K)
    ext, rng, dt = q + p, _seed(profile, n, L, salt), _dt(BC.bits_of(profile))
    a = B.random_words(rng, ext * TERMS, BATCH, n, dt).reshape(BATCH, TERMS, L + K, n)
    b = B.random_words(rng, ext * (TERMS * COMPS), len(ks), n, dt).reshape(
        len(ks), COMPS, TERMS, L + K, n)
    w = B.random_words(rng, ext, len(ks), n, dt)
    c0 = B.random_words(rng, q, BATCH, n, dt)
    for l, mod in enumerate(ext):
        a[0, 0, l, :2] = b[0, 0, 0, l, :2] = w[0, l, :2] = (mod - 1, mod - 1)
    return q, p, a, b, w, c0


@pytest.mark.parametrize("profile,n,shape", _cases((SMALL_N, BIG_N)))
def test_ksntt_mac(profile, n, shape, torch_cuda):
    ks = (5, 2 * n - 1)
    q, p, a, b, _, _ = _mac_operands(profile, n, shape, ks, 7)
    with nttmul.NttKeySwitch(n, q, p, shape[2]) as kn:
        got = _ksntt_mac(torch_cuda, kn, a, b, ks)
    want = ksntt_ref.mac(a, b, ks, q + p) if n == SMALL_N else \
        ksntt_ref.mac_composition(a, b, ks, q + p)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("profile,n,shape", _cases((SMALL_N, BIG_N)))
def test_lintrans_apply(profile, n, shape, torch_cuda):
    """Weights and c_0 on, comps 2, terms 3, k = (5, 2n - 1)."""
    ks = (5, 2 * n - 1)
    q, p, a, b, w, c0 = _mac_operands(profile, n, shape, ks, 8)
    with nttmul.NttLinTrans(n, q, p) as lt, nttmul.NttKeySwitch(n, q, p, 1) as kn:
        got = _lintrans(torch_cuda, lt, a, b, ks, w, c0)
        want = lintrans_ref.apply(a, b, ks, q, p, w, c0) if n == SMALL_N else \
            lintrans_ref.composition(kn, a, b, ks, q, p, w, c0)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("op", ("high", "relin"))
@pytest.mark.parametrize("profile,n,shape", _cases((SMALL_N, BIG_N)))
def test_ctmul(profile, n, shape, op, pairs, torch_cuda):
    L, K, _ = shape
    q, p = BC.basis(profile, L, K)
    ext, dt = q + p, _dt(BC.bits_of(profile))
    rng = _seed(profile, n, L, pairs, 9)
    up = B.random_words(rng, ext * TERMS, BATCH, n, dt).reshape(BATCH, TERMS, L + K, n)
    key = B.random_words(rng, ext * TERMS, 2, n, dt).reshape(2, TERMS, L + K, n)
    x = B.random_words(rng, q * (2 * pairs), BATCH, n, dt).reshape(BATCH, pairs, 2, L, n)
    y = B.random_words(rng, q * (2 * pairs), BATCH, n, dt).reshape(BATCH, pairs, 2, L, n)
    for l, mod in enumerate(q):
        x[0, :, :, l, :2] = y[0, :, :, l, :2] = mod - 1
    with nttmul.NttCtMul(n, q, p) as ct, _Plain(n, q) as plain, \
            nttmul.NttKeySwitch(n, q, p, 1) as kn:
        if op == "high":
            got = _ct_high(torch_cuda, ct, x, y)
            want = ctmul_ref.high(x, y, q) if n == SMALL_N else \
                ctmul_ref.tensor_composition(plain, x, y, q)[2]
        else:
            got = _ct_relin(torch_cuda, ct, up, key, x, y)
            want = ctmul_ref.relin(up, key, x, y, q, p) if n == SMALL_N else \
                ctmul_ref.composition(kn, plain, up, key, x, y, q, p)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------
# Worst-case fills on the chains and the reversed chains
# ---------------------------------------------------------------------------------------------

def _fill_cases():
    return [pytest.param(p, n, c, id=f"{p}-n{n}-{c}") for bits in (64, 32) for p in BC.CHAINS[bits]
            for n in FILL_N for c in FILL_COUNTS[bits]]


def _filled(values, batch, n, dt):
    x = np.empty((batch, len(values), n), dtype=dt)
    x[:] = np.array(values, dtype=dt)[None, :, None]
    return x


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("op", FILL_OPS)
@pytest.mark.parametrize("profile,n,count", _fill_cases())
def test_worst_case_fills(profile, n, count, op, fill, torch_cuda):
    """`count` limbs are summed: the L limbs of Q for convert and the one digit of the modups, the
    K limbs of P for mdntt_moddown.  worst: every coefficient holds bconv_ref.worst_case /
    ks_ref.worst_case of the profile's bases, every y_i = b_i - 1 under every target modulus.  top:
    every word at its own modulus - 1."""
    torch, dt, batch = torch_cuda, _dt(BC.bits_of(profile)), 2
    if op == "mdntt_moddown":
        q, p = BC.basis(profile, 2, count)
        x = _filled([v - 1 for v in q + p], batch, n, dt)
        if fill == "worst":                                        # the transform of the worst case
            with _hoist_ctx(n)(n, p) as low:
                x[:, 2:] = low.forward(_filled(B.worst_case(p), batch, n, dt))
        got = _mdntt(torch, n, q, p, x)
        want = mdntt_ref.moddown(x, q, p) if n == SMALL_N else _compose_moddown(n, q, p, x)
        assert np.array_equal(got, want)
        return
    q, p = BC.basis(profile, count, 2)
    top = _filled([v - 1 for v in q], batch, n, dt)
    if op == "convert":
        x = _filled(B.worst_case(q), batch, n, dt) if fill == "worst" else top
        got = _bconv(torch, n, q, p, "convert", x)
        assert np.array_equal(got, B.convert(x, q, p))
        if fill == "worst":                                        # alpha = L - 1 at its maximum
            v, Bq = B.crt(B.worst_case(q), q), int(np.prod([int(m) for m in q], dtype=object))
            assert [int(t) for t in got[0, :, 0]] == [(v + (count - 1) * Bq) % c for c in p]
    elif op == "ks_modup":
        x = _filled(ks_ref.worst_case(q, count), batch, n, dt) if fill == "worst" else top
        assert np.array_equal(_ks(torch, n, q, p, count, "modup", x), ks_ref.modup(x, q, p, count))
    else:
        if fill == "worst":
            with _hoist_ctx(n)(n, q) as low:
                x = low.forward(_filled(ks_ref.worst_case(q, count), batch, n, dt))
        else:
            x = top
        got = _ksntt_modup(torch, n, q, p, count, x)
        want = ksntt_ref.modup(x, q, p, count) if n == SMALL_N else \
            _compose_modup(n, q, p, count, x)
        assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------
# The three chains at n = 256, zero-noise keys on the profile's bases
# ---------------------------------------------------------------------------------------------

def _chain_bases(profile):
    L, K, _ = HC.CHAIN_SHAPE
    return BC.basis(profile, L, K)


@pytest.mark.parametrize("profile", CHAIN_PROFILES)
def test_chain_key_switch(profile, torch_cuda):
    """ksntt_modup -> ksntt_mac -> mdntt_moddown on hoist_ref.chain's keys."""
    n, bits = SMALL_N, BC.bits_of(profile)
    ch = H.chain(n, bits, _chain_bases(profile))
    q, p, alpha, ks = ch["q"], ch["p"], ch["alpha"], ch["ks"]
    assert (q, p) == _chain_bases(profile)
    batch, rots, L = ch["x"].shape[0], len(ks), len(q)
    with nttmul.RnsHoistContext(n, q) as low, nttmul.NttKeySwitch(n, q, p, alpha) as kn:
        x_hat = low.forward(ch["x"])
        up_hat = _ksntt_modup(torch_cuda, n, q, p, alpha, x_hat)
        assert np.array_equal(up_hat, ch["up_hat"])
        mid_hat = _ksntt_mac(torch_cuda, kn, up_hat, ch["key_hat"], ks)
        out_hat = _mdntt(torch_cuda, n, q, p, mid_hat.reshape(batch * rots * 2, L + len(p), n))
        back = low.inverse(out_hat).reshape(batch, rots, 2, L, n)
    assert np.array_equal(back, ch["out"])
    errs = H.chain_errors(ch, back)
    print("key switch chain errors", profile, errs, "bound", H.chain_bound())
    assert max(errs) <= H.chain_bound()


@pytest.mark.parametrize("profile", CHAIN_PROFILES)
def test_chain_linear_transform(profile, torch_cuda):
    """ksntt_modup -> lintrans_apply (R = 3, weights and c_0) -> mdntt_moddown."""
    n, bits = SMALL_N, BC.bits_of(profile)
    ch = lintrans_ref.chain(n, bits, _chain_bases(profile))
    q, p, alpha, ks = ch["q"], ch["p"], ch["alpha"], ch["ks"]
    assert len(ks) == 3 and (q, p) == _chain_bases(profile)
    batch, L, M = ch["x"].shape[0], len(q), len(q) + len(p)
    with nttmul.RnsHoistContext(n, q) as low, nttmul.NttLinTrans(n, q, p) as lt:
        up_hat = _ksntt_modup(torch_cuda, n, q, p, alpha, low.forward(ch["x"]))
        assert np.array_equal(up_hat, ch["up_hat"])
        mid = _lintrans(torch_cuda, lt, up_hat, ch["key_hat"], ks, ch["w_hat"], ch["c0_hat"])
        assert np.array_equal(mid, ch["mid_lt"])
        out_hat = _mdntt(torch_cuda, n, q, p, mid.reshape(batch * 2, M, n))
        back = low.inverse(out_hat).reshape(batch, 2, L, n)
    assert np.array_equal(back, ch["out_lt"])
    errs = lintrans_ref.chain_errors(ch, back)
    print("linear transform chain errors", profile, errs, "bound", H.chain_bound())
    assert max(errs) <= H.chain_bound()


@pytest.mark.parametrize("profile", CHAIN_PROFILES)
def test_chain_ciphertext_product(profile, torch_cuda):
    """ctmul_high -> ksntt_modup -> ctmul_relin -> mdntt_moddown, pairs = 1."""
    n, bits = SMALL_N, BC.bits_of(profile)
    ch = ctmul_ref.chain(n, bits, 1, _chain_bases(profile))
    q, p, alpha = ch["q"], ch["p"], ch["alpha"]
    assert (q, p) == _chain_bases(profile)
    batch, L, M = ch["x"].shape[0], len(q), len(q) + len(p)
    with nttmul.RnsHoistContext(n, q) as low, nttmul.NttCtMul(n, q, p) as ct:
        d2_hat = _ct_high(torch_cuda, ct, ch["x_hat"], ch["y_hat"])
        assert np.array_equal(d2_hat, ch["d2_hat"])
        up_hat = _ksntt_modup(torch_cuda, n, q, p, alpha, d2_hat)
        assert np.array_equal(up_hat, ch["up_hat"])
        mid = _ct_relin(torch_cuda, ct, up_hat, ch["key_hat"], ch["x_hat"], ch["y_hat"])
        assert np.array_equal(mid, ch["mid"])
        out_hat = _mdntt(torch_cuda, n, q, p, mid.reshape(batch * 2, M, n))
        out = low.inverse(out_hat).reshape(batch, 2, L, n)
    assert np.array_equal(out, ch["out"])
    errs = ctmul_ref.chain_errors(ch, out, ch["d"])
    print("ciphertext product chain errors", profile, errs, "bound", ctmul_ref.chain_bound())
    assert max(errs) <= ctmul_ref.chain_bound()


# ---------------------------------------------------------------------------------------------
# NTTMUL_FLAG_VALIDATE checks each word against its own limb, whatever the limbs' order
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", VALIDATE_OPS)
@pytest.mark.parametrize("profile", CHAIN_PROFILES)
def test_validate_flag_on_unsorted_limbs(profile, op, torch_cuda):
    """The smallest modulus among the operand's limbs, placed in its own limb, is NTTMUL_ERANGE; the
    same value in the largest limb is in range and the call succeeds."""
    torch, n, (L, K, alpha) = torch_cuda, SMALL_N, SHAPES[0]
    bits = BC.bits_of(profile)
    q, p = BC.basis(profile, L, K)
    ext, dt, rng = q + p, _dt(bits), _seed(profile, 10)
    ks = (5,)

    def call(x):
        """One call with x as its first operand, the flag set."""
        if op == "ks":
            return _ks(torch, n, q, p, alpha, "modup", x, validate=True)
        if op == "mdntt":
            return _mdntt(torch, n, q, p, x, validate=True)
        if op == "ksntt":
            return _ksntt_modup(torch, n, q, p, alpha, x, validate=True)
        if op == "lintrans":
            b = B.random_words(rng, ext * 2, 1, n, dt).reshape(1, 1, 2, L + K, n)
            with nttmul.NttLinTrans(n, q, p, validate=True) as lt:
                return _lintrans(torch, lt, x.reshape(BATCH, 2, L + K, n), b, ks, None, None)
        with nttmul.NttCtMul(n, q, p, validate=True) as ct:
            y = x.reshape(BATCH, 1, 2, L, n)
            return _ct_high(torch, ct, y, y.copy())

    limbs = {"ks": q, "mdntt": ext, "ksntt": q, "lintrans": ext * 2, "ctmul": q * 2}[op]
    good = B.random_words(rng, limbs, BATCH, n, dt)
    small, large = limbs.index(min(limbs)), limbs.index(max(limbs))
    assert limbs[small] < limbs[large]
    call(good)
    bad = good.copy()
    bad[BATCH - 1, small, n - 1] = limbs[small]
    with pytest.raises(nttmul.NttmulError) as ei:
        call(bad)
    assert ei.value.status == nttmul.NTTMUL_ERANGE
    fine = good.copy()
    fine[BATCH - 1, large, n - 1] = limbs[small]
    call(fine)


def test_the_tables_are_whole():
    """Every profile, operation and shape the module runs, counted against basis_cases."""
    assert set(PROFILES) == set(BC.PROFILES) and len(PROFILES) == 5
    assert set(BC.OF_BITS[32]) | set(BC.OF_BITS[64]) == set(PROFILES)
    assert len(_cases((SMALL_N, BIG_N))) == len(BC.PROFILES) * 2 * len(SHAPES)
    assert len(_cases((SMALL_N, BIG_N), DIGIT_SHAPES)) == len(BC.PROFILES) * 2 * len(DIGIT_SHAPES)
    assert len(_fill_cases()) == sum(len(BC.CHAINS[b]) * len(FILL_N) * len(FILL_COUNTS[b])
                                     for b in (32, 64))
    assert set(MP_PROFILES) <= set(PROFILES) and {BC.bits_of(p) for p in MP_PROFILES} == {32, 64}
    assert set(CHAIN_PROFILES) == {BC.CHAINS[32][0], BC.CHAINS[64][0]}
    assert max(max(FILL_COUNTS[64]), SHAPES[0][0]) <= min(BC.MAX_SHAPE)
    for bits, cadence in ((64, 4), (32, 2)):
        assert min(FILL_COUNTS[bits]) < cadence < max(FILL_COUNTS[bits])
