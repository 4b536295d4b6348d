"""GPU parity under full occupancy and past 4 GiB (tests/scale_cases.py).

Every launch of a scale case holds at least 2 * 8192 waves (twice what 256 compute units can hold
at once) and ends in a partial last workgroup where the kernel can have one, so workgroups share
a compute unit, its LDS and its SIMDs, start in slots others have left, and contend for the L2:
the conditions under which a misplaced barrier of an LDS exchange shows.  Inputs are made on the
device, outputs are preset to a sentinel no canonical word equals, and every word of every output
is compared bit for bit.  The code under test is never its own reference:

* libnttmul.so: the whole batch against the CPU oracle (OpenMP over the batch): the fill, forward,
  the pointwise product, inverse, the product, the reordered transform, also in place.
* the limb-aware libraries: the whole output, on the device, against the composition the README
  states as the contract, built from plain contexts of (n, q_l) and torch integer arithmetic; and a
  sample (scale_cases.sample: polynomial 0, the last, the partial last workgroup, the first
  workgroup past 8192 resident waves, one from each 1 / 64 of the batch, at least 256) against the
  oracle or the Python-integer references.
* operands past 2^31 and 2^32 bytes: the same call in chunks whose every operand stays below
  1 GiB, and windows at the start, on both sides of the two offsets and at the end against the
  oracle or the Python-integer references.
"""
import functools
from math import prod

import numpy as np
import pytest

import bconv_ref
import dispatch_cases as D
import galois_ref
import ks_ref
import nttmul
import scale_cases as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FWD = ("mulntt_ct_std2rev", "mixed_powers_rev")          # forward, standard in, bit-reversed out
FWD_REV2STD = ("mulntt_ct_rev2std", "mixed_powers")      # mode 2: bit-reversed in, standard out
INV = ("nttmul_gs_rev2std", "inv_mixed_powers_rev")      # inverse, before the scaling by n^-1
GIB = 1 << 30


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _dt(torch, bits):
    return torch.int32 if bits == 32 else torch.int64


def _sentinel(torch, shape, bits):
    """An output buffer whose every word has all bits set: no modulus here reaches it."""
    return torch.full(shape, -1, dtype=_dt(torch, bits), device="cuda")


def _u64(t, bits):
    """A device tensor as a host uint64 array of the same shape."""
    return t.cpu().numpy().view(np.uint32 if bits == 32 else np.uint64).astype(np.uint64)


def _same(t, bits, want, what):
    """Every word of the device tensor t ([polys, n]) equals the host array want."""
    got = _u64(t, bits).reshape(want.shape)
    bad = np.flatnonzero((got != want).any(axis=-1).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} polynomials differ, first {bad[0]}"


@functools.lru_cache(maxsize=None)
def _plan(n, q):
    return O.Plan(n, q)


def _ofwd(n, q, x):
    return _plan(n, q).transform_batch(FWD[0], x, FWD[1])


def _oinv(n, q, x_hat):
    P = _plan(n, q)
    return P.transform_batch(INV[0], x_hat, INV[1], P.inv_n)


def _omac(n, q, a_hat, b_hat):
    """The oracle's INTT(sum_t a_hat[t] o b_hat[t]) for lists of uint64 [polys, n] arrays."""
    P, acc = _plan(n, q), None
    for x, y in zip(a_hat, b_hat):
        t = P.mul_batch(x, np.broadcast_to(y, x.shape))
        acc = t if acc is None else (acc + t) % np.uint64(q)     # both below 2^62
    return _oinv(n, q, acc)


_PLAIN = {}


def _plain(n, q):
    """A plain context of lib/libnttmul.so, kept for the module."""
    if (n, q) not in _PLAIN:
        _PLAIN[n, q] = nttmul.Context(n, q)
    return _PLAIN[n, q]


@pytest.fixture(scope="module", autouse=True)
def _close_plain_contexts():
    yield
    while _PLAIN:
        _PLAIN.popitem()[1].close()


def _ids(rows):
    def one(s):
        c = s.case
        what = [s.family, getattr(c, "op", ""), str(c.n),
                f"u{getattr(c, 'word_bits', None) or getattr(c, 'bits', None) or S.R.word_bits(c.moduli)}",
                "shared" if getattr(c, "shared", False) and s.family == "mac" else "",
                s.alias.replace("=", ""), "sub" if s.sub else ""]
        return "-".join(w for w in what if w)
    return [one(s) for s in rows]


# ---------------------------------------------------------------------------------------------
# 1. libnttmul.so against the oracle, the whole batch
# ---------------------------------------------------------------------------------------------

def _plain_rows(n, q, w):
    return [s for s in S.rows_of("plain")
            if (s.case.n, s.case.q, s.case.word_bits) == (n, q, w) and not s.sub]


PLAIN_CHAINS = sorted({(s.case.n, s.case.q, s.case.word_bits) for s in S.rows_of("plain")})


def _filled(torch, ctx, n, q, w, batch):
    """a, b from fill_random_device into sentinel buffers, held to the oracle's fill, then with
    every word q - 1 in the first and the last polynomial; and the same as host arrays."""
    a, b = _sentinel(torch, (batch * n,), w), _sentinel(torch, (batch * n,), w)
    ctx.fill_random_device(a, b, 0, batch, w, stream=_stream(torch))
    ea, eb = O.fill_inputs(n, q, 0, batch)
    torch.cuda.synchronize()
    _same(a, w, ea, "fill a")
    _same(b, w, eb, "fill b")
    for t, e in ((a, ea), (b, eb)):
        v = t.view(batch, n)
        v[0], v[-1] = q - 1, q - 1
        e[0], e[-1] = q - 1, q - 1
    return a, b, ea, eb


@pytest.mark.parametrize("n,q,w", PLAIN_CHAINS)
def test_plain_chain_against_the_oracle(n, q, w, torch_cuda):
    """fill, forward, pointwise, inverse and the product of one (n, q, word) at the batch at which
    every one of them meets the rule; forward and inverse also in place.  Every word of every
    result against the oracle's OpenMP loops; operands unchanged; the product's kernels are the
    mirror's."""
    torch, s = torch_cuda, _stream(torch_cuda)
    rows = [r for r in _plain_rows(n, q, w) if r.case.mode != 2]
    batch, = {r.case.batch for r in rows}
    assert {(r.case.op, r.case.mode, r.alias) for r in rows} == {
        ("fill", 0, ""), ("multiply", 0, ""), ("pointwise", 0, ""), ("transform", 0, ""),
        ("transform", 0, "out=in"), ("transform", 3, ""), ("transform", 3, "out=in")}
    ctx = nttmul.Context(n, q)
    P = _plan(n, q)
    a, b, ea, eb = _filled(torch, ctx, n, q, w, batch)
    a0, b0 = a.clone(), b.clone()
    words = (batch * n,)

    fa, fb = _sentinel(torch, words, w), b.clone()
    ctx.forward_device(fa, a, batch, w, stream=s)
    ctx.forward_device(fb, fb, batch, w, stream=s)             # in place
    wa, wb = _ofwd(n, q, ea), _ofwd(n, q, eb)
    torch.cuda.synchronize()
    _same(fa, w, wa, "forward")
    _same(fb, w, wb, "forward in place")
    fa0, fb0 = fa.clone(), fb.clone()

    pw = _sentinel(torch, words, w)
    ctx.pointwise_device(pw, fa, fb, batch, w, stream=s)
    wp = P.mul_batch(wa, wb)
    del wa, wb
    torch.cuda.synchronize()
    _same(pw, w, wp, "pointwise")
    assert torch.equal(fa, fa0) and torch.equal(fb, fb0)
    del fa, fb, fa0, fb0

    c1, c2 = _sentinel(torch, words, w), pw.clone()
    ctx.inverse_device(c1, pw, batch, w, stream=s)
    ctx.inverse_device(c2, c2, batch, w, stream=s)             # in place
    wc = _oinv(n, q, wp)
    torch.cuda.synchronize()
    _same(c1, w, wc, "inverse")
    assert torch.equal(c2, c1), "inverse in place"
    _same(pw, w, wp, "inverse changed its input")
    del wp, pw, c1, c2

    c = _sentinel(torch, words, w)
    ctx.multiply_device(c, a, b, batch, w, stream=s)
    names = [nttmul.dispatch_key(k) for k in ctx.last_kernel_name().split("+")]
    assert names == D.product_keys(D.Case("multiply", n, q, w, batch))
    torch.cuda.synchronize()
    _same(c, w, wc, "product")
    # (the oracle's chain is its product: the reference's own sequence on both ends of the batch)
    for p in (0, batch - 1):
        assert np.array_equal(wc[p], P.product4(ea[p], eb[p]))
    assert torch.equal(a, a0) and torch.equal(b, b0)
    ctx.close()


PLAIN_REORDER = sorted({(s.case.n, s.case.q, s.case.word_bits) for s in S.rows_of("plain")
                        if s.case.mode == 2})


@pytest.mark.parametrize("n,q,w", PLAIN_REORDER)
def test_plain_reordered_transform_against_the_oracle(n, q, w, torch_cuda):
    """Mode 2 (forward, bit-reversed in, standard out: k_bitrev, the transform, k_bitrev_inplace),
    out of place and in place, every word against the oracle's loop of that order."""
    torch, s = torch_cuda, _stream(torch_cuda)
    rows = [r for r in _plain_rows(n, q, w) if r.case.mode == 2]
    batch, = {r.case.batch for r in rows}
    assert {r.alias for r in rows} == {"", "out=in"}
    ctx = nttmul.Context(n, q)
    a, b, ea, _ = _filled(torch, ctx, n, q, w, batch)
    a0 = a.clone()
    out = _sentinel(torch, (batch * n,), w)
    ctx.transform_device(out, a, nttmul.XF_REV2STD, batch, w, stream=s)
    b.copy_(a)                                                 # b: the buffer of the in-place call
    ctx.transform_device(b, b, nttmul.XF_REV2STD, batch, w, stream=s)
    want = _plan(n, q).transform_batch(FWD_REV2STD[0], ea, FWD_REV2STD[1])
    torch.cuda.synchronize()
    _same(out, w, want, "mode 2")
    assert torch.equal(b, out), "mode 2 in place"
    assert torch.equal(a, a0)
    ctx.close()


def test_plain_product_in_three_sub_batches(torch_cuda):
    """A multi-pass product whose lowered scratch_mb splits it into three sub-batches, the first
    two of which meet the rule on their own: every product against the oracle."""
    torch, st = torch_cuda, _stream(torch_cuda)
    s, = [r for r in S.rows_of("plain") if r.sub]
    c = s.case
    assert len(S.sub_batches(s)) == 3
    ctx = nttmul.Context(c.n, c.q, scratch_mb=s.sub)
    a, b, ea, eb = _filled(torch, ctx, c.n, c.q, c.word_bits, c.batch)
    a0, b0 = a.clone(), b.clone()
    out = _sentinel(torch, (c.batch * c.n,), c.word_bits)
    ctx.multiply_device(out, a, b, c.batch, c.word_bits, stream=st)
    want = _plan(c.n, c.q).fast_batch_u32(ea.astype(np.uint32), eb.astype(np.uint32))[0]
    torch.cuda.synchronize()
    _same(out, c.word_bits, want.astype(np.uint64), "product in sub-batches")
    assert torch.equal(a, a0) and torch.equal(b, b0)
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 2. the limb-aware libraries: compositions on the device, samples on the host
# ---------------------------------------------------------------------------------------------

def _rand(torch, polys, moduli, n, bits, seed):
    """[polys, limbs, n] canonical words, limb l below moduli[l] from a seeded torch.randint;
    every word q_l - 1 in the first and the last polynomial."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((polys, len(moduli), n), dtype=_dt(torch, bits), device="cuda")
    for l, q in enumerate(moduli):
        x[:, l, :] = torch.randint(0, q, (polys, n), generator=gen, device="cuda",
                                   dtype=torch.int64).to(x.dtype)
        x[0, l, :] = q - 1
        x[-1, l, :] = q - 1
    return x


def _addmod(torch, x, y, q):
    """x + y mod q for canonical tensors, without leaving the word (q < 2^62 or q < 2^31)."""
    d = x - (q - y)
    return torch.where(d < 0, d + q, d)


def _mulmod_const(torch, x, k, q):
    """x * k mod q for an int64 tensor x >= 0 and a Python integer 0 <= k < q: one product where
    it fits 64 bits, else double-and-add over the bits of k (sums stay below 2^63)."""
    x = x % q
    if q < (1 << 31):
        return (x * k) % q
    acc = torch.zeros_like(x)
    for bit in bin(k)[2:]:
        acc = _addmod(torch, acc, acc, q)
        if bit == "1":
            acc = _addmod(torch, acc, x, q)
    return acc


def _plain_unary(torch, op, n, q, bits, x):
    """forward / inverse of a plain context on a [polys, n] tensor of one limb."""
    x = x.contiguous()
    out = torch.empty_like(x)
    getattr(_plain(n, q), op + "_device")(out, x, x.shape[0], bits, stream=_stream(torch))
    return out


def _plain_mac(torch, n, q, bits, a_hat, b_hat):
    """INTT(sum_t a_hat[t] o b_hat[t]) by a plain context of (n, q): pointwise products summed in
    torch, one inverse; a_hat[t], b_hat[t]: [polys, n] tensors of one limb."""
    ctx, s, acc = _plain(n, q), _stream(torch), None
    for x, y in zip(a_hat, b_hat):
        x, y = x.contiguous(), y.expand_as(x).contiguous()
        t = torch.empty_like(x)
        ctx.pointwise_device(t, x, y, x.shape[0], bits, stream=s)
        acc = t if acc is None else _addmod(torch, acc, t, q)
    return _plain_unary(torch, "inverse", n, q, bits, acc)


def _take(t, idx, bits):
    """Rows idx of a device tensor as a host uint64 array."""
    return _u64(t[idx], bits)


def _sample(torch, s):
    polys = S.sample(S.launches(s), S.batch_of(s))
    return polys, torch.tensor(polys, device="cuda")


def _limb_ctx(family, n, moduli, scratch_mb=0):
    lib = {"rns": "Rns", "macn": "RnsMacn", "hoist": "RnsHoist"}[family]
    if n <= 4096:
        return getattr(nttmul, lib + "Context")(n, moduli)
    return getattr(nttmul, lib.replace("Rns", "RnsMp") + "Context")(n, moduli, scratch_mb=scratch_mb)


RNS_ROWS = S.rows_of("rns") + S.rows_of("rnsmp")


@pytest.mark.parametrize("s", RNS_ROWS, ids=_ids(RNS_ROWS))
def test_rns_calls_equal_plain_contexts_per_limb(s, torch_cuda):
    """nttmul_rns_* / nttmul_rnsmp_*: limb l of the whole output equals a plain context of
    (n, q_l); the sample equals the oracle."""
    torch, st, c = torch_cuda, _stream(torch_cuda), s.case
    n, moduli, batch, bits = c.n, c.moduli, c.batch, S.R.word_bits(c.moduli)
    L, terms = len(moduli), c.terms
    mirror = S.R.rns_kernel if s.family == "rns" else S.M.kernel_name
    ctx = _limb_ctx("rns", n, moduli, c.scratch_mb if s.family == "rnsmp" else 0)
    assert ctx.kernel_name(c.op) == mirror(c.op, n, moduli)
    polys, idx = _sample(torch, s)
    out = _sentinel(torch, (batch, L, n), bits)
    if c.op in ("forward", "inverse"):
        x = _rand(torch, batch, moduli, n, bits, 1)
        x0 = x.clone()
        getattr(ctx, c.op + "_device")(out, x, batch, stream=st)
        ofn = _ofwd if c.op == "forward" else _oinv
        for l, q in enumerate(moduli):
            assert torch.equal(out[:, l], _plain_unary(torch, c.op, n, q, bits, x[:, l])), (c.op, l)
            got, want = _take(out[:, l], idx, bits), ofn(n, q, _take(x[:, l], idx, bits))
            assert S.mismatching(got, want, polys) == [], l
        assert torch.equal(x, x0)
    elif c.op == "multiply":
        a, b = _rand(torch, batch, moduli, n, bits, 2), _rand(torch, batch, moduli, n, bits, 3)
        a0, b0 = a.clone(), b.clone()
        ctx.multiply_device(out, a, b, batch, stream=st)
        for l, q in enumerate(moduli):
            al, bl = a[:, l].contiguous(), b[:, l].contiguous()
            want = torch.empty_like(al)
            _plain(n, q).multiply_device(want, al, bl, batch, bits, stream=st)
            assert torch.equal(out[:, l], want), l
            want = _omac(n, q, [_ofwd(n, q, _take(al, idx, bits))], [_ofwd(n, q, _take(bl, idx, bits))])
            assert S.mismatching(_take(out[:, l], idx, bits), want, polys) == [], l
        assert torch.equal(a, a0) and torch.equal(b, b0)
    else:
        a = _rand(torch, batch * terms, moduli, n, bits, 4).view(batch, terms, L, n)
        bh = _rand(torch, batch * terms, moduli, n, bits, 5).view(batch, terms, L, n)
        a0, b0 = a.clone(), bh.clone()
        ctx.mac_ntt_device(out, a, bh, batch, terms, stream=st)
        for l, q in enumerate(moduli):
            ah = [_plain_unary(torch, "forward", n, q, bits, a[:, t, l]) for t in range(terms)]
            want = _plain_mac(torch, n, q, bits, ah, [bh[:, t, l] for t in range(terms)])
            assert torch.equal(out[:, l], want), l
            want = _omac(n, q, [_ofwd(n, q, _take(a[:, t, l], idx, bits)) for t in range(terms)],
                         [_take(bh[:, t, l], idx, bits) for t in range(terms)])
            assert S.mismatching(_take(out[:, l], idx, bits), want, polys) == [], l
        assert torch.equal(a, a0) and torch.equal(bh, b0)
    torch.cuda.synchronize()
    ctx.close()


MAC_ROWS = S.rows_of("mac")


@pytest.mark.parametrize("s", MAC_ROWS, ids=_ids(MAC_ROWS))
def test_mac_equals_the_plain_composition(s, torch_cuda):
    """nttmul_mac_ntt_device (k_mac), terms = 3, shared and per-batch b_hat: the whole output
    equals INTT(sum_t NTT(a_t) o b_hat_t) built from the plain calls; the sample equals the
    oracle."""
    torch, st, c = torch_cuda, _stream(torch_cuda), s.case
    n, q, bits, batch, terms = c.n, c.q, c.word_bits, c.batch, c.terms
    ctx = nttmul.MacContext(n, q)
    assert ctx.mac_kernel_name(bits) == S.MC.mac_kernel(n, q, bits)
    polys, idx = _sample(torch, s)
    a = _rand(torch, batch * terms, (q,), n, bits, 6).view(batch, terms, n)
    bh = _rand(torch, (1 if c.shared else batch) * terms, (q,), n, bits, 7).view(-1, terms, n)
    a0, b0 = a.clone(), bh.clone()
    out = _sentinel(torch, (batch, n), bits)
    ctx.mac_ntt_device(out, a, bh, batch, terms, bits, shared=c.shared, stream=st)
    ah = [_plain_unary(torch, "forward", n, q, bits, a[:, t]) for t in range(terms)]
    assert torch.equal(out, _plain_mac(torch, n, q, bits, ah, [bh[:, t] for t in range(terms)]))
    bs = [_u64(bh[0, t], bits) if c.shared else _take(bh[:, t], idx, bits) for t in range(terms)]
    want = _omac(n, q, [_ofwd(n, q, _take(a[:, t], idx, bits)) for t in range(terms)], bs)
    assert S.mismatching(_take(out, idx, bits), want, polys) == []
    assert torch.equal(a, a0) and torch.equal(bh, b0)
    ctx.close()


MACN_ROWS = S.rows_of("macn")


@pytest.mark.parametrize("s", MACN_ROWS, ids=_ids(MACN_ROWS))
def test_macn_equals_the_plain_composition(s, torch_cuda):
    """macn_ntt with comps = 2, terms = 3 and a shared b_hat, both families: component i of limb l
    equals INTT(sum_t NTT(a_t) o b_hat[i][t]) from a plain context of (n, q_l); the sample equals
    the oracle."""
    torch, st, c = torch_cuda, _stream(torch_cuda), s.case
    n, moduli, batch, bits = c.n, c.moduli, c.batch, S.R.word_bits(c.moduli)
    L, terms, comps = len(moduli), c.terms, c.comps
    ctx = _limb_ctx("macn", n, moduli, c.scratch_mb)
    assert ctx.macn_kernel_name(comps) == S.N.kernel_name(n, moduli, comps)
    polys, idx = _sample(torch, s)
    a = _rand(torch, batch * terms, moduli, n, bits, 8).view(batch, terms, L, n)
    bh = _rand(torch, comps * terms, moduli, n, bits, 9).view(comps, terms, L, n)
    a0, b0 = a.clone(), bh.clone()
    out = _sentinel(torch, (batch, comps, L, n), bits)
    ctx.macn_ntt_device(out, a, bh, batch, terms, comps, shared=True, stream=st)
    for l, q in enumerate(moduli):
        ah = [_plain_unary(torch, "forward", n, q, bits, a[:, t, l]) for t in range(terms)]
        oh = [_ofwd(n, q, _take(a[:, t, l], idx, bits)) for t in range(terms)]
        for i in range(comps):
            want = _plain_mac(torch, n, q, bits, ah, [bh[i, t, l] for t in range(terms)])
            assert torch.equal(out[:, i, l], want), (l, i)
            want = _omac(n, q, oh, [_u64(bh[i, t, l], bits) for t in range(terms)])
            assert S.mismatching(_take(out[:, i, l], idx, bits), want, polys) == [], (l, i)
    assert torch.equal(a, a0) and torch.equal(bh, b0)
    ctx.close()


HOIST_ROWS = S.rows_of("hoist")


@pytest.mark.parametrize("s", HOIST_ROWS, ids=_ids(HOIST_ROWS))
def test_hoist_equals_the_plain_composition(s, torch_cuda):
    """hoist_ntt with three rotations, comps = 2, terms = 3, both families: result (r, i) of limb
    l equals INTT(sum_t sigma_{k_r}(a_hat_t) o b_hat[r][i][t]) with the NTT-order permutation from
    tests/galois_ref.py as a torch index_select and the plain calls of (n, q_l); the sample equals
    the oracle on the same permutation."""
    torch, st, c = torch_cuda, _stream(torch_cuda), s.case
    n, moduli, batch, bits = c.n, c.moduli, c.batch, S.R.word_bits(c.moduli)
    L, terms, comps, rots = len(moduli), c.terms, c.comps, len(c.ks)
    ctx = _limb_ctx("hoist", n, moduli, c.scratch_mb)
    assert ctx.hoist_kernel_name(comps) == S.H.kernel_name(n, moduli, comps)
    polys, idx = _sample(torch, s)
    ah = _rand(torch, batch * terms, moduli, n, bits, 10).view(batch, terms, L, n)
    bh = _rand(torch, rots * comps * terms, moduli, n, bits, 11).view(rots, comps, terms, L, n)
    a0, b0 = ah.clone(), bh.clone()
    out = _sentinel(torch, (batch, rots, comps, L, n), bits)
    ctx.hoist_ntt_device(out, ah, bh, c.ks, batch, terms, comps, stream=st)
    for r, k in enumerate(c.ks):
        src = galois_ref.np_tables(n, int(k))[2]
        src_t = torch.from_numpy(src).cuda()
        for l, q in enumerate(moduli):
            rot = [torch.index_select(ah[:, t, l], 1, src_t) for t in range(terms)]
            orot = [_take(ah[:, t, l], idx, bits)[:, src] for t in range(terms)]
            for i in range(comps):
                want = _plain_mac(torch, n, q, bits, rot, [bh[r, i, t, l] for t in range(terms)])
                assert torch.equal(out[:, r, i, l], want), (r, l, i)
                want = _omac(n, q, orot, [_u64(bh[r, i, t, l], bits) for t in range(terms)])
                assert S.mismatching(_take(out[:, r, i, l], idx, bits), want, polys) == [], (r, l, i)
    assert torch.equal(ah, a0) and torch.equal(bh, b0)
    ctx.close()


def _torch_convert(torch, x, from_q, to_q):
    """The header's conversion in int64 tensors: y_i = x_i (B / b_i)^-1 mod b_i, then for every
    target c_j the sum over i of y_i (B / b_i mod c_j) mod c_j; x: [polys, L, n]."""
    B = prod(from_q)
    ys = [_mulmod_const(torch, x[:, i].to(torch.int64), pow(B // b, -1, b), b)
          for i, b in enumerate(from_q)]
    out = []
    for c in to_q:
        acc = None
        for y, b in zip(ys, from_q):
            t = _mulmod_const(torch, y, (B // b) % c, c)
            acc = t if acc is None else _addmod(torch, acc, t, c)
        out.append(acc)
    return torch.stack(out, dim=1)


def _torch_moddown(torch, x, from_q, to_q):
    """(x_j - convert(x's from_q limbs)_j) B^-1 mod c_j; x: [polys, K + L, n], to_q's limbs first."""
    K, B = len(to_q), prod(from_q)
    conv = _torch_convert(torch, x[:, K:], from_q, to_q)
    out = []
    for j, c in enumerate(to_q):
        d = _addmod(torch, x[:, j].to(torch.int64), c - conv[:, j], c) % c
        out.append(_mulmod_const(torch, d, pow(B, -1, c), c))
    return torch.stack(out, dim=1)


BCONV_ROWS = S.rows_of("bconv")


@pytest.mark.parametrize("s", BCONV_ROWS, ids=_ids(BCONV_ROWS))
def test_bconv_equals_the_torch_composition(s, torch_cuda):
    """convert and moddown with (L, K) = (4, 5): the whole output equals the header's formula in
    int64 tensors; the sample equals tests/bconv_ref.py in Python integers."""
    torch, st, c = torch_cuda, _stream(torch_cuda), s.case
    from_q, to_q = S.B.bases(c.bits, c.L, c.K)
    conv = nttmul.BaseConverter(c.n, from_q, to_q)
    assert conv.kernel_name(c.op) == S.B.bconv_kernel(c.op, c.n, c.bits)
    polys, idx = _sample(torch, s)
    moduli = from_q if c.op == "convert" else to_q + from_q
    x = _rand(torch, c.batch, moduli, c.n, c.bits, 12)
    x0 = x.clone()
    out = _sentinel(torch, (c.batch, c.K, c.n), c.bits)
    getattr(conv, c.op + "_device")(out, x, c.batch, stream=st)
    compose = _torch_convert if c.op == "convert" else _torch_moddown
    assert torch.equal(out.to(torch.int64), compose(torch, x, from_q, to_q))
    want = getattr(bconv_ref, c.op)(_take(x, idx, c.bits), from_q, to_q)
    assert S.mismatching(_take(out, idx, c.bits), want, polys) == []
    assert torch.equal(x, x0)
    conv.close()


KS_ROWS = S.rows_of("ks")


@pytest.mark.parametrize("s", KS_ROWS, ids=_ids(KS_ROWS))
def test_ks_equals_the_torch_composition(s, torch_cuda):
    """modup and moddown with (L, K, alpha) = (4, 2, 2): modup's digit d equals the conversion of
    the digit's limbs to every modulus of Q u P, moddown the conversion from P to Q, in int64
    tensors; the sample equals tests/ks_ref.py and bconv_ref.py in Python integers."""
    torch, st, c = torch_cuda, _stream(torch_cuda), s.case
    q, p = S.K.moduli_of(c)
    ext = q + p
    ks = nttmul.KeySwitchBasis(c.n, q, p, c.alpha)
    assert ks.kernel_name(c.op) == S.K.kernel_name(c.op, c.n, c.bits)
    polys, idx = _sample(torch, s)
    if c.op == "modup":
        x = _rand(torch, c.batch, q, c.n, c.bits, 13)
        out = _sentinel(torch, (c.batch, S.K.dnum(c), len(ext), c.n), c.bits)
    else:
        x = _rand(torch, c.batch, ext, c.n, c.bits, 14)
        out = _sentinel(torch, (c.batch, c.L, c.n), c.bits)
    x0 = x.clone()
    getattr(ks, c.op + "_device")(out, x, c.batch, stream=st)
    if c.op == "modup":
        for d, dig in enumerate(ks_ref.digits(c.L, c.alpha)):
            want = _torch_convert(torch, x[:, dig.start:dig.stop], [q[i] for i in dig], ext)
            assert torch.equal(out[:, d].to(torch.int64), want), d
        want = ks_ref.modup(_take(x, idx, c.bits), q, p, c.alpha)
    else:
        assert torch.equal(out.to(torch.int64), _torch_moddown(torch, x, p, q))
        want = bconv_ref.moddown(_take(x, idx, c.bits), p, q)
    assert S.mismatching(_take(out, idx, c.bits), want, polys) == []
    assert torch.equal(x, x0)
    ks.close()


def _torch_coeff(torch, x, k, moduli):
    """sigma_k in coefficient order as index_select and a negation per limb; x: [polys, L, n]."""
    src, neg, _ = galois_ref.np_tables(x.shape[-1], int(k))
    g = torch.index_select(x, 2, torch.from_numpy(src).to(x.device))
    q = torch.tensor(moduli, dtype=torch.int64, device=x.device).to(x.dtype).reshape(1, -1, 1)
    return torch.where(torch.from_numpy(neg).to(x.device).reshape(1, 1, -1), (q - g) % q, g)


def _torch_ntt(torch, x, k):
    hat = galois_ref.np_tables(x.shape[-1], int(k))[2]
    return torch.index_select(x, 2, torch.from_numpy(hat).to(x.device))


GALOIS_ROWS = S.rows_of("galois")


@pytest.mark.parametrize("s", GALOIS_ROWS, ids=_ids(GALOIS_ROWS))
def test_galois_equals_the_torch_composition(s, torch_cuda):
    """coeff, ntt and ntt_many (four automorphisms): the whole output equals an index_select with
    the tables of tests/galois_ref.py (and the negation where(neg, q - x, x) in coefficient
    order); the sample equals galois_ref's own functions.  coeff at n = 65536 (and 32768 on 64-bit
    words) stages a polynomial in two and four residue classes by sibling workgroups."""
    torch, st, c = torch_cuda, _stream(torch_cuda), s.case
    n, moduli, batch, bits = c.n, c.moduli, c.batch, S.G.word_bits(c.moduli)
    gal = nttmul.GaloisContext(n, moduli)
    assert gal.kernel_name(c.op, len(c.ks)) == S.G.kernel_name(c.op, n, moduli)
    polys, idx = _sample(torch, s)
    x = _rand(torch, batch, moduli, n, bits, 15)
    x[batch // 2] = 0                                          # -0 = 0
    x0 = x.clone()
    xs = _take(x, idx, bits)
    if c.op == "ntt_many":
        out = _sentinel(torch, (len(c.ks), batch, len(moduli), n), bits)
        gal.ntt_many_device(out, x, c.ks, batch, stream=st)
        for i, k in enumerate(c.ks):
            assert torch.equal(out[i], _torch_ntt(torch, x, k)), k
            assert S.mismatching(_take(out[i], idx, bits), galois_ref.ntt(xs, int(k)), polys) == []
    else:
        k, = c.ks
        out = _sentinel(torch, (batch, len(moduli), n), bits)
        getattr(gal, c.op + "_device")(out, x, k, batch, stream=st)
        if c.op == "coeff":
            assert torch.equal(out, _torch_coeff(torch, x, k, moduli))
            want = galois_ref.coeff(xs, int(k), moduli)
        else:
            assert torch.equal(out, _torch_ntt(torch, x, k))
            want = galois_ref.ntt(xs, int(k))
        assert S.mismatching(_take(out, idx, bits), want, polys) == []
    assert torch.equal(x, x0)
    gal.close()


# ---------------------------------------------------------------------------------------------
# 3. operands past 2^31 and 2^32 bytes
# ---------------------------------------------------------------------------------------------

WINDOW = 64


def _need(torch, nbytes, what):
    free, _ = torch.cuda.mem_get_info()
    if free < 1.5 * nbytes:
        pytest.skip(f"{what}: {free / GIB:.1f} GiB free, the buffers take {nbytes / GIB:.1f} GiB "
                    f"and the test asks for 1.5 times that")


def _windows(entries, entry_bytes, per=1):
    """The batch entries of the windows: WINDOW output polynomials (`per` to an entry) at the
    start, on each side of byte offsets 2^31 and 2^32 of an operand of entry_bytes per entry, and
    at the end; sorted, within the batch."""
    w = -(-WINDOW // per)
    out = set(range(w)) | set(range(entries - w, entries))
    for off in (1 << 31, 1 << 32):
        e = off // entry_bytes                   # the entry that holds (or follows) the offset
        out |= set(range(e - w, e + w + 1))
    return sorted(e for e in out if 0 <= e < entries)


def test_plain_product_past_4_gib(torch_cuda):
    """The u32 product at n = 4096 with batch 2^18 + 3: each operand is just over 4 GiB, so
    k_rows' per-polynomial descriptors are built past byte offsets 2^31 and 2^32.  Against the
    same call in chunks below 1 GiB per operand, and against the oracle on the windows."""
    torch, s = torch_cuda, _stream(torch_cuda)
    n, q, w, batch = 4096, D.Q31, 32, (1 << 18) + 3
    poly = n * 4
    assert batch * poly > 1 << 32
    chunk = GIB // poly - 1
    _need(torch, (3 * batch + chunk) * poly, "plain product past 4 GiB")
    ctx = nttmul.Context(n, q)
    a = torch.empty(batch * n, dtype=torch.int32, device="cuda")
    b = torch.empty_like(a)
    c = _sentinel(torch, (batch * n,), w)
    ctx.fill_random_device(a, b, 0, batch, w, stream=s)
    ctx.multiply_device(c, a, b, batch, w, stream=s)
    part = _sentinel(torch, (chunk * n,), w)
    for p0 in range(0, batch, chunk):
        cnt = min(chunk, batch - p0)
        sl = slice(p0 * n, (p0 + cnt) * n)
        ctx.multiply_device(part, a[sl], b[sl], cnt, w, stream=s)
        assert torch.equal(c[sl], part[:cnt * n]), p0
    P = _plan(n, q)
    cv = c.view(batch, n)
    ws = _windows(batch, poly)
    assert ws[0] == 0 and ws[-1] == batch - 1 and {(1 << 31) // poly - 1, (1 << 31) // poly,
                                                   (1 << 32) // poly - 1, (1 << 32) // poly} <= set(ws)
    runs = np.split(np.array(ws), np.flatnonzero(np.diff(ws) > 1) + 1)
    for run in runs:
        ea, eb = O.fill_inputs(n, q, int(run[0]), len(run))
        want = P.fast_batch_u32(ea.astype(np.uint32), eb.astype(np.uint32))[0].astype(np.uint64)
        got = _u64(cv[int(run[0]):int(run[-1]) + 1], w)
        assert S.mismatching(got, want, list(run)) == []
    ctx.close()


def _hoist_rotations(n, rots):
    ks = [2 * n - 1] + [pow(5, e, 2 * n) for e in range(1, rots)]
    assert len(set(ks)) == rots
    return ks


def test_hoist_output_past_4_gib(torch_cuda):
    """nttmul_rns_hoist_ntt at n = 4096, L = 3, 32-bit words, 16 rotations, comps = 2, terms = 2,
    batch 2732: c is just over 4 GiB from a 270 MB a_hat.  Against the same call in chunks whose
    c stays below 1 GiB, and against the oracle on the windows of c."""
    torch, st = torch_cuda, _stream(torch_cuda)
    n, moduli, bits, rots, comps, terms, batch = 4096, S.R.BASIS32, 32, 16, 2, 2, 2731 + 1
    L = len(moduli)
    entry = rots * comps * L * n * 4             # bytes of c per batch entry
    assert batch * entry > 1 << 32
    chunk = GIB // entry - 1
    _need(torch, (batch + chunk) * entry + 2 * batch * terms * L * n * 4, "hoist past 4 GiB")
    ks = _hoist_rotations(n, rots)
    ctx = nttmul.RnsHoistContext(n, moduli)
    ah = _rand(torch, batch * terms, moduli, n, bits, 16).view(batch, terms, L, n)
    bh = _rand(torch, rots * comps * terms, moduli, n, bits, 17).view(rots, comps, terms, L, n)
    c = _sentinel(torch, (batch, rots, comps, L, n), bits)
    ctx.hoist_ntt_device(c, ah, bh, ks, batch, terms, comps, stream=st)
    part = _sentinel(torch, (chunk, rots, comps, L, n), bits)
    for p0 in range(0, batch, chunk):
        cnt = min(chunk, batch - p0)
        ctx.hoist_ntt_device(part, ah[p0:p0 + cnt], bh, ks, cnt, terms, comps, stream=st)
        assert torch.equal(c[p0:p0 + cnt], part[:cnt]), p0
    ws = _windows(batch, entry, rots * comps)
    idx = torch.tensor(ws, device="cuda")
    for r, k in enumerate(ks):
        src = galois_ref.np_tables(n, int(k))[2]
        for l, q in enumerate(moduli):
            rot = [_take(ah[:, t, l], idx, bits)[:, src] for t in range(terms)]
            for i in range(comps):
                want = _omac(n, q, rot, [_u64(bh[r, i, t, l], bits) for t in range(terms)])
                assert S.mismatching(_take(c[:, r, i, l], idx, bits), want, ws) == [], (r, l, i)
    ctx.close()


def test_galois_ntt_many_output_past_4_gib(torch_cuda):
    """galois_ntt_many with 16 automorphisms at n = 4096, L = 3, 32-bit words: the input is just
    over 256 MiB, the output just over 4 GiB.  Against the same call in chunks whose output stays
    below 1 GiB, and against tests/galois_ref.py on the windows of the output."""
    torch, st = torch_cuda, _stream(torch_cuda)
    n, moduli, bits, count = 4096, S.M.BASIS32, 32, 16
    L = len(moduli)
    entry = L * n * 4
    batch = (256 << 20) // entry + 1
    assert batch * entry > 256 << 20 and count * batch * entry > 1 << 32
    chunk = GIB // (count * entry) - 1
    _need(torch, (count + 2) * batch * entry + count * chunk * entry, "galois_ntt_many past 4 GiB")
    ks = S.G.many_ks(n, count)
    gal = nttmul.GaloisContext(n, moduli)
    x = _rand(torch, batch, moduli, n, bits, 18)
    out = _sentinel(torch, (count, batch, L, n), bits)
    gal.ntt_many_device(out, x, ks, batch, stream=st)
    part = _sentinel(torch, (count, chunk, L, n), bits)
    for p0 in range(0, batch, chunk):
        cnt = min(chunk, batch - p0)
        pv = part.view(-1)[:count * cnt * L * n].view(count, cnt, L, n)
        gal.ntt_many_device(pv, x[p0:p0 + cnt], ks, cnt, stream=st)
        assert torch.equal(out[:, p0:p0 + cnt], pv), p0
    flat = out.view(count * batch, L, n)
    ws = _windows(count * batch, entry)
    got = _take(flat, torch.tensor(ws, device="cuda"), bits)
    xs = _u64(x, bits)
    for j, e in enumerate(ws):
        i, p = divmod(e, batch)
        assert np.array_equal(got[j], galois_ref.ntt(xs[p:p + 1], int(ks[i]))[0]), (i, p)
    gal.close()


def test_ks_modup_output_past_4_gib(torch_cuda):
    """ks_modup with (L, K, alpha) = (4, 2, 1) at n = 4096 on 32-bit words: six output words per
    input word, the output just over 4 GiB.  Against the same call in chunks whose output stays
    below 1 GiB, and against tests/ks_ref.py on the windows of the output."""
    torch, st = torch_cuda, _stream(torch_cuda)
    n, bits, L, K, alpha = 4096, 32, 4, 2, 1
    q, p = ks_ref.bases(bits, L, K)
    per = L * (L + K)                            # output polynomials per batch entry
    entry = per * n * 4
    batch = (1 << 32) // entry + 1
    assert batch * entry > 1 << 32
    chunk = GIB // entry - 1
    _need(torch, (batch + chunk) * entry + 2 * batch * L * n * 4, "ks_modup past 4 GiB")
    ks = nttmul.KeySwitchBasis(n, q, p, alpha)
    x = _rand(torch, batch, q, n, bits, 19)
    out = _sentinel(torch, (batch, L, L + K, n), bits)
    ks.modup_device(out, x, batch, stream=st)
    part = _sentinel(torch, (chunk, L, L + K, n), bits)
    for p0 in range(0, batch, chunk):
        cnt = min(chunk, batch - p0)
        ks.modup_device(part, x[p0:p0 + cnt], cnt, stream=st)
        assert torch.equal(out[p0:p0 + cnt], part[:cnt]), p0
    ws = _windows(batch, entry, per)
    idx = torch.tensor(ws, device="cuda")
    want = ks_ref.modup(_take(x, idx, bits), q, p, alpha)
    assert S.mismatching(_take(out, idx, bits), want, ws) == []
    ks.close()
