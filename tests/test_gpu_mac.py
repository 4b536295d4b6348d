"""GPU parity of products and dot products against NTT-domain operands (include/nttmul_mac.h,
lib/libnttmul_mac.so, csrc/mac_dev.hpp k_mac).

    c[p] = INTT( sum_t NTT(a[p][t]) o b_hat[shared ? 0 : p][t] )

Everything is bit-exact: against the CPU oracle's products summed in Python integers, and, for
operands no product produces (every word q - 1, arbitrary canonical b_hat), against the library's
own forward / pointwise / inverse calls with the sum on the host.  Shapes are the smallest at
which the kernel can go wrong: every n has its own register layouts and exchanges, and batch 17
leaves a partial last block at each (tests/mac_cases.py)."""
import functools

import numpy as np
import pytest

import dispatch_cases as D
import guarded as G
import mac_cases as M
import nttmul
from oracle import oracle as O
from test_gpu_parity import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _to_dev(torch, x, bits):
    x = np.ascontiguousarray(x, dtype=_dt(bits))
    return torch.from_numpy(x.view(np.int32 if bits == 32 else np.int64).reshape(-1)).cuda()


def _mac_device(torch, ctx, a, b_hat, shared, bits, stream=0):
    """One nttmul_mac_ntt_device call on numpy operands, out of a guarded arena
    (tests/guarded.py: every operand between sentinel guards, aligned to its word only; after the
    call no guard word and no input word has changed and every word of c is written); returns
    (c, a after, b_hat after)."""
    batch, terms, n = a.shape
    arena = G.DeviceArena(torch, bits, G.guard_words(terms * n), c=batch * n, a=a, b_hat=b_hat)
    dc, da, db = arena["c"], arena["a"], arena["b_hat"]
    ctx.mac_ntt_device(dc, da, db, batch, terms, bits, shared=shared, stream=stream)
    torch.cuda.synchronize()
    arena.check()
    return tuple(arena.get(k, shape).astype(np.uint64)
                 for k, shape in (("c", (batch, n)), ("a", a.shape), ("b_hat", b_hat.shape)))


def _sum_mod(rows, q):
    """sum of uint64 arrays mod q, in Python integers."""
    acc = rows[0].astype(object)
    for r in rows[1:]:
        acc = acc + r.astype(object)
    return (acc % q).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _operands(n, q, batch, terms, p0=40):
    a, b = O.fill_inputs(n, q, p0, batch * terms)
    return a.reshape(batch, terms, n), b.reshape(batch, terms, n)


@functools.lru_cache(maxsize=None)
def _oracle_products(n, q, batch, terms):
    """prod[s][p][t] = oracle product of a[p][t] with b[p][t] (s = 0) or b[0][t] (s = 1, the
    shared operand), computed once per (n, q) and shared by every case that needs a prefix."""
    P = O.Plan(n, q)
    a, b = _operands(n, q, batch, terms)
    out = np.zeros((2, batch, terms, n), dtype=np.uint64)
    for p in range(batch):
        for t in range(terms):
            out[0, p, t] = P.product_merged(a[p, t], b[p, t])
            out[1, p, t] = out[0, p, t] if p == 0 else P.product_merged(a[p, t], b[0, t])
    return out


def _expected(n, q, batch, tmax, terms, shared):
    prod = _oracle_products(n, q, batch, tmax)[int(shared)]
    return _sum_mod([prod[:, t] for t in range(terms)], q)


# ---------------------------------------------------------------------------------------------
# 1. parity with the oracle
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q", [(n, q) for n in M.MAC_N for q in M.moduli_at(n)])
def test_parity_with_the_oracle(n, q, torch_cuda):
    """Every n, one modulus per arithmetic class, every word width the class allows, terms 1 and
    3 (7 at n = 256 and 4096), shared and per-batch b_hat, batch 17; b_hat = forward(b).  Equal,
    bit for bit, to the sum of the oracle's products."""
    cases = [c for c in M.parity_cases() if (c.n, c.q) == (n, q)]
    tmax = max(c.terms for c in cases)
    ctx = nttmul.MacContext(n, q)
    a, b = _operands(n, q, M.BATCH, tmax)
    for bits in D.word_options(q):
        b_hat = ctx.forward(b.reshape(-1, n), dtype=_dt(bits)).reshape(b.shape).astype(np.uint64)
        assert nttmul.dispatch_key(ctx.mac_kernel_name(bits)) == M.mac_kernel(n, q, bits)
        for case in (c for c in cases if c.word_bits == bits):
            ai = np.ascontiguousarray(a[:, :case.terms])
            bi = np.ascontiguousarray(b_hat[0, :case.terms] if case.shared else b_hat[:, :case.terms])
            got, _, _ = _mac_device(torch_cuda, ctx, ai, bi, case.shared, bits)
            want = _expected(n, q, M.BATCH, tmax, case.terms, case.shared)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (case, f"{bad.size} polynomials differ, first {bad[0]}")
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 2. worst-case ranges
# ---------------------------------------------------------------------------------------------

def _range_modulus(n, q):
    if q is not None:
        return q
    m31 = (1 << 31) - 1
    return m31 if (m31 - 1) % (2 * n) == 0 and O.is_prime(m31) else nttmul.find_prime(n, 31, False)


def _existing_path(ctx, a, b_hat, shared, q, bits):
    """inverse((sum_t pointwise(forward(a_t), b_hat_t)) mod q), the sum on the host: three
    existing, separately tested calls."""
    dt = _dt(bits)
    batch, terms, n = a.shape
    rows = []
    for t in range(terms):
        bt = np.broadcast_to(b_hat[t], (batch, n)) if shared else b_hat[:, t]
        rows.append(ctx.pointwise(ctx.forward(a[:, t], dtype=dt), bt, dtype=dt).astype(np.uint64))
    return ctx.inverse(_sum_mod(rows, q), dtype=dt).astype(np.uint64)


@pytest.mark.parametrize("n", M.RANGE_N)
@pytest.mark.parametrize("q0", M.RANGE_MODULI)
def test_worst_case_ranges(n, q0, torch_cuda):
    """Every coefficient of a and every word of b_hat equal to q - 1, seven terms: the largest
    values the accumulator can hold in each class (two moduli at the top of the Plantard range,
    the full-word and the 62-bit modulus).  Then once with b_hat random in [0, q),
    the transform of nothing in particular: any canonical vector is accepted."""
    q = _range_modulus(n, q0)
    assert q < (1 << 62) and (q - 1) % (2 * n) == 0
    bits = D.native_bits(q)
    ctx = nttmul.MacContext(n, q)
    batch, terms = M.RANGE_BATCH, M.TERMS_LONG
    a = np.full((batch, terms, n), q - 1, dtype=np.uint64)
    for shared in (False, True):
        b_hat = np.full((terms, n) if shared else a.shape, q - 1, dtype=np.uint64)
        got, _, _ = _mac_device(torch_cuda, ctx, a, b_hat, shared, bits)
        assert np.array_equal(got, _existing_path(ctx, a, b_hat, shared, q, bits)), (q, shared)
    rng = np.random.default_rng(n + q % 1000)
    b_hat = rng.integers(0, q, size=a.shape, dtype=np.uint64)
    b_hat[0, 0, :2] = (q - 1, 0)
    a2, _ = _operands(n, q, batch, terms, p0=90)
    got, _, _ = _mac_device(torch_cuda, ctx, a2, b_hat, False, bits)
    assert np.array_equal(got, _existing_path(ctx, a2, b_hat, False, q, bits)), q
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 3. cyclic contexts
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q0,omega", M.CYCLIC)
def test_cyclic_contexts(n, q0, omega, torch_cuda):
    """On a NTTMUL_FLAG_CYCLIC context the same call uses the cyclic transforms: the sum of the
    cyclic schoolbook products."""
    q = q0 or nttmul.find_prime(n, 31, True)
    ctx = nttmul.MacContext(n, q, psi=omega, cyclic=True)
    batch, terms = 5, M.CYCLIC_TERMS
    a, b = _operands(n, q, batch, terms, p0=60)
    b_hat = ctx.forward(b.reshape(-1, n)).reshape(b.shape).astype(np.uint64)
    got, _, _ = _mac_device(torch_cuda, ctx, a, b_hat, False, 32)
    want = _sum_mod([np.stack([O.cyclic_schoolbook(a[p, t], b[p, t], n, q) for p in range(batch)])
                     for t in range(terms)], q)
    assert np.array_equal(got, want)
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 4. device-path rules
# ---------------------------------------------------------------------------------------------

def test_device_path_rules(torch_cuda):
    """A non-null stream; a shared operand really shared (tiling it per batch gives the same
    result); inputs unchanged; the empty batch; bad arguments; n = 8192 unsupported; and the
    product bookkeeping (nttmul_last_kernel_name) untouched."""
    torch = torch_cuda
    n, q, bits = M.RULES
    ctx = nttmul.MacContext(n, q)
    batch, terms = 5, 2
    a, b = _operands(n, q, batch, terms, p0=70)
    b_hat = ctx.forward(b[0]).astype(np.uint64)                     # [terms][n]
    side = torch.cuda.Stream()
    shared, a_after, b_after = _mac_device(torch, ctx, a, b_hat, True, bits, stream=side.cuda_stream)
    assert np.array_equal(a_after, a) and np.array_equal(b_after, b_hat)
    tiled = np.ascontiguousarray(np.broadcast_to(b_hat, (batch, terms, n)))
    per_batch, _, _ = _mac_device(torch, ctx, a, tiled, False, bits, stream=side.cuda_stream)
    assert np.array_equal(shared, per_batch)
    assert np.array_equal(shared, _expected_rules(n, q, a, b))
    assert ctx.last_kernel_name() == ""
    # an empty batch enqueues nothing and dereferences nothing
    ctx.mac_ntt_device(0, 0, 0, 0, 1, bits)
    da = _to_dev(torch, a, bits)
    for args in ((da, da, da, batch, 0, bits),                      # terms = 0
                 (0, da, da, batch, 1, bits)):                      # NULL c
        with pytest.raises(nttmul.NttmulError) as ei:
            ctx.mac_ntt_device(*args)
        assert ei.value.status == nttmul.NTTMUL_EINVAL
    with pytest.raises(ValueError):                                 # no such word
        ctx.mac_ntt_device(da, da, da, batch, 1, 16)
    ctx.close()
    wide = nttmul.MacContext(256, D.Q62)
    d64 = torch.zeros(256, dtype=torch.int64, device="cuda")
    with pytest.raises(nttmul.NttmulError) as ei:                   # 32-bit words for q >= 2^32
        wide._check(wide._lib.nttmul_mac_ntt_device(wide._h, d64.data_ptr(), d64.data_ptr(),
                                                    d64.data_ptr(), 1, 1, 0, 32, 0, None))
    assert ei.value.status == nttmul.NTTMUL_EINVAL
    wide.close()
    big = nttmul.MacContext(M.UNSUPPORTED_N, D.Q31)
    d = torch.zeros(M.UNSUPPORTED_N, dtype=torch.int32, device="cuda")
    with pytest.raises(nttmul.NttmulError) as ei:
        big.mac_ntt_device(d, d, d, 1, 1, 32)
    assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED
    with pytest.raises(nttmul.NttmulError) as ei:
        big.mac_kernel_name(32)
    assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED
    big.close()


def _expected_rules(n, q, a, b):
    P = O.Plan(n, q)
    return _sum_mod([np.stack([P.product_merged(a[p, t], b[0, t]) for p in range(a.shape[0])])
                     for t in range(a.shape[1])], q)


def test_validate_flag_checks_both_operands(torch_cuda):
    """NTTMUL_FLAG_VALIDATE: a word equal to q in b_hat, or in a, is NTTMUL_ERANGE; clean
    operands pass, with a shared operand too (its range check covers [terms][n] words only)."""
    torch = torch_cuda
    n, q, bits = M.VALIDATE
    ctx = nttmul.MacContext(n, q, validate=True)
    batch, terms = 3, 2
    a, b = _operands(n, q, batch, terms, p0=80)
    b_hat = ctx.forward(b.reshape(-1, n)).reshape(b.shape).astype(np.uint64)
    good, _, _ = _mac_device(torch, ctx, a, b_hat, False, bits)
    assert np.array_equal(good, _existing_path(ctx, a, b_hat, False, q, bits))
    _mac_device(torch, ctx, a, b_hat[0], True, bits)
    for which in ("a", "b_hat"):
        x, y = a.copy(), b_hat.copy()
        (x if which == "a" else y)[batch - 1, terms - 1, n - 1] = q
        with pytest.raises(nttmul.NttmulError) as ei:
            _mac_device(torch, ctx, x, y, False, bits)
        assert ei.value.status == nttmul.NTTMUL_ERANGE, which
    y = b_hat[0].copy()
    y[terms - 1, n - 1] = q
    with pytest.raises(nttmul.NttmulError) as ei:
        _mac_device(torch, ctx, a, y, True, bits)
    assert ei.value.status == nttmul.NTTMUL_ERANGE
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 5. host forms
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q", M.moduli_at(M.HOST[0]))
def test_host_forms(q, torch_cuda):
    """nttmul_mac_ntt_u32 / _u64 on numpy arrays, against the oracle sum; shapes are checked."""
    n, batch, terms = M.HOST
    ctx = nttmul.MacContext(n, q)
    a, b = _operands(n, q, M.BATCH, 3)
    a, b = a[:batch, :terms], b[:batch, :terms]
    want = [_expected(n, q, M.BATCH, 3, terms, s)[:batch] for s in (False, True)]
    for bits in D.word_options(q):
        dt = _dt(bits)
        b_hat = ctx.forward(b.reshape(-1, n), dtype=dt).reshape(b.shape)
        got = ctx.mac_ntt(a, b_hat, dtype=dt)
        assert got.dtype == dt and got.shape == (batch, n)
        assert np.array_equal(got.astype(np.uint64), want[0]), bits
        got = ctx.mac_ntt(a, b_hat[0], shared=True, dtype=dt)
        assert np.array_equal(got.astype(np.uint64), want[1]), bits
    with pytest.raises(ValueError):
        ctx.mac_ntt(a, b_hat[0])                        # [terms][n] without shared
    with pytest.raises(ValueError):
        ctx.mac_ntt(a[:, 0], b_hat[:, 0])               # no terms axis
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 6. dispatch anchor
# ---------------------------------------------------------------------------------------------

def test_mirror_agrees_with_the_library_dispatch(torch_cuda):
    """nttmul_mac_kernel_name (the dry run of the launching statement) equals the mirror's kernel
    for every case of tests/mac_cases.py, and names a kernel of the loaded code object."""
    table = nttmul.kernel_hashes(nttmul.MAC_LIB_PATH)
    ctxs = {}
    for case in M.all_cases():
        ck = (case.n, case.q)
        if ck not in ctxs:
            ctxs[ck] = nttmul.MacContext(case.n, case.q)
        name = ctxs[ck].mac_kernel_name(case.word_bits)
        assert name == M.mac_kernel(case.n, case.q, case.word_bits), case
        assert nttmul.dispatch_key(name) in table, name
    assert len(ctxs) >= 15
    for ctx in ctxs.values():
        ctx.close()
