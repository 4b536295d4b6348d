"""GPU parity of the limb-aware multi-pass calls (include/nttmul_rnsmp.h, lib/libnttmul_rnsmp.so,
csrc/rnsmp_dev.hpp k_rnsmp_cols_fwd / k_rnsmp_rows / k_rnsmp_xform / k_rnsmp_mac /
k_rnsmp_cols_inv): every pass one launch over [batch][limbs][n] operands, 4096 < n <= 65536.

Everything is bit-exact.  Expected products come from the CPU oracle per (polynomial, limb),
summed in Python integers for the mac.  The transforms, and one product per (n, class), are
compared limb by limb against plain contexts nttmul_create(n, q_l) of the same loaded library over
limb-major copies: the header's bit-for-bit promise.  Inputs are the oracle's counter-based fill
per limb, so every limb's words are canonical for its own modulus.  Shapes are the smallest at
which the kernels can go wrong (tests/rnsmp_cases.py): every n has its own column pass, batch 3 is
more than one polynomial and no power of two, L = 3 and 5 put a limb between two others."""
import functools

import numpy as np
import pytest

import guarded as G
import nttmul
import rnsmp_cases as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CLASSES = {"u32": R.BASIS32, "u64": R.BASIS64}


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


def _from_dev(t, bits, shape):
    return t.cpu().numpy().view(_dt(bits)).reshape(shape).astype(np.uint64)


def _call(torch, ctx, op, a, b=None, shared=False, stream=0, in_place=False):
    """One device call on numpy operands, out of a guarded arena (tests/guarded.py: every operand
    between sentinel guards, aligned to its word only, the output preset to the sentinel; after
    the call no guard word and no input has changed and every output word is written); returns
    (result, operands after the call)."""
    bits = ctx.word_bits
    batch = a.shape[0]
    words = batch * ctx.limbs * ctx.n
    operands = dict(a=a) if b is None else dict(a=a, b=b)
    if not in_place:
        operands["c"] = words
    guard = G.guard_words(a.size // batch, 0 if b is None else b.size // (1 if shared else batch))
    arena = G.DeviceArena(torch, bits, guard, inplace=("a",) if in_place else (), **operands)
    da, db = arena["a"], None if b is None else arena["b"]
    dc = da if in_place else arena["c"]
    if op == "multiply":
        ctx.multiply_device(dc, da, db, batch, stream=stream)
    elif op == "forward":
        ctx.forward_device(dc, da, batch, stream=stream)
    elif op == "inverse":
        ctx.inverse_device(dc, da, batch, stream=stream)
    else:
        ctx.mac_ntt_device(dc, da, db, batch, a.shape[1], shared=shared, stream=stream)
    torch.cuda.synchronize()
    arena.check()
    after = [arena.get(k, x.shape).astype(np.uint64) for k, x in (("a", a), ("b", b)) if x is not None]
    return arena.get("a" if in_place else "c", (batch, ctx.limbs, ctx.n)).astype(np.uint64), after


def _sum_mod(rows, q):
    """sum of uint64 arrays mod q, in Python integers."""
    acc = rows[0].astype(object)
    for r in rows[1:]:
        acc = acc + r.astype(object)
    return (acc % q).astype(np.uint64)


def _tmax(n):
    return max(R.terms_at(n))


@functools.lru_cache(maxsize=None)
def _limb_operands(n, q, batch, terms, p0=40):
    a, b = O.fill_inputs(n, q, p0, batch * terms)
    a.setflags(write=False)
    b.setflags(write=False)
    return a.reshape(batch, terms, n), b.reshape(batch, terms, n)


def _operands(n, moduli, batch, terms, p0=40):
    """a, b of shape [batch, terms, limbs, n], limb l canonical for moduli[l]."""
    per = [_limb_operands(n, q, batch, terms, p0) for q in moduli]
    return (np.ascontiguousarray(np.stack([x[0] for x in per], axis=2)),
            np.ascontiguousarray(np.stack([x[1] for x in per], axis=2)))


@functools.lru_cache(maxsize=None)
def _oracle_products(n, q):
    """prod[s][p][t] = oracle product of a[p][t] with b[p][t] (s = 0) or b[0][t] (s = 1, the
    shared operand) of one limb, computed once per (n, q) and shared by every test."""
    P = O.Plan(n, q)
    batch, terms = R.BATCH, _tmax(n)
    a, b = _limb_operands(n, q, batch, terms)
    out = np.zeros((2, batch, terms, n), dtype=np.uint64)
    for p in range(batch):
        for t in range(terms):
            out[0, p, t] = P.product_merged(a[p, t], b[p, t])
            out[1, p, t] = out[0, p, t] if p == 0 else P.product_merged(a[p, t], b[0, t])
    out.setflags(write=False)
    return out


def _expected_mac(n, moduli, terms, shared):
    """[BATCH, limbs, n]: per limb, the sum over t < terms of the oracle's products."""
    return np.stack([_sum_mod([_oracle_products(n, q)[int(shared)][:, t] for t in range(terms)], q)
                     for q in moduli], axis=1)


def _oracle_rows(n, moduli, a, b):
    """Oracle products of a, b [batch, limbs, n] per (polynomial, limb)."""
    return np.stack([np.stack([O.Plan(n, q).product_merged(a[p, l], b[p, l])
                               for l, q in enumerate(moduli)]) for p in range(a.shape[0])])


_PLAIN = {}


def _plain(n, q):
    """A plain context nttmul_create(n, q) of the loaded lib/libnttmul_rnsmp.so itself (kept for
    the module: a handful of (n, q))."""
    if (n, q) not in _PLAIN:
        _PLAIN[n, q] = nttmul.Context(n, q, _lib=nttmul.load_rnsmp_library())
    return _PLAIN[n, q]


@pytest.fixture(scope="module", autouse=True)
def _close_plain_contexts():
    yield
    while _PLAIN:
        _PLAIN.popitem()[1].close()


def _plain_per_limb(op, n, moduli, x, dtype, y=None):
    """op of plain contexts on limb-major copies of x (and y) [batch, limbs, n], limb by limb."""
    out = []
    for l, q in enumerate(moduli):
        args = [np.ascontiguousarray(v[:, l]) for v in (x, y) if v is not None]
        out.append(getattr(_plain(n, q), op)(*args, dtype=dtype))
    return np.stack(out, axis=1).astype(np.uint64)


def _plain_forward_terms(n, moduli, b, dtype):
    """forward of b [batch, terms, limbs, n] per limb, by plain contexts."""
    batch, terms = b.shape[:2]
    flat = _plain_per_limb("forward", n, moduli, b.reshape(batch * terms, len(moduli), n), dtype)
    return flat.reshape(b.shape)


def _differ(got, want):
    bad = np.argwhere((got != want).any(axis=-1))
    return f"{len(bad)} (polynomial, limb) pairs differ, first {bad[0] if len(bad) else None}"


PARAMS = [(n, c) for n in R.RNSMP_N for c in CLASSES]


def _bases(n, cls):
    return [m for m in R.bases_at(n) if R.word_bits(m) == R.word_bits(CLASSES[cls])]


# ---------------------------------------------------------------------------------------------
# 1. products
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,cls", PARAMS)
def test_product_parity_with_the_oracle(n, cls, torch_cuda):
    """Every n, L in {1, 3} (and five 32-bit limbs at two n), batch 3 and 1: each (p, l) equals
    the oracle's product mod q_l; operands unchanged; the L = 3 result equals plain contexts' of
    the same library limb by limb."""
    for moduli in _bases(n, cls):
        ctx = nttmul.RnsMpContext(n, moduli)
        assert (ctx.limbs, ctx.word_bits) == (len(moduli), R.word_bits(moduli))
        assert ctx.kernel_name("multiply") == R.kernel_name("multiply", n, moduli)
        a, b = _operands(n, moduli, R.BATCH, _tmax(n))
        a, b = np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(b[:, 0])
        want = np.stack([_oracle_products(n, q)[0][:, 0] for q in moduli], axis=1)
        for batch in (R.BATCH, 1):
            got, after = _call(torch_cuda, ctx, "multiply", a[:batch], b[:batch])
            assert np.array_equal(got, want[:batch]), (moduli, batch, _differ(got, want[:batch]))
            assert np.array_equal(after[0], a[:batch]) and np.array_equal(after[1], b[:batch])
        if len(moduli) == 3:
            got, _ = _call(torch_cuda, ctx, "multiply", a, b)
            plain = _plain_per_limb("multiply", n, moduli, a, ctx.io_dtype, b)
            assert np.array_equal(got, plain), (moduli, _differ(got, plain))
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 2. transforms
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,cls", PARAMS)
def test_transforms_equal_plain_contexts_per_limb(n, cls, torch_cuda):
    """forward and inverse against plain contexts of (n, q_l), limb by limb (output order and
    range included), batch 3 and 1; then inverse(forward(a)) == a with both calls in place."""
    for moduli in _bases(n, cls):
        ctx = nttmul.RnsMpContext(n, moduli)
        dt = ctx.io_dtype
        a, _ = _operands(n, moduli, R.BATCH, _tmax(n))
        a = np.ascontiguousarray(a[:, 0])
        fwd = _plain_per_limb("forward", n, moduli, a, dt)
        inv = _plain_per_limb("inverse", n, moduli, a, dt)
        for op, want in (("forward", fwd), ("inverse", inv)):
            assert ctx.kernel_name(op) == R.kernel_name(op, n, moduli)
            for batch in (R.BATCH, 1):
                got, after = _call(torch_cuda, ctx, op, a[:batch])
                assert np.array_equal(got, want[:batch]), (op, moduli, batch, _differ(got, want[:batch]))
                assert np.array_equal(after[0], a[:batch])
        hat, after = _call(torch_cuda, ctx, "forward", a, in_place=True)
        assert np.array_equal(hat, fwd) and np.array_equal(after[0], fwd)
        back, _ = _call(torch_cuda, ctx, "inverse", hat, in_place=True)
        assert np.array_equal(back, a), (moduli, _differ(back, a))
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 3. multiply-accumulate against NTT-domain operands
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,cls", PARAMS)
def test_mac_parity_with_the_oracle(n, cls, torch_cuda):
    """terms 1 and 3 (7 at n = 8192 and 65536), shared and per-batch b_hat = forward(b) by plain
    contexts, batch 3 (and once batch 1): each (p, l) equals the sum of the oracle's products
    mod q_l."""
    for moduli in _bases(n, cls):
        ctx = nttmul.RnsMpContext(n, moduli)
        assert ctx.kernel_name("mac") == R.kernel_name("mac", n, moduli)
        a, b = _operands(n, moduli, R.BATCH, _tmax(n))
        b_hat = _plain_forward_terms(n, moduli, b, ctx.io_dtype)
        for terms in R.terms_at(n):
            for shared in (False, True):
                ai = np.ascontiguousarray(a[:, :terms])
                bi = np.ascontiguousarray(b_hat[0, :terms] if shared else b_hat[:, :terms])
                got, after = _call(torch_cuda, ctx, "mac", ai, bi, shared=shared)
                want = _expected_mac(n, moduli, terms, shared)
                assert np.array_equal(got, want), (moduli, terms, shared, _differ(got, want))
                assert np.array_equal(after[0], ai) and np.array_equal(after[1], bi)
        terms = _tmax(n)                                    # and a batch of one
        got, _ = _call(torch_cuda, ctx, "mac", a[:1, :terms], b_hat[:1, :terms])
        assert np.array_equal(got, _expected_mac(n, moduli, terms, False)[:1]), moduli
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 4. worst-case ranges
# ---------------------------------------------------------------------------------------------

def _existing_mac(n, moduli, a, b_hat, shared, dt):
    """Per limb inverse((sum_t pointwise(forward(a_t), b_hat_t)) mod q), the sum on the host:
    three calls of a plain context."""
    out = []
    for l, q in enumerate(moduli):
        P = _plain(n, q)
        rows = []
        for t in range(a.shape[1]):
            bt = np.broadcast_to(b_hat[t, l], a[:, t, l].shape) if shared else b_hat[:, t, l]
            rows.append(P.pointwise(P.forward(np.ascontiguousarray(a[:, t, l]), dtype=dt),
                                    np.ascontiguousarray(bt), dtype=dt).astype(np.uint64))
        out.append(P.inverse(_sum_mod(rows, q), dtype=dt).astype(np.uint64))
    return np.stack(out, axis=1)


@pytest.mark.parametrize("n", R.RANGE_N)
@pytest.mark.parametrize("cls", list(CLASSES))
def test_worst_case_ranges(n, cls, torch_cuda):
    """Every word q_l - 1: the product against the oracle, and a seven-term mac (the largest
    values the accumulator can hold in each class, on rows that read the column pass's lazy
    words) against plain contexts' forward / pointwise / inverse with the sum on the host,
    shared and per-batch."""
    moduli = CLASSES[cls]
    ctx = nttmul.RnsMpContext(n, moduli)
    batch, terms, L = R.RANGE_BATCH, R.TERMS_LONG, len(moduli)
    top = np.array([q - 1 for q in moduli], dtype=np.uint64)
    a = np.ascontiguousarray(np.broadcast_to(top[None, None, :, None], (batch, terms, L, n)))
    got, _ = _call(torch_cuda, ctx, "multiply", a[:, 0], a[:, 0])
    want = np.stack([O.Plan(n, q).product_merged(a[0, 0, l], a[0, 0, l]) for l, q in enumerate(moduli)])
    assert np.array_equal(got, np.broadcast_to(want, got.shape))
    for shared in (False, True):
        b_hat = a[0] if shared else a
        got, _ = _call(torch_cuda, ctx, "mac", a, b_hat, shared=shared)
        assert np.array_equal(got, _existing_mac(n, moduli, a, b_hat, shared, ctx.io_dtype)), shared
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 5. sub-batches
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,moduli,batch,want_chunks,terms,mbatch,want_mchunks", R.SUBBATCH)
def test_sub_batches_with_one_mib_of_scratch(n, moduli, batch, want_chunks, terms, mbatch,
                                             want_mchunks, torch_cuda):
    """scratch_mb = 1: the batch runs in the sub-batches the mirror computes (asserted through the
    mirror, whose rule is rnsmp.cpp run's), each output preset to the sentinel and equal, bit for
    bit, to what a context with the default scratch writes in one pass and to the oracle."""
    assert R.chunks(R.Case("multiply", n, moduli, batch, scratch_mb=1)) == list(want_chunks)
    assert R.chunks(R.Case("forward", n, moduli, batch, scratch_mb=1)) == list(want_chunks)
    assert R.chunks(R.Case("mac", n, moduli, mbatch, terms, scratch_mb=1)) == list(want_mchunks)
    assert len(R.chunks(R.Case("multiply", n, moduli, batch))) == 1
    small, whole = nttmul.RnsMpContext(n, moduli, scratch_mb=1), nttmul.RnsMpContext(n, moduli)
    assert (small.info.scratch_mb, whole.info.scratch_mb) == (1, R.DEFAULT_SCRATCH_MB)
    a, b = _operands(n, moduli, max(batch, mbatch), terms, p0=90)
    x, y = np.ascontiguousarray(a[:batch, 0]), np.ascontiguousarray(b[:batch, 0])
    got, _ = _call(torch_cuda, small, "multiply", x, y)
    ref, _ = _call(torch_cuda, whole, "multiply", x, y)
    assert np.array_equal(got, ref), _differ(got, ref)
    some = sorted({0, want_chunks[0] - 1, want_chunks[0] % batch, batch - 1})   # chunk borders
    assert np.array_equal(got[some], _oracle_rows(n, moduli, x[some], y[some]))
    hat, _ = _call(torch_cuda, small, "forward", x)
    ref, _ = _call(torch_cuda, whole, "forward", x)
    assert np.array_equal(hat, ref), _differ(hat, ref)
    back, _ = _call(torch_cuda, small, "inverse", hat)
    assert np.array_equal(back, x), _differ(back, x)
    b_hat = np.stack([_call(torch_cuda, whole, "forward", np.ascontiguousarray(b[:mbatch, t]))[0]
                      for t in range(terms)], axis=1)
    am = np.ascontiguousarray(a[:mbatch])
    for shared in (False, True):
        bi = np.ascontiguousarray(b_hat[0] if shared else b_hat)
        got, _ = _call(torch_cuda, small, "mac", am, bi, shared=shared)
        ref, _ = _call(torch_cuda, whole, "mac", am, bi, shared=shared)
        assert np.array_equal(got, ref), (shared, _differ(got, ref))
        last = mbatch - 1
        want = np.stack([_sum_mod([O.Plan(n, q).product_merged(a[last, t, l], b[0 if shared else last, t, l])
                                   for t in range(terms)], q) for l, q in enumerate(moduli)])
        assert np.array_equal(got[last], want), shared
    small.close()
    whole.close()


# ---------------------------------------------------------------------------------------------
# 6. rules of the device path
# ---------------------------------------------------------------------------------------------

def test_reversed_basis_permutes_the_limbs(torch_cuda):
    """The same basis in reversed order gives the same limbs in reversed order, for every
    operation: the table index, the twiddle base and the addressing follow the limb, nothing else
    does."""
    n, moduli = R.RULES
    rev = moduli[::-1]
    batch, terms = 5, 2
    a, b = _operands(n, moduli, batch, terms, p0=70)
    fwd_ctx, rev_ctx = nttmul.RnsMpContext(n, moduli), nttmul.RnsMpContext(n, rev)
    b_hat = _plain_forward_terms(n, moduli, b, fwd_ctx.io_dtype)
    flip = lambda x: np.ascontiguousarray(np.flip(x, axis=-2))          # noqa: E731
    for op, x, y in (("multiply", a[:, 0], b[:, 0]), ("forward", a[:, 0], None),
                     ("inverse", a[:, 0], None), ("mac", a, b_hat)):
        got, _ = _call(torch_cuda, fwd_ctx, op, np.ascontiguousarray(x),
                       None if y is None else np.ascontiguousarray(y))
        got_rev, _ = _call(torch_cuda, rev_ctx, op, flip(x), None if y is None else flip(y))
        assert np.array_equal(flip(got_rev), got), op
    assert [rev_ctx.limb_info(l).q for l in range(3)] == list(rev)
    info = fwd_ctx.limb_info(1)
    assert (info.n, info.q, info.psi) == (n, moduli[1], nttmul.smallest_psi(n, moduli[1]))
    fwd_ctx.close()
    rev_ctx.close()


def test_device_path_rules(torch_cuda):
    """A non-default stream; the empty batch; bad arguments on a live context; shapes checked
    before the call."""
    torch = torch_cuda
    n, moduli = R.RULES
    ctx = nttmul.RnsMpContext(n, moduli)
    batch, terms = 5, 2
    a, b = _operands(n, moduli, batch, terms, p0=70)
    side = torch.cuda.Stream()
    want = _oracle_rows(n, moduli, a[:, 0], b[:, 0])
    got, _ = _call(torch, ctx, "multiply", np.ascontiguousarray(a[:, 0]),
                   np.ascontiguousarray(b[:, 0]), stream=side.cuda_stream)
    assert np.array_equal(got, want)
    b_hat = _plain_forward_terms(n, moduli, b, ctx.io_dtype)
    shared, _ = _call(torch, ctx, "mac", a, np.ascontiguousarray(b_hat[0]), shared=True,
                      stream=side.cuda_stream)
    tiled = np.ascontiguousarray(np.broadcast_to(b_hat[0], a.shape))
    per_batch, _ = _call(torch, ctx, "mac", a, tiled, stream=side.cuda_stream)
    assert np.array_equal(shared, per_batch)
    # an empty batch enqueues nothing and dereferences nothing
    ctx.multiply_device(0, 0, 0, 0)
    ctx.forward_device(0, 0, 0)
    ctx.mac_ntt_device(0, 0, 0, 0, 1)
    da = _to_dev(torch, a, 32)
    for call in (lambda: ctx.mac_ntt_device(da, da, da, 1, 0),             # terms = 0
                 lambda: ctx.mac_ntt_device(0, da, da, 1, 1),              # NULL c
                 lambda: ctx.multiply_device(da, da, 0, 1),                # NULL b
                 lambda: ctx.inverse_device(da, 0, 1)):                    # NULL in
        with pytest.raises(nttmul.NttmulError) as ei:
            call()
        assert ei.value.status == nttmul.NTTMUL_EINVAL
    with pytest.raises(nttmul.NttmulError) as ei:
        p = da.data_ptr()
        ctx.multiply_device(p, p, p, 1, dev=7)                             # not the context's
    assert ei.value.status == nttmul.NTTMUL_ENODEV
    with pytest.raises(ValueError):                                        # too few words
        ctx.multiply_device(da, da, da, batch * terms + 1)
    with pytest.raises(ValueError):                                        # 64-bit tensor
        ctx.forward_device(da.to(torch.int64), da.to(torch.int64), 1)
    with pytest.raises(nttmul.NttmulError) as ei:
        ctx.kernel_name(4)
    assert ei.value.status == nttmul.NTTMUL_EINVAL
    ctx.close()
    for bad_n in (4096, 131072):
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.RnsMpContext(bad_n, moduli[:1])
        assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED


@pytest.mark.parametrize("n,moduli,limb,other", R.VALIDATE)
def test_validate_flag_checks_each_word_against_its_own_limb(n, moduli, limb, other, torch_cuda):
    """NTTMUL_FLAG_VALIDATE: a word equal to q_limb in limb `limb` is NTTMUL_ERANGE in every
    operand of every operation, while the same value in a limb with a larger modulus passes --
    the check is per limb.  Clean operands pass, a shared b_hat too."""
    torch = torch_cuda
    ctx = nttmul.RnsMpContext(n, moduli, validate=True)
    batch, terms = 3, 2
    a, b = _operands(n, moduli, batch, terms, p0=80)
    b_hat = _plain_forward_terms(n, moduli, b, ctx.io_dtype)
    value = moduli[limb]
    assert value < moduli[other]
    calls = {"multiply": (a[:, 0], b[:, 0]), "forward": (a[:, 0], None),
             "inverse": (a[:, 0], None), "mac": (a, b_hat)}
    for op, (x, y) in calls.items():
        x = np.ascontiguousarray(x)
        y = None if y is None else np.ascontiguousarray(y)
        _call(torch, ctx, op, x, y)                                         # clean
        for which in (0, 1) if y is not None else (0,):
            ops = [x.copy(), None if y is None else y.copy()]
            ops[which][batch - 1, ..., other, n - 1] = value                # in range there
            _call(torch, ctx, op, *ops)
            ops[which][batch - 1, ..., limb, n - 1] = value                 # out of range here
            with pytest.raises(nttmul.NttmulError) as ei:
                _call(torch, ctx, op, *ops)
            assert ei.value.status == nttmul.NTTMUL_ERANGE, (op, which)
    y = np.ascontiguousarray(b_hat[0])
    _call(torch, ctx, "mac", a, y, shared=True)
    y[terms - 1, limb, n - 1] = value
    with pytest.raises(nttmul.NttmulError) as ei:
        _call(torch, ctx, "mac", a, y, shared=True)
    assert ei.value.status == nttmul.NTTMUL_ERANGE
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 7. host forms
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,moduli", R.HOST)
def test_host_forms_equal_device_forms(n, moduli, torch_cuda):
    """nttmul_rnsmp_multiply / forward / inverse / mac_ntt on numpy arrays equal the device forms
    (and the oracle, for the product); shapes are checked."""
    ctx = nttmul.RnsMpContext(n, moduli)
    dt = ctx.io_dtype
    batch, terms = R.HOST_BATCH, R.HOST_TERMS
    a, b = _operands(n, moduli, batch, terms, p0=60)
    x, y = np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(b[:, 0])
    got = ctx.multiply(x, y)
    assert got.dtype == dt and got.shape == (batch, len(moduli), n)
    dev, _ = _call(torch_cuda, ctx, "multiply", x, y)
    assert np.array_equal(got.astype(np.uint64), dev)
    assert np.array_equal(dev, _oracle_rows(n, moduli, x, y))
    hat = ctx.forward(x)
    assert np.array_equal(hat.astype(np.uint64), _call(torch_cuda, ctx, "forward", x)[0])
    assert np.array_equal(ctx.inverse(hat).astype(np.uint64), x)
    assert np.array_equal(ctx.inverse(x).astype(np.uint64), _call(torch_cuda, ctx, "inverse", x)[0])
    b_hat = np.stack([ctx.forward(b[:, t]) for t in range(terms)], axis=1)
    for shared in (False, True):
        bi = np.ascontiguousarray(b_hat[0] if shared else b_hat)
        got = ctx.mac_ntt(a, bi, shared=shared)
        assert got.dtype == dt and got.shape == (batch, len(moduli), n)
        dev, _ = _call(torch_cuda, ctx, "mac", a, bi.astype(np.uint64), shared=shared)
        assert np.array_equal(got.astype(np.uint64), dev), shared
    with pytest.raises(ValueError):
        ctx.mac_ntt(a, b_hat[0])                        # [terms, limbs, n] without shared
    with pytest.raises(ValueError):
        ctx.mac_ntt(a[:, 0], b_hat[:, 0])               # no terms axis
    with pytest.raises(ValueError):
        ctx.multiply(a[:, 0, :2], b[:, 0, :2])          # too few limbs
    with pytest.raises(ValueError):
        ctx.forward(a[0, 0])                            # no batch axis
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 8. lifetime: one context, two streams, a scratch that grows after its first use
# ---------------------------------------------------------------------------------------------

def test_one_context_serves_two_streams_and_a_growing_scratch(torch_cuda):
    """Product, mac, forward and inverse in turn on one context, alternating between two streams
    with no synchronisation between the calls, every step on inputs of its own and into an output
    preset to the sentinel; the batch is raised in the middle, so the scratch grows after its
    first use.  Every output is compared bit for bit at the end: the scratch is handed from
    stream to stream by the context's event."""
    torch = torch_cuda
    n, moduli = R.RULES
    bits, L, terms = 32, len(moduli), R.LIFETIME_TERMS
    ctx = nttmul.RnsMpContext(n, moduli)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    sent = G.sentinel(bits)
    steps, k = [], 0
    for rnd, batch in enumerate(R.LIFETIME_BATCHES * 2):        # 2, 5, 2, 5: grows at the second
        a, b = _operands(n, moduli, batch, terms, p0=100 + 10 * rnd)
        b_hat = _plain_forward_terms(n, moduli, b, ctx.io_dtype)
        x, y = np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(b[:, 0])
        want = {"multiply": lambda: _oracle_rows(n, moduli, x, y),
                "mac": lambda: np.stack([_sum_mod([O.Plan(n, q).product_merged(a[p, t, l], b[p, t, l])
                                                   for t in range(terms)], q)
                                         for p in range(batch) for l, q in enumerate(moduli)]
                                        ).reshape(batch, L, n),
                "forward": lambda: _plain_per_limb("forward", n, moduli, x, ctx.io_dtype),
                "inverse": lambda: _plain_per_limb("inverse", n, moduli, x, ctx.io_dtype)}
        for op in ("multiply", "mac", "forward", "inverse"):
            ins = {"multiply": (x, y), "mac": (a, b_hat), "forward": (x,), "inverse": (x,)}[op]
            dins = [_to_dev(torch, v, bits) for v in ins]
            out = _to_dev(torch, np.full(batch * L * n, sent, dtype=np.uint64).astype(_dt(bits)), bits)
            steps.append((op, batch, dins, out, want[op](), streams[k % 2]))
            k += 1
    torch.cuda.synchronize()
    for op, batch, dins, out, _, s in steps:                    # no synchronisation in this loop
        if op == "multiply":
            ctx.multiply_device(out, dins[0], dins[1], batch, stream=s.cuda_stream)
        elif op == "mac":
            ctx.mac_ntt_device(out, dins[0], dins[1], batch, terms, stream=s.cuda_stream)
        elif op == "forward":
            ctx.forward_device(out, dins[0], batch, stream=s.cuda_stream)
        else:
            ctx.inverse_device(out, dins[0], batch, stream=s.cuda_stream)
    torch.cuda.synchronize()
    for i, (op, batch, _, out, want, _) in enumerate(steps):
        got = _from_dev(out, bits, (batch, L, n))
        assert not (got == sent).any(), (i, op)
        assert np.array_equal(got, want), (i, op, batch, _differ(got, want))
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 9. dispatch anchor
# ---------------------------------------------------------------------------------------------

def test_mirror_agrees_with_the_library_dispatch(torch_cuda):
    """nttmul_rnsmp_kernel_name (the dry run of the launching statements) equals the mirror's
    sequence for every case of tests/rnsmp_cases.py, and names kernels of the loaded code object."""
    table = nttmul.kernel_hashes(nttmul.RNSMP_LIB_PATH)
    ctxs = {}
    for case in R.all_cases():
        ck = (case.n, case.moduli)
        if ck not in ctxs:
            ctxs[ck] = nttmul.RnsMpContext(case.n, case.moduli)
        name = ctxs[ck].kernel_name(case.op)
        assert name == R.kernel_name(case.op, case.n, case.moduli), case
        assert all(k in table for k in name.split(" + ")), name
        assert ctxs[ck].kernel_name(R.OPS.index(case.op)) == name
    assert len(ctxs) >= 18
    for ctx in ctxs.values():
        ctx.close()
