"""GPU parity of the 32-bit-modulus kernels on 64-bit caller words, and of the standalone
transforms at every size.

A caller reaches these kernels with word_bits = 64 (the *_u64 entry points, torch.int64 device
buffers) on a context whose q < 2^32: the arithmetic stays 32-bit (Arith32P / Arith32P3 /
Arith32W) while operands, results and the bit-reversal buffer are 8-byte words.  Everything is
bit-exact against the CPU oracle; the axes come from tests/dispatch_cases.py, whose ledger test
names the kernels each case launches."""
import numpy as np
import pytest

import dispatch_cases as D
import guarded as G
import nttmul
from oracle import oracle as O
from test_gpu_parity import (_as_np, _check_whole_batch, _random_primes, _xf_expected,  # noqa: F401
                             torch_cuda)

pytestmark = pytest.mark.gpu


def _mulmod_rows(x, y, q):
    """x * y mod q elementwise with Python integers."""
    return ((x.astype(object) * y.astype(object)) % q).astype(np.uint64)


def _guarded_host(ctx, entry, dt, x, y=None, mode=None):
    """One host-buffer call (nttmul_transform_batch_* with `mode`, nttmul_pointwise_batch_* with
    y) whose operands and result live in a guarded arena (tests/guarded.py: between sentinel
    guards, aligned to their word only): after the call no guard word and no input word has
    changed and every output word is written.  Returns the result in x's shape."""
    bits = 32 if dt == np.uint32 else 64
    operands = dict(out=x.size, x=x) if y is None else dict(out=x.size, x=x, y=y)
    arena = G.HostArena(bits, G.guard_words(ctx.n), **operands)
    fn = getattr(ctx._lib, f"{entry}_u{bits}")
    ptrs = [arena[k].ctypes.data for k in operands]
    ctx._check(fn(ctx._h, *([] if mode is None else [mode]), *ptrs, x.shape[0]))
    arena.check()
    return arena.get("out", x.shape)


def test_named_moduli_are_what_the_tables_say(torch_cuda):
    assert _random_primes([33], 17, seed=D.SEED33) == [D.Q33]
    assert all(O.is_prime(q) and (q - 1) % (1 << 17) == 0
               for q in D.PLANTARD + D.WIDE + D.ARITH64)


# ---------------------------------------------------------------------------------------------
# 1a. products
# ---------------------------------------------------------------------------------------------

def _edge_operands(n, q, batch=3):
    a, b = O.fill_inputs(n, q, 7 + batch, batch)
    a[1] = q - 1
    b[2] = 0; b[2, n - 1] = 1                        # multiply by x^(n-1)
    return a, b


@pytest.mark.parametrize("n,q", D.U64_MULTIPASS)
def test_multipass_products_in_u64_words(n, q, torch_cuda):
    """n > 4096, q < 2^32, u64 words: k_cols_fwd<A,u64,L1> reads and k_cols_inv<A,u64,L1> writes
    8-byte words around 4-byte scratch.  The result is the oracle's, and equals the u32 call's
    widened to u64 (so every upper half is zero); the library names the u64 column kernels, and
    those are kernels of the loaded code object."""
    P = O.Plan(n, q)
    ctx = nttmul.Context(n, q)
    a, b = _edge_operands(n, q)
    c64 = ctx.multiply(a, b, dtype=np.uint64)
    assert c64.dtype == np.uint64
    assert np.array_equal(c64, P.product_batch(a, b)[0].reshape(3, n))
    c32 = ctx.multiply(a.astype(np.uint32), b.astype(np.uint32))
    assert c32.dtype == np.uint32 and np.array_equal(c64, c32.astype(np.uint64))
    A, L1 = D.arith_class(q), n.bit_length() - 13
    name = ctx.kernel_name(64)
    assert name == (f"k_cols_fwd<{A},u64,{L1}> + k_rows<{A},u32,u32,12,{L1}> + "
                    f"k_cols_inv<{A},u64,{L1}>")
    assert list(nttmul.dispatched_kernel_hashes(name)) == \
        D.kernels_of(D.Case("multiply", n, q, 64, 3))


@pytest.mark.parametrize("n,q", D.U64_FUSED)
def test_fused_products_in_u64_words(n, q, torch_cuda):
    """n <= 4096 in u64 words, n = 512 and 2048 included (k_rows<A,u64,u64,LOGS,0>: the generic
    load path instead of the u32 buffer loads), at the ends of the Arith32P3 range and on the
    full-word modulus; launch path on both sides (small_server = -1)."""
    P = O.Plan(n, q)
    ctx = nttmul.Context(n, q, small_server=-1)
    a, b = _edge_operands(n, q)
    c64 = ctx.multiply(a, b, dtype=np.uint64)
    for i in range(3):
        assert np.array_equal(c64[i], P.product_merged(a[i], b[i])), i
    c32 = ctx.multiply(a.astype(np.uint32), b.astype(np.uint32))
    assert np.array_equal(c64, c32.astype(np.uint64))
    assert [nttmul.dispatch_key(ctx.kernel_name(64, 3))] == \
        D.kernels_of(D.Case("multiply", n, q, 64, 3))


# ---------------------------------------------------------------------------------------------
# 1b. every transform mode and pointwise, every size, every class, both word widths
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q,cyclic", D.XF_SWEEP)
def test_transform_modes_every_size_and_word(n, q, cyclic, torch_cuda):
    """nttmul_transform_* in all six (direction, order, scaling) modes and nttmul_pointwise_*, at
    every power of two 256 .. 65536 (512, 2048 and 32768 are run by no other test), one modulus
    per arithmetic class negacyclic and cyclic (three more moduli, the seeded 33-bit prime among
    them, at the three new sizes), in the native word and in u64 where q < 2^32.
    Batch 3: with two polynomials per thread group (dispatch_cases.xform_upg, 32-bit arithmetic
    up to n = 4096) the last group holds one; row 0 random, row 1 all q - 1, row 2 a unit impulse
    at n - 1.  Batch 1: the first group is the ragged one."""
    P = O.Plan(n, q)
    ctx = nttmul.Context(n, q, psi=P.omega if cyclic else 0, cyclic=cyclic)
    x, y = O.fill_inputs(n, q, 21, 3)
    x[1] = q - 1
    y[1] = q - 1
    x[2] = 0; x[2, n - 1] = 1
    exp = {m: np.stack([_xf_expected(P, x[i], m, cyclic, n, q) for i in range(3)])
           for m in D.XF_MODES}
    pw = _mulmod_rows(x, y, q)
    for bits in D.word_options(q):
        dt = np.uint32 if bits == 32 else np.uint64
        for batch in D.XF_SWEEP_BATCHES:
            xs, ys = x[:batch].astype(dt), y[:batch].astype(dt)
            for m in D.XF_MODES:
                got = _guarded_host(ctx, "nttmul_transform_batch", dt, xs, mode=m)
                assert got.dtype == dt
                assert np.array_equal(got.astype(np.uint64), exp[m][:batch]), (bits, batch, m)
            got = _guarded_host(ctx, "nttmul_pointwise_batch", dt, xs, ys)
            assert np.array_equal(got.astype(np.uint64), pw[:batch]), (bits, batch, "pointwise")


# ---------------------------------------------------------------------------------------------
# 1c. device path
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q,batch", D.U64_DEVICE)
def test_device_path_in_u64_words(n, q, batch, torch_cuda):
    """torch.int64 device buffers on a 32-bit modulus: k_fill<u64> gives the oracle's inputs, the
    product is the oracle's for the whole batch, inverse(pointwise(forward a, forward b)) is that
    product, and the forward and reordered outputs equal the oracle transform row by row."""
    torch = torch_cuda
    P = O.Plan(n, q)
    ctx = nttmul.Context(n, q)
    # every buffer is an output of some call, between sentinel guards and 8-byte aligned only
    # (tests/guarded.py); that a and b stay what the fill wrote is part of _check_whole_batch
    names = ("a", "b", "c", "fa", "fb", "pw", "c2", "r")
    arena = G.DeviceArena(torch, 64, G.guard_words(n), **{k: batch * n for k in names})
    a, b, c, fa, fb, pw, c2, r = (arena[k] for k in names)
    s = torch.cuda.current_stream().cuda_stream
    ctx.fill_random_device(a, b, 0, batch, 64, stream=s)
    ctx.multiply_device(c, a, b, batch, 64, stream=s)
    assert ctx.last_kernel_name() == ctx.kernel_name(64, batch) != ""
    assert [nttmul.dispatch_key(k) for k in ctx.last_kernel_name().split("+")] == \
        D.kernels_of(D.Case("multiply", n, q, 64, batch))
    ctx.forward_device(fa, a, batch, 64, stream=s)
    ctx.forward_device(fb, b, batch, 64, stream=s)
    ctx.pointwise_device(pw, fa, fb, batch, 64, stream=s)
    ctx.inverse_device(c2, pw, batch, 64, stream=s)
    ctx.transform_device(r, a, nttmul.XF_REV2STD, batch, 64, stream=s)
    torch.cuda.synchronize()
    arena.check()
    assert _check_whole_batch(n, q, 64, 0, batch, a, b, c) == batch
    assert torch.equal(c2, c)
    ha, hfa, hfb, hpw, hr = (_as_np(t, 64).reshape(batch, n) for t in (a, fa, fb, pw, r))
    for i in range(batch):
        assert np.array_equal(hfa[i], _xf_expected(P, ha[i], 0, False, n, q)), i
        assert np.array_equal(hr[i], _xf_expected(P, ha[i], 2, False, n, q)), i
    assert np.array_equal(hpw, _mulmod_rows(hfa, hfb, q))


# ---------------------------------------------------------------------------------------------
# 1d. range validation
# ---------------------------------------------------------------------------------------------

def _expect_erange(fn, *args, **kw):
    with pytest.raises(nttmul.NttmulError) as ei:
        fn(*args, **kw)
    assert ei.value.status == nttmul.NTTMUL_ERANGE


@pytest.mark.parametrize("n,q", D.VALIDATE)
def test_validate_flag_in_u64_words_host(n, q, torch_cuda):
    """NTTMUL_FLAG_VALIDATE on u64 words against a 32-bit q (k_check_range<u64>), host path: a
    coefficient of exactly 2^32 (low half 0: a check after truncation would accept it), of
    q + 2^32 and of q is NTTMUL_ERANGE wherever it sits -- a or b of multiply, the operand of
    forward and inverse, b of pointwise -- and the same buffers restored succeed and are exact.
    The q-valued coefficient also in u32 words for forward and pointwise."""
    P = O.Plan(n, q)
    ctx = nttmul.Context(n, q, validate=True)
    a, b = O.fill_inputs(n, q, 0, 2)
    u64 = np.uint64
    for k, bad in enumerate((1 << 32, q + (1 << 32), q)):
        pos = (1, n - 1) if k == 0 else (0, 5)       # the batch's last word, and an early one
        keep_a, keep_b = a[pos], b[pos]
        a[pos] = bad
        _expect_erange(ctx.multiply, a, b, dtype=u64)
        _expect_erange(ctx.forward, a, dtype=u64)
        _expect_erange(ctx.inverse, a, dtype=u64)
        a[pos] = keep_a
        b[pos] = bad
        _expect_erange(ctx.multiply, a, b, dtype=u64)
        _expect_erange(ctx.pointwise, a, b, dtype=u64)
        b[pos] = keep_b
    assert np.array_equal(ctx.multiply(a, b, dtype=u64), P.product_batch(a, b)[0].reshape(2, n))
    fa = ctx.forward(a, dtype=u64)
    for i in range(2):
        assert np.array_equal(fa[i], _xf_expected(P, a[i], 0, False, n, q))
    assert np.array_equal(ctx.inverse(fa, dtype=u64), a)
    assert np.array_equal(ctx.pointwise(a, b, dtype=u64), _mulmod_rows(a, b, q))
    a32, b32 = a.astype(np.uint32), b.astype(np.uint32)
    a32[1, 7] = q
    _expect_erange(ctx.forward, a32)
    _expect_erange(ctx.pointwise, b32, a32)
    a32[1, 7] = a[1, 7]
    assert np.array_equal(ctx.forward(a32).astype(u64), fa)
    assert np.array_equal(ctx.pointwise(b32, a32).astype(u64), _mulmod_rows(a, b, q))


@pytest.mark.parametrize("n,q", D.VALIDATE)
def test_validate_flag_in_u64_words_device(n, q, torch_cuda):
    """The same on the device path (torch.int64 buffers): each bad coefficient is refused by
    multiply_device, forward_device, inverse_device and pointwise_device, and the restored
    buffers give the oracle's product."""
    torch = torch_cuda
    ctx = nttmul.Context(n, q, validate=True)
    a = torch.empty(2 * n, dtype=torch.int64, device="cuda")
    b, c = torch.empty_like(a), torch.empty_like(a)
    s = torch.cuda.current_stream().cuda_stream
    ctx.fill_random_device(a, b, 0, 2, 64, stream=s)
    torch.cuda.synchronize()
    for k, bad in enumerate((1 << 32, q + (1 << 32), q)):
        pos = 2 * n - 1 if k == 0 else 5
        keep_a, keep_b = int(a[pos]), int(b[pos])
        a[pos] = bad
        _expect_erange(ctx.multiply_device, c, a, b, 2, 64, stream=s)
        _expect_erange(ctx.forward_device, c, a, 2, 64, stream=s)
        _expect_erange(ctx.inverse_device, c, a, 2, 64, stream=s)
        a[pos] = keep_a
        b[pos] = bad
        _expect_erange(ctx.multiply_device, c, a, b, 2, 64, stream=s)
        _expect_erange(ctx.pointwise_device, c, a, b, 2, 64, stream=s)
        b[pos] = keep_b
    ctx.multiply_device(c, a, b, 2, 64, stream=s)
    torch.cuda.synchronize()
    assert _check_whole_batch(n, q, 64, 0, 2, a, b, c) == 2


# ---------------------------------------------------------------------------------------------
# 1e. host path, several chunks
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pinned", [False, True])
def test_host_path_chunks_in_u64_words(pinned, torch_cuda):
    """600 products of n = 4096 in u64 words on q < 2^31: three 8 MiB chunks (256 + 256 + 88)
    over the pipeline slots, pageable (staged, path 0) and page-locked (direct DMA, path 1).
    Every product equals the oracle's; forward and inverse take the same chunked path."""
    n, q, batch = D.U64_HOST_CHUNKS
    P = O.Plan(n, q)
    ctx = nttmul.Context(n, q)
    a, b = O.fill_inputs(n, q, 41, batch)
    a[batch - 1] = q - 1
    if pinned:
        ap, bp, out = (nttmul.host_empty((batch, n), np.uint64) for _ in range(3))
        ap[...] = a
        bp[...] = b
        out[...] = 0
        assert ctx.multiply(ap, bp, dtype=np.uint64, out=out) is out
        c = out
    else:
        c = ctx.multiply(a, b, dtype=np.uint64)
    assert ctx.last_host_path() == (1 if pinned else 0)
    assert np.array_equal(c, P.product_batch(a, b)[0].reshape(batch, n))
    fa = ctx.forward(a, dtype=np.uint64)
    for i in (0, 255, 256, 511, 512, batch - 1):             # both ends of every chunk
        assert np.array_equal(fa[i], _xf_expected(P, a[i], 0, False, n, q)), i
    assert np.array_equal(ctx.inverse(fa, dtype=np.uint64), a)
