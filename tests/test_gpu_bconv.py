"""GPU parity of the base-conversion calls (include/nttmul_bconv.h, lib/libnttmul_bconv.so,
csrc/bconv_dev.hpp k_bconv): convert and moddown, one launch each over [batch][limbs][n] operands.

Every comparison is bit-exact against tests/bconv_ref.py (Python integers).  The shapes are the
smallest at which the kernel can go wrong (tests/bconv_cases.py): n = 256 with batch 3 leaves a
partial last workgroup and puts several polynomials into one; K runs over both sides of the
target-limb tile; L runs over both sides of each accumulator cadence and over the lengths at which
an unfolded sum overflows, on the all-y_i = b_i - 1 input."""
from math import prod

import numpy as np
import pytest

import bconv_cases as B
import bconv_ref as R
import guarded as G
import nttmul

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _call(torch, conv, op, x, stream=0):
    """One device call on a numpy operand, out of a guarded arena (tests/guarded.py: both operands
    between sentinel guards, aligned to their word only; after the call no guard word and no
    input word has changed and every output word is written); returns (result, the operand after
    the call)."""
    bits, batch = conv.word_bits, x.shape[0]
    arena = G.DeviceArena(torch, bits, G.guard_words(x.size // batch),
                          out=batch * conv.to_limbs * conv.n, x=x)
    out, dx = arena["out"], arena["x"]
    getattr(conv, f"{op}_device")(out, dx, batch, stream=stream)
    torch.cuda.synchronize()
    arena.check()
    return arena.get("out", (batch, conv.to_limbs, conv.n)), arena.get("x", x.shape)


def _input(op, bits, from_q, to_q, batch, n, seed):
    """Seeded canonical words for op: [batch, L, n], or [batch, K + L, n] for moddown."""
    moduli = tuple(from_q) if op == "convert" else tuple(to_q) + tuple(from_q)
    return R.random_words(np.random.default_rng(seed), moduli, batch, n, _dt(bits))


def _expect(op, x, from_q, to_q):
    return (R.convert if op == "convert" else R.moddown)(x, from_q, to_q)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("op", B.OPS)
@pytest.mark.parametrize("L,K", B.SHAPES)
def test_parity(L, K, op, bits, torch_cuda):
    from_q, to_q = B.bases(bits, L, K)
    x = _input(op, bits, from_q, to_q, B.BATCH, B.N, 100 * L + K)
    with nttmul.BaseConverter(B.N, from_q, to_q) as conv:
        assert (conv.from_limbs, conv.to_limbs, conv.word_bits) == (L, K, bits)
        got, after = _call(torch_cuda, conv, op, x)
    assert np.array_equal(after, x)
    assert np.array_equal(got, _expect(op, x, from_q, to_q))


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("op", B.OPS)
def test_parity_at_the_largest_n(op, bits, torch_cuda):
    L, K = B.BIG_SHAPE
    from_q, to_q = B.bases(bits, L, K)
    x = _input(op, bits, from_q, to_q, B.BIG_BATCH, B.BIG_N, 4096)
    with nttmul.BaseConverter(B.BIG_N, from_q, to_q) as conv:
        got, _ = _call(torch_cuda, conv, op, x)
    assert np.array_equal(got, _expect(op, x, from_q, to_q))


@pytest.mark.parametrize("bits,L", [(b, L) for b in (32, 64) for L in B.CADENCE_L[b]])
def test_accumulator_cadence(bits, L, torch_cuda):
    """Every coefficient of the first half holds the worst-case vector (every y_i = b_i - 1), the
    second half random words; convert and moddown."""
    from_q, to_q = B.bases(bits, L, B.CADENCE_K)
    n, K = B.N, B.CADENCE_K
    x = _input("moddown", bits, from_q, to_q, 1, n, L)
    x[0, K:, :n // 2] = np.array(R.worst_case(from_q), dtype=_dt(bits))[:, None]
    with nttmul.BaseConverter(n, from_q, to_q) as conv:
        got, _ = _call(torch_cuda, conv, "convert", np.ascontiguousarray(x[:, K:, :]))
        down, _ = _call(torch_cuda, conv, "moddown", x)
    want = R.convert(x[:, K:, :], from_q, to_q)
    assert np.array_equal(got, want)
    # the worst case is x + (L - 1) B: alpha at its maximum
    B_, v = prod(from_q), R.crt(R.worst_case(from_q), from_q)
    assert [int(got[0, j, 0]) for j in range(K)] == [(v + (L - 1) * B_) % c for c in to_q]
    assert np.array_equal(down, R.moddown(x, from_q, to_q))


@pytest.mark.parametrize("op", B.OPS)
@pytest.mark.parametrize("split", (1, 2))
def test_small_moduli(split, op, torch_cuda):
    """7681, 12289 and 786433 on 32-bit words, both directions."""
    from_q, to_q = B.SMALL[:split], B.SMALL[split:]
    for f, t in ((from_q, to_q), (to_q, from_q)):
        x = _input(op, 32, f, t, B.BATCH, B.N, 7681 + split)
        x[0, -len(f):, 0] = np.array(R.worst_case(f), dtype=np.uint32)
        with nttmul.BaseConverter(B.N, f, t) as conv:
            got, _ = _call(torch_cuda, conv, op, x)
        assert np.array_equal(got, _expect(op, x, f, t))


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("L", B.EXACT_L)
def test_moddown_is_exact_on_multiples_and_for_one_limb(L, bits, torch_cuda):
    """X = B Z with Z random below C comes back as Z's residues, for any L; for L = 1 and random X
    moddown is floor(X / b_0) mod c_j."""
    K, n, batch = 3, B.N, B.BATCH
    from_q, to_q = B.bases(bits, L, K)
    Bp, C = prod(from_q), prod(to_q)
    rng = np.random.default_rng(bits + L)
    def residues(X):
        return [X % c for c in to_q] + [X % b for b in from_q]
    Z = [[int.from_bytes(rng.bytes(32), "little") % C for _ in range(n)] for _ in range(batch)]
    x = np.array([[residues(Bp * z) for z in row] for row in Z], dtype=object)
    x = np.ascontiguousarray(x.transpose(0, 2, 1)).astype(_dt(bits))
    with nttmul.BaseConverter(n, from_q, to_q) as conv:
        got, _ = _call(torch_cuda, conv, "moddown", x)
        for p in range(batch):
            for j, c in enumerate(to_q):
                assert [int(v) for v in got[p, j]] == [z % c for z in Z[p]]
        if L == 1:
            X = [[int.from_bytes(rng.bytes(40), "little") % (Bp * C) for _ in range(n)]
                 for _ in range(batch)]
            x = np.array([[residues(v) for v in row] for row in X], dtype=object)
            x = np.ascontiguousarray(x.transpose(0, 2, 1)).astype(_dt(bits))
            got, _ = _call(torch_cuda, conv, "moddown", x)
            for p in range(batch):
                for j, c in enumerate(to_q):
                    assert [int(v) for v in got[p, j]] == [(v // Bp) % c for v in X[p]]


@pytest.mark.parametrize("bits", (32, 64))
def test_moddown_is_the_composition_of_convert(bits, torch_cuda):
    """moddown equals this library's own convert output, subtracted and multiplied by binv in
    Python integers."""
    L, K = 5, 3
    from_q, to_q = B.bases(bits, L, K)
    x = _input("moddown", bits, from_q, to_q, B.BATCH, B.N, 53)
    _, _, binv = nttmul.bconv_plan(B.N, from_q, to_q)
    with nttmul.BaseConverter(B.N, from_q, to_q) as conv:
        conv_out, _ = _call(torch_cuda, conv, "convert", np.ascontiguousarray(x[:, K:, :]))
        down, _ = _call(torch_cuda, conv, "moddown", x)
    for j, c in enumerate(to_q):
        want = (x[:, j, :].astype(object) - conv_out[:, j, :].astype(object)) * binv[j] % c
        assert np.array_equal(down[:, j, :].astype(object), want)


@pytest.mark.parametrize("bits", (32, 64))
def test_validate_flag_checks_each_word_against_its_own_limb(bits, torch_cuda):
    """A word equal to its own limb's modulus but below a neighbour's is NTTMUL_ERANGE in either
    operation; without the flag the call succeeds."""
    from_q, to_q = B.bases(bits, 2, 2)                  # descending primes: from_q[1] < from_q[0]
    assert from_q[1] < from_q[0] and to_q[1] < to_q[0] < from_q[1]
    n, batch = B.N, 2
    with nttmul.BaseConverter(n, from_q, to_q, validate=True) as strict, \
            nttmul.BaseConverter(n, from_q, to_q) as lax:
        for op in B.OPS:
            good = _input(op, bits, from_q, to_q, batch, n, 9)
            got, _ = _call(torch_cuda, strict, op, good)
            assert np.array_equal(got, _expect(op, good, from_q, to_q))
            spots = [(good.shape[1] - 1, from_q[1])] + ([(1, to_q[1])] if op == "moddown" else [])
            for limb, q in spots:
                bad = good.copy()
                bad[1, limb, n - 1] = q                 # in range for limb - 1, not for its own
                with pytest.raises(nttmul.NttmulError) as ei:
                    _call(torch_cuda, strict, op, bad)
                assert ei.value.status == nttmul.NTTMUL_ERANGE, (op, limb)
                _call(torch_cuda, lax, op, bad)         # no flag, no check


@pytest.mark.parametrize("bits", (32, 64))
def test_host_forms_equal_the_device_forms(bits, torch_cuda):
    L, K = B.HOST[bits]
    from_q, to_q = B.bases(bits, L, K)
    with nttmul.BaseConverter(B.N, from_q, to_q) as conv:
        assert conv.io_dtype == _dt(bits)
        for op in B.OPS:
            x = _input(op, bits, from_q, to_q, B.BATCH, B.N, 77)
            dev, _ = _call(torch_cuda, conv, op, x)
            host = getattr(conv, op)(x)
            assert host.dtype == _dt(bits) and np.array_equal(host, dev)
            assert np.array_equal(host, _expect(op, x, from_q, to_q))
            assert getattr(conv, op)(x[:0]).shape == (0, K, B.N)
        with pytest.raises(ValueError):
            conv.convert(np.zeros((1, L + 1, B.N), dtype=_dt(bits)))


def test_device_path_rules(torch_cuda):
    """A non-default stream; the empty batch; bad arguments on a live converter."""
    torch = torch_cuda
    from_q, to_q = B.bases(32, 2, 1)
    with nttmul.BaseConverter(B.N, from_q, to_q) as conv:
        side = torch.cuda.Stream()
        for op in B.OPS:
            x = _input(op, 32, from_q, to_q, B.BATCH, B.N, 5)
            got, _ = _call(torch, conv, op, x, stream=side.cuda_stream)
            assert np.array_equal(got, _expect(op, x, from_q, to_q))
            out = torch.full((B.N,), 7, dtype=torch.int32, device="cuda")
            getattr(conv, f"{op}_device")(out, out, 0)                 # batch = 0: a no-op
            torch.cuda.synchronize()
            assert bool((out == 7).all())
            fn = getattr(conv._lib, f"nttmul_bconv_{op}_device")
            assert fn(conv._h, None, out.data_ptr(), 1, 0, None) == nttmul.NTTMUL_EINVAL
            assert fn(conv._h, out.data_ptr(), None, 1, 0, None) == nttmul.NTTMUL_EINVAL
            assert fn(conv._h, None, None, 0, 0, None) == nttmul.NTTMUL_OK
            assert fn(conv._h, out.data_ptr(), out.data_ptr(), 1, 99, None) == nttmul.NTTMUL_ENODEV
            with pytest.raises(ValueError):                            # too small a tensor
                getattr(conv, f"{op}_device")(out, out, 2)
        assert conv._lib.nttmul_bconv_kernel_name(conv._h, 2, None, 0) == nttmul.NTTMUL_EINVAL
        assert (conv.info.n, conv.info.from_limbs, conv.info.to_limbs, conv.info.ndev) == \
            (B.N, 2, 1, 1)


def test_mirror_agrees_with_the_library_dispatch(torch_cuda):
    """tests/bconv_cases.py bconv_kernel against nttmul_bconv_kernel_name, and the names are
    kernels the library holds."""
    held = nttmul.kernel_hashes(nttmul.BCONV_LIB_PATH)
    for bits in (32, 64):
        for n, (L, K) in ((256, (1, 2)), (1024, (2, 1)), (4096, (3, 5))):
            from_q, to_q = B.bases(bits, L, K)
            with nttmul.BaseConverter(n, from_q, to_q) as conv:
                for op in B.OPS:
                    name = conv.kernel_name(op)
                    assert name == B.bconv_kernel(op, n, bits) == conv.kernel_name(B.OPS.index(op))
                    assert nttmul.dispatch_key(name) in held
