"""GPU parity of ModDown on NTT-domain limbs (include/nttmul_mdntt.h, lib/libnttmul_mdntt.so,
csrc/mdntt_dev.hpp k_mdntt_*): two launches per sub-batch up to n = 4096, four above.

Every case is compared bit for bit, on every output word and at every degree, with the CPU
reference (tests/full_ref.py over tests/mdntt_ref.py and the oracle's transforms), which shares no
code with the device; and beside it with the device composition it replaces -- inverse over Q u P
(nttmul.RnsHoistContext / RnsMpHoistContext), KeySwitchBasis.moddown, forward over Q -- which says
which side is wrong when the two disagree.  Every output is preset to
the sentinel in a guarded arena (tests/guarded.py).  The shapes are the smallest at which the
kernels can go wrong (tests/mdntt_cases.py).  Any canonical vector is a transform of something, so
the inputs are seeded canonical words."""
from math import prod

import numpy as np
import pytest

import bconv_ref as B
import full_ref as F
import guarded as G
import mdntt_cases as C
import mdntt_ref as ref
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


def _to_dev(torch, x, bits):
    x = np.ascontiguousarray(x, dtype=_dt(bits))
    return torch.from_numpy(x.view(np.int32 if bits == 32 else np.int64).reshape(-1)).cuda()


def _from_dev(t, bits, shape):
    return t.cpu().numpy().view(_dt(bits)).reshape(shape)


def _hoist_ctx(n):
    return nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext


def _compose(torch, n, q, p, x_hat):
    """forward_Q(ks_moddown(inverse_{Q u P}(x_hat))) on the device, three calls."""
    bits, batch, L, M = 8 * x_hat.dtype.itemsize, x_hat.shape[0], len(q), len(q) + len(p)
    Ctx = _hoist_ctx(n)
    tdt = torch.int32 if bits == 32 else torch.int64
    with Ctx(n, q + p) as ext, Ctx(n, q) as low, nttmul.KeySwitchBasis(n, q, p, 1) as ks:
        dx = _to_dev(torch, x_hat, bits)
        coef = torch.empty(batch * M * n, dtype=tdt, device="cuda")
        down = torch.empty(batch * L * n, dtype=tdt, device="cuda")
        out = torch.empty(batch * L * n, dtype=tdt, device="cuda")
        ext.inverse_device(coef, dx, batch)
        ks.moddown_device(down, coef, batch)
        low.forward_device(out, down, batch)
        torch.cuda.synchronize()
        return _from_dev(out, bits, (batch, L, n))


def _call(torch, md, x_hat, stream=0):
    """One device call on a numpy operand, out of a guarded arena: both operands between sentinel
    guards, aligned to their word only, the output preset to the sentinel; after the call no guard
    word and no input word has changed and every output word is written."""
    bits, batch = md.word_bits, x_hat.shape[0]
    shape = (batch, md.q_limbs, md.n)
    arena = G.DeviceArena(torch, bits, G.guard_words((md.q_limbs + md.p_limbs) * md.n),
                          out=int(np.prod(shape)), x=x_hat)
    md.moddown_device(arena["out"], arena["x"], batch, stream=stream)
    torch.cuda.synchronize()
    arena.check()
    return arena.get("out", shape)


def _input(case, seed):
    q, p = C.moduli_of(case)
    return B.random_words(np.random.default_rng(seed), q + p, case.batch, case.n, _dt(case.bits))


def _want(x_hat, q, p):
    """The CPU reference of every output word."""
    return F.reference("mdntt", "moddown", x_hat, q, p)


def _id(case):
    return f"u{case.bits}-n{case.n}x{case.batch}-{case.L}.{case.K}" + \
        ("-small" if case.moduli else "")


@pytest.mark.parametrize("case", C.parity_cases(), ids=_id)
def test_parity(case, torch_cuda):
    """Grid and pairs (batch 3 and 33), the limb counts, K over the fold cadence (the P part of a
    batch-1 input at n = 256 is the transform of the conversion's worst case, every y_j = p_j - 1
    at every coefficient), every degree, the small moduli."""
    q, p = C.moduli_of(case)
    x = _input(case, 1000 * case.L + 10 * case.K + case.n)
    if case.batch == 1 and case.n == C.N:
        worst = np.array(B.worst_case(p), dtype=_dt(case.bits))
        flat = np.empty((1, case.K, case.n), dtype=_dt(case.bits))
        flat[0] = worst[:, None]
        x[0, case.L:, :] = ref.forward(flat, p)[0]
    with nttmul.NttModDown(case.n, q, p) as md:
        assert (md.q_limbs, md.p_limbs, md.word_bits) == (case.L, case.K, case.bits)
        assert (md.info.n, 1 << md.info.logn, md.info.ndev, md.info.scratch_mb) == \
            (case.n, case.n, 1, C.DEFAULT_SCRATCH_MB)
        got = _call(torch_cuda, md, x)
    assert np.array_equal(got, _compose(torch_cuda, case.n, q, p, x))
    F.assert_equal(got, _want(x, q, p), _id(case))


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n", C.RANGE_N)
@pytest.mark.parametrize("fill", C.RANGE_FILLS)
def test_worst_case_ranges(fill, n, bits, torch_cuda):
    """Every word at its modulus - 1; a zero P part, where out = x_hat P^-1 limb by limb; a zero
    Q part."""
    L, K = C.RANGE_SHAPE
    case = C.Case(bits, n, 2, L, K)
    q, p = C.moduli_of(case)
    ext = q + p
    x = _input(case, n + bits)
    if fill == "top":
        for l, m in enumerate(ext):
            x[:, l, :] = m - 1
    elif fill == "zero_p":
        x[:, L:, :] = 0
    else:
        x[:, :L, :] = 0
    with nttmul.NttModDown(n, q, p) as md:
        got = _call(torch_cuda, md, x)
    assert np.array_equal(got, _compose(torch_cuda, n, q, p, x))
    if fill == "zero_p":
        P = prod(int(v) for v in p)
        for l, m in enumerate(q):
            want = (x[:, l, :].astype(object) * pow(P, -1, m) % m).astype(_dt(bits))
            assert np.array_equal(got[:, l, :], want), l
    F.assert_equal(got, _want(x, q, p), (fill, n, bits))


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,L", C.RESCALE)
def test_rescale_is_the_exact_floor(n, L, bits, torch_cuda):
    """K = 1: the inverse transform of out is floor(X / p) mod q_l for random big integers X in
    [0, Q p), the ends of the range among them; and out itself is the CPU reference's, word for
    word."""
    torch = torch_cuda
    batch = C.RESCALE_BATCH
    case = C.Case(bits, n, batch, L, 1)
    q, p = C.moduli_of(case)
    ext = q + p
    bound = prod(int(v) for v in ext)
    rng = np.random.default_rng(n * L + bits)
    X = [ref.big_integers(rng, n, bound) for _ in range(batch)]
    x = np.stack([ref.residues(Xb, ext, _dt(bits)) for Xb in X])
    Ctx = _hoist_ctx(n)
    with Ctx(n, ext) as big, Ctx(n, q) as low, nttmul.NttModDown(n, q, p) as md:
        x_hat = big.forward(x)
        got = _call(torch, md, x_hat)
        back = low.inverse(got)
    assert np.array_equal(x_hat, ref.forward(x, ext))
    F.assert_equal(got, _want(x_hat, q, p), (n, L, bits))
    for b in range(batch):
        assert np.array_equal(back[b].astype(object), ref.rescale_floor(X[b], q, p[0])), b


def test_sub_batches_and_two_streams(torch_cuda):
    """scratch_mb = 1: three sub-batches with a partial last one at n = 4096, one polynomial each
    at n = 65536; then, on the grown scratch, two calls on two streams with no synchronisation
    between them."""
    torch = torch_cuda
    for case, (*_, want) in zip(C.subbatch_cases(), C.SUBBATCH):
        assert C.chunks(case) == list(want) and len(want) == 3
        q, p = C.moduli_of(case)
        with nttmul.NttModDown(case.n, q, p, scratch_mb=1) as md:
            assert md.info.scratch_mb == 1
            small = _input(case._replace(batch=1), 3)
            got = _call(torch, md, small)
            assert np.array_equal(got, _compose(torch, case.n, q, p, small))
            F.assert_equal(got, _want(small, q, p), (case, "one polynomial"))
            x = _input(case, 4)                 # the scratch grows to a whole sub-batch
            want_x = _compose(torch, case.n, q, p, x)
            assert np.array_equal(_call(torch, md, x), want_x)
            F.assert_equal(want_x, _want(x, q, p), (case, "sub-batches"))
            y = _input(case, 5)
            want_y = _compose(torch, case.n, q, p, y)
            F.assert_equal(want_y, _want(y, q, p), (case, "second stream"))
            tdt = torch.int64
            dx, dy = _to_dev(torch, x, 64), _to_dev(torch, y, 64)
            ox = torch.empty(want_x.size, dtype=tdt, device="cuda")
            oy = torch.empty(want_y.size, dtype=tdt, device="cuda")
            torch.cuda.synchronize()
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            md.moddown_device(ox, dx, case.batch, stream=s1.cuda_stream)
            md.moddown_device(oy, dy, case.batch, stream=s2.cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(_from_dev(ox, 64, want_x.shape), want_x)
            assert np.array_equal(_from_dev(oy, 64, want_y.shape), want_y)


@pytest.mark.parametrize("bits", (32, 64))
def test_validate_flag_checks_each_word_against_its_own_limb(bits, torch_cuda):
    """A word equal to its own limb's modulus (in range for the limb before it: the primes
    descend) is NTTMUL_ERANGE and out is untouched; a clean input succeeds; without the flag there
    is no check."""
    torch = torch_cuda
    n, batch, (L, K) = C.VALIDATE
    q, p = C.moduli_of(C.Case(bits, n, batch, L, K))
    ext = q + p
    assert all(a > b for a, b in zip(ext, ext[1:]))
    good = _input(C.Case(bits, n, batch, L, K), 9)
    with nttmul.NttModDown(n, q, p, validate=True) as strict, nttmul.NttModDown(n, q, p) as lax:
        want = _compose(torch, n, q, p, good)
        assert np.array_equal(_call(torch, strict, good), want)
        F.assert_equal(want, _want(good, q, p), bits)
        for limb in (1, L + K - 1):
            bad = good.copy()
            bad[batch - 1, limb, n - 1] = ext[limb]
            out = torch.full((batch * L * n,), -1, dtype=torch.int32 if bits == 32 else torch.int64,
                             device="cuda")
            with pytest.raises(nttmul.NttmulError) as ei:
                strict.moddown_device(out, _to_dev(torch, bad, bits), batch)
            assert ei.value.status == nttmul.NTTMUL_ERANGE, limb
            torch.cuda.synchronize()
            assert bool((out == -1).all())
            _call(torch, lax, bad)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,batch", C.HOST)
def test_host_form_equals_the_device_form(n, batch, bits, torch_cuda):
    L, K = C.HOST_SHAPE
    case = C.Case(bits, n, batch, L, K)
    q, p = C.moduli_of(case)
    x = _input(case, 77)
    with nttmul.NttModDown(n, q, p) as md:
        assert md.io_dtype == _dt(bits)
        dev = _call(torch_cuda, md, x)
        host = md.moddown(x)
        assert host.dtype == _dt(bits) and np.array_equal(host, dev)
        assert md.moddown(x[:0]).shape == (0, L, n)
        with pytest.raises(ValueError):
            md.moddown(np.zeros((1, L, n), dtype=_dt(bits)))
    assert np.array_equal(dev, _compose(torch_cuda, n, q, p, x))
    F.assert_equal(dev, _want(x, q, p), (n, batch, bits))


def test_device_path_rules(torch_cuda):
    """A non-default stream; the empty batch; bad arguments on a live context."""
    torch = torch_cuda
    L, K = 3, 2
    case = C.Case(32, C.N, 3, L, K)
    q, p = C.moduli_of(case)
    with nttmul.NttModDown(C.N, q, p) as md:
        side = torch.cuda.Stream()
        x = _input(case, 5)
        got = _call(torch, md, x, stream=side.cuda_stream)
        F.assert_equal(got, _want(x, q, p))
        out = torch.full((C.N,), 7, dtype=torch.int32, device="cuda")
        md.moddown_device(out, out, 0)                               # batch = 0: a no-op
        torch.cuda.synchronize()
        assert bool((out == 7).all())
        fn = md._lib.nttmul_mdntt_moddown_device
        assert fn(md._h, None, out.data_ptr(), 1, 0, None) == nttmul.NTTMUL_EINVAL
        assert fn(md._h, out.data_ptr(), None, 1, 0, None) == nttmul.NTTMUL_EINVAL
        assert fn(md._h, None, None, 0, 0, None) == nttmul.NTTMUL_OK
        assert fn(md._h, out.data_ptr(), out.data_ptr(), 1, 99, None) == nttmul.NTTMUL_ENODEV
        host = md._lib.nttmul_mdntt_moddown
        assert host(md._h, None, None, 0) == nttmul.NTTMUL_OK
        assert host(md._h, None, out.data_ptr(), 1) == nttmul.NTTMUL_EINVAL
        with pytest.raises(ValueError):                              # too small a tensor
            md.moddown_device(out, out, 2)
        assert md._lib.nttmul_mdntt_kernel_name(md._h, None, 1) == nttmul.NTTMUL_EINVAL
        assert md._lib.nttmul_mdntt_kernel_name(md._h, None, 0) == len(C.kernel_name(C.N, 32))


def test_mirror_agrees_with_the_library_dispatch(torch_cuda):
    """tests/mdntt_cases.py kernel_name against nttmul_mdntt_kernel_name at every degree, and the
    names are kernels the library holds."""
    held = nttmul.kernel_hashes(nttmul.MDNTT_LIB_PATH)
    for bits in (32, 64):
        for n in C.ALL_N:
            q, p = C.moduli_of(C.Case(bits, n, 1, 2, 1))
            with nttmul.NttModDown(n, q, p) as md:
                name = md.kernel_name()
                assert name == C.kernel_name(n, bits)
                for part in name.split(" + "):
                    assert nttmul.dispatch_key(part) in held
