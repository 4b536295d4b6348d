"""GPU parity of the key-switch calls (include/nttmul_ks.h, lib/libnttmul_ks.so, csrc/ks_dev.hpp
k_ks_modup; ModDown on bconv_dev.hpp k_bconv<W,1> up to n = 65536): one launch each.

Every comparison is bit-exact against Python integers (tests/ks_ref.py, tests/bconv_ref.py), and
every output is preset to the sentinel in a guarded arena (tests/guarded.py).  The shapes are the
smallest at which the kernel can go wrong (tests/ks_cases.py): n = 256 with batch 3 leaves a
partial workgroup that holds several polynomials on 32-bit words; (L, K, alpha) runs over even
digits, a short last digit, one digit, dnum = L, and L + K on both sides of the target-limb tile
and at 64; the digit width runs over both sides of each accumulator cadence and over the lengths
at which an unfolded sum overflows, on the all-y_i = q_i - 1 input.

The chain test runs a whole hybrid key switch: modup, mac_ntt (shared, terms = dnum) per key
component through nttmul.RnsContext (n = 256) or nttmul.RnsMpContext (n = 8192), moddown, with a
zero-noise key.  Every stage is bit-exact, and per limb every coefficient of c0 + c1 s - x s' lies
within (K + 1)(1 + h) of 0.  The bound is derived: before ModDown c0 + c1 s = P x s' mod P Q
exactly; each ModDown subtracts r_i = c_i mod P, coefficients in [0, P), and at most K - 1
multiples of P, so after the division by P the error of c_i is in (-K, 0]; r_1 s is a signed sum
of h such terms, r_0 one: (K + 1)(1 + h) covers both with room to spare."""
import numpy as np
import pytest

import bconv_ref as B
import guarded as G
import ks_cases as C
import ks_ref as ref
import nttmul
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _out_shape(ks, op, batch):
    ext = ks.q_limbs + ks.p_limbs
    return (batch, ks.digits, ext, ks.n) if op == "modup" else (batch, ks.q_limbs, ks.n)


def _call(torch, ks, op, x, stream=0):
    """One device call on a numpy operand, out of a guarded arena: both operands between sentinel
    guards, aligned to their word only, the output preset to the sentinel; after the call no guard
    word and no input word has changed and every output word is written."""
    bits, batch = ks.word_bits, x.shape[0]
    shape = _out_shape(ks, op, batch)
    arena = G.DeviceArena(torch, bits, G.guard_words(int(np.prod(shape[1:]))),
                          out=int(np.prod(shape)), x=x)
    getattr(ks, f"{op}_device")(arena["out"], arena["x"], batch, stream=stream)
    torch.cuda.synchronize()
    arena.check()
    return arena.get("out", shape)


def _input(case, seed):
    q, p = C.moduli_of(case)
    moduli = q if case.op == "modup" else q + p
    return B.random_words(np.random.default_rng(seed), moduli, case.batch, case.n, _dt(case.bits))


def _assert_modup(got, x, q, p, alpha):
    assert np.array_equal(got, ref.modup(x, q, p, alpha))
    for d, rng in enumerate(ref.digits(len(q), alpha)):       # own limbs, bit for bit
        assert np.array_equal(got[:, d, rng.start:rng.stop, :], x[:, rng.start:rng.stop, :])


def _id(case):
    return f"u{case.bits}-n{case.n}x{case.batch}-{case.L}.{case.K}.{case.alpha}" + \
        ("-small" if case.moduli else "")


@pytest.mark.parametrize("case", C.modup_cases(), ids=_id)
def test_modup_parity(case, torch_cuda):
    """Grid and tiles, cadence (the first half of a batch-1 input holds the worst case, every
    y_i = q_i - 1, the second half random words), the degrees and the small moduli."""
    q, p = C.moduli_of(case)
    x = _input(case, 1000 * case.L + 10 * case.K + case.alpha)
    if case.batch == 1:
        worst = np.array(ref.worst_case(q, case.alpha), dtype=_dt(case.bits))
        x[0, :, :case.n // 2] = worst[:, None]
    with nttmul.KeySwitchBasis(case.n, q, p, case.alpha) as ks:
        assert (ks.q_limbs, ks.p_limbs, ks.digit_limbs, ks.digits, ks.word_bits) == \
            (case.L, case.K, case.alpha, C.dnum(case), case.bits)
        assert (ks.info.n, 1 << ks.info.logn, ks.info.ndev) == (case.n, case.n, 1)
        got = _call(torch_cuda, ks, "modup", x)
    _assert_modup(got, x, q, p, case.alpha)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,batch", C.MODDOWN)
def test_moddown_above_the_converters_degrees(n, batch, bits, torch_cuda):
    L, K = C.MODDOWN_SHAPE
    case = C.Case("moddown", bits, n, batch, L, K, 1)
    q, p = C.moduli_of(case)
    x = _input(case, n + bits)
    with nttmul.KeySwitchBasis(n, q, p, 1) as ks:
        got = _call(torch_cuda, ks, "moddown", x)
    assert np.array_equal(got, B.moddown(x, p, q))


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,batch", C.MODDOWN_BCONV)
def test_moddown_equals_the_base_converter(n, batch, bits, torch_cuda):
    L, K = C.MODDOWN_SHAPE
    case = C.Case("moddown", bits, n, batch, L, K, 1)
    q, p = C.moduli_of(case)
    x = _input(case, n + bits + 1)
    with nttmul.KeySwitchBasis(n, q, p, 1) as ks, nttmul.BaseConverter(n, p, q) as conv:
        got = _call(torch_cuda, ks, "moddown", x)
        assert np.array_equal(got, conv.moddown(x))
    assert np.array_equal(got, B.moddown(x, p, q))


@pytest.mark.parametrize("bits", (32, 64))
def test_validate_flag_checks_each_word_against_its_own_limb(bits, torch_cuda):
    """A word of the last polynomial equal to its own limb's modulus (in range for the limb before
    it: the primes descend) is NTTMUL_ERANGE; a clean input succeeds; without the flag there is
    no check."""
    n, batch, (L, K, alpha) = C.VALIDATE
    q, p = ref.bases(bits, L, K)
    ext = q + p
    assert all(a > b for a, b in zip(ext, ext[1:]))
    with nttmul.KeySwitchBasis(n, q, p, alpha, validate=True) as strict, \
            nttmul.KeySwitchBasis(n, q, p, alpha) as lax:
        for op in C.OPS:
            good = _input(C.Case(op, bits, n, batch, L, K, alpha), 9)
            got = _call(torch_cuda, strict, op, good)
            if op == "modup":
                _assert_modup(got, good, q, p, alpha)
            else:
                assert np.array_equal(got, B.moddown(good, p, q))
            for limb in {1, good.shape[1] - 1}:
                bad = good.copy()
                bad[batch - 1, limb, n - 1] = ext[limb]
                with pytest.raises(nttmul.NttmulError) as ei:
                    _call(torch_cuda, strict, op, bad)
                assert ei.value.status == nttmul.NTTMUL_ERANGE, (op, limb)
                _call(torch_cuda, lax, op, bad)


@pytest.mark.parametrize("bits", (32, 64))
def test_host_forms_equal_the_device_forms(bits, torch_cuda):
    n, batch, (L, K, alpha) = C.HOST
    q, p = ref.bases(bits, L, K)
    with nttmul.KeySwitchBasis(n, q, p, alpha) as ks:
        assert ks.io_dtype == _dt(bits)
        for op in C.OPS:
            x = _input(C.Case(op, bits, n, batch, L, K, alpha), 77)
            dev = _call(torch_cuda, ks, op, x)
            host = getattr(ks, op)(x)
            assert host.dtype == _dt(bits) and np.array_equal(host, dev)
            if op == "modup":
                _assert_modup(host, x, q, p, alpha)
            else:
                assert np.array_equal(host, B.moddown(x, p, q))
            assert getattr(ks, op)(x[:0]).shape == _out_shape(ks, op, 0)
        with pytest.raises(ValueError):
            ks.modup(np.zeros((1, L + 1, n), dtype=_dt(bits)))
        with pytest.raises(ValueError):
            ks.moddown(np.zeros((1, L, n), dtype=_dt(bits)))


def test_device_path_rules(torch_cuda):
    """A non-default stream; the empty batch; bad arguments on a live context."""
    torch = torch_cuda
    L, K, alpha = 3, 2, 2
    q, p = ref.bases(32, L, K)
    with nttmul.KeySwitchBasis(C.N, q, p, alpha) as ks:
        side = torch.cuda.Stream()
        for op in C.OPS:
            x = _input(C.Case(op, 32, C.N, C.BATCH, L, K, alpha), 5)
            got = _call(torch, ks, op, x, stream=side.cuda_stream)
            want = ref.modup(x, q, p, alpha) if op == "modup" else B.moddown(x, p, q)
            assert np.array_equal(got, want)
            out = torch.full((C.N,), 7, dtype=torch.int32, device="cuda")
            getattr(ks, f"{op}_device")(out, out, 0)                   # batch = 0: a no-op
            torch.cuda.synchronize()
            assert bool((out == 7).all())
            fn = getattr(ks._lib, f"nttmul_ks_{op}_device")
            assert fn(ks._h, None, out.data_ptr(), 1, 0, None) == nttmul.NTTMUL_EINVAL
            assert fn(ks._h, out.data_ptr(), None, 1, 0, None) == nttmul.NTTMUL_EINVAL
            assert fn(ks._h, None, None, 0, 0, None) == nttmul.NTTMUL_OK
            assert fn(ks._h, out.data_ptr(), out.data_ptr(), 1, 99, None) == nttmul.NTTMUL_ENODEV
            host = getattr(ks._lib, f"nttmul_ks_{op}")
            assert host(ks._h, None, None, 0) == nttmul.NTTMUL_OK
            assert host(ks._h, None, out.data_ptr(), 1) == nttmul.NTTMUL_EINVAL
            with pytest.raises(ValueError):                            # too small a tensor
                getattr(ks, f"{op}_device")(out, out, 2)
        assert ks._lib.nttmul_ks_kernel_name(ks._h, 2, None, 0) == nttmul.NTTMUL_EINVAL
        assert ks._lib.nttmul_ks_kernel_name(ks._h, 0, None, 0) == len("k_ks_modup<u32>")


def test_mirror_agrees_with_the_library_dispatch(torch_cuda):
    """tests/ks_cases.py kernel_name against nttmul_ks_kernel_name, and the names are kernels the
    library holds."""
    held = nttmul.kernel_hashes(nttmul.KS_LIB_PATH)
    for bits in (32, 64):
        for n, (L, K, alpha) in ((256, (1, 1, 1)), (4096, (3, 2, 2)), (8192, (4, 2, 2)),
                                 (65536, (5, 3, 5))):
            q, p = ref.bases(bits, L, K)
            with nttmul.KeySwitchBasis(n, q, p, alpha) as ks:
                for op in C.OPS:
                    name = ks.kernel_name(op)
                    assert name == C.kernel_name(op, n, bits) == ks.kernel_name(C.OPS.index(op))
                    assert nttmul.dispatch_key(name) in held


def _to_dev(torch, x, bits):
    x = np.ascontiguousarray(x, dtype=_dt(bits))
    return torch.from_numpy(x.view(np.int32 if bits == 32 else np.int64).reshape(-1)).cuda()


def _from_dev(t, bits, shape):
    return t.cpu().numpy().view(_dt(bits)).reshape(shape)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,kind", C.CHAIN)
def test_hybrid_key_switch_chain(n, kind, bits, torch_cuda):
    torch = torch_cuda
    L, K, alpha = C.CHAIN_SHAPE
    batch, h = C.CHAIN_BATCH, C.CHAIN_H
    q, p = ref.bases(bits, L, K)
    ext, M, dn = q + p, L + K, -(-L // alpha)
    rng = np.random.default_rng(n + bits)
    s, s2 = ref.ternary(rng, n, h), ref.ternary(rng, n, h)
    key = [k.astype(_dt(bits)) for k in ref.keygen(rng, n, q, p, alpha, s, s2)]   # (b, a)
    x = B.random_words(rng, q, batch, n, _dt(bits))
    Mac = nttmul.RnsContext if kind == "rns" else nttmul.RnsMpContext
    sentinel = int(G.sentinel(bits)) - (1 << bits)              # all bits set, as a signed word
    tdt = torch.int32 if bits == 32 else torch.int64
    with nttmul.KeySwitchBasis(n, q, p, alpha) as ks, Mac(n, ext) as mac:
        assert ks.digits == dn
        st = torch.cuda.current_stream().cuda_stream
        dx = _to_dev(torch, x, bits)
        dkey = [_to_dev(torch, k, bits) for k in key]
        dhat = [torch.full_like(k, sentinel) for k in dkey]
        up = torch.full((batch * dn * M * n,), sentinel, dtype=tdt, device="cuda")
        mid = [torch.full((batch * M * n,), sentinel, dtype=tdt, device="cuda") for _ in key]
        out = [torch.full((batch * L * n,), sentinel, dtype=tdt, device="cuda") for _ in key]
        for k, kh in zip(dkey, dhat):                           # key_hat: [dnum][L + K][n]
            mac.forward_device(kh, k, dn, stream=st)
        ks.modup_device(up, dx, batch, stream=st)
        for i in range(2):
            mac.mac_ntt_device(mid[i], up, dhat[i], batch, dn, shared=True, stream=st)
            ks.moddown_device(out[i], mid[i], batch, stream=st)
        torch.cuda.synchronize()
        got_up = _from_dev(up, bits, (batch, dn, M, n))
        got_mid = [_from_dev(t, bits, (batch, M, n)) for t in mid]
        got = [_from_dev(t, bits, (batch, L, n)) for t in out]
    # 1. every stage bit-exact against Python integers
    _assert_modup(got_up, x, q, p, alpha)
    plans = [O.Plan(n, m) for m in ext]
    for i in range(2):
        want = np.empty((batch, M, n), dtype=_dt(bits))
        for b in range(batch):
            for l, m in enumerate(ext):
                acc = sum(plans[l].product_merged(got_up[b, d, l], key[i][d, l]).astype(object)
                          for d in range(dn))
                want[b, l] = (acc % m).astype(_dt(bits))
        assert np.array_equal(got_mid[i], want), i
        assert np.array_equal(got[i], B.moddown(got_mid[i], p, q)), i
    # 2. the key-switch identity
    bound = (K + 1) * (1 + h)
    for b in range(batch):
        err = ref.key_switch_error(x[b], got[0][b], got[1][b], q, s, s2)
        assert err <= bound, (b, err, bound)
