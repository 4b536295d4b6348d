"""GPU parity of ModUp and the key mac on NTT-domain limbs (include/nttmul_ksntt.h,
lib/libnttmul_ksntt.so, csrc/ksntt_dev.hpp k_ksntt_*).

Every case is compared bit for bit with the device composition it replaces:
  (A) modup(x_hat) == forward(ks_modup(inverse(x_hat))) with the extended basis' own contexts,
  (B) mac(a_hat, b_hat, k) == forward(hoist_ntt(a_hat, b_hat, k)),
  (C) mdntt_moddown(mac(modup(x_hat), key_hat, k)) == forward of the coefficient-order chain's
      output, on hoist_ref.chain's keys, within its bound +-(K + 1)(1 + h),
and, on every output word at every degree, with the CPU reference (tests/full_ref.py over
tests/ksntt_ref.py and the oracle's transforms), which shares no code with the device: the
compositions beside it say which side is wrong when the two disagree.  Operands are
device-resident, every output is preset to the sentinel (tests/guarded.py for the small cases, a
fill for the large ones).  The shapes are the smallest at which the kernels can go wrong
(tests/ksntt_cases.py).  Any canonical vector is a transform of something, so the inputs are
seeded canonical words."""
import numpy as np
import pytest

import bconv_ref as B
import full_ref as F
import guarded as G
import hoist_ref as H
import ks_ref
import ksntt_cases as C
import ksntt_ref as ref
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


def _tdt(torch, bits):
    return torch.int32 if bits == 32 else torch.int64


def _to_dev(torch, x, bits):
    x = np.ascontiguousarray(x, dtype=_dt(bits))
    return torch.from_numpy(x.view(np.int32 if bits == 32 else np.int64).reshape(-1)).cuda()


def _from_dev(t, bits, shape):
    return t.cpu().numpy().view(_dt(bits)).reshape(shape)


def _ctx(n):
    return nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext


def _compose_modup(torch, n, q, p, alpha, x_hat):
    """forward_{Q u P}(ks_modup(inverse_Q(x_hat))) on the device, three calls."""
    bits, batch, L, M = 8 * x_hat.dtype.itemsize, x_hat.shape[0], len(q), len(q) + len(p)
    dn = -(-L // alpha)
    Ctx = _ctx(n)
    with Ctx(n, q + p) as ext, Ctx(n, q) as low, nttmul.KeySwitchBasis(n, q, p, alpha) as ks:
        dx = _to_dev(torch, x_hat, bits)
        coef = torch.empty(batch * L * n, dtype=_tdt(torch, bits), device="cuda")
        up = torch.empty(batch * dn * M * n, dtype=_tdt(torch, bits), device="cuda")
        out = torch.empty_like(up)
        low.inverse_device(coef, dx, batch)
        ks.modup_device(up, coef, batch)
        ext.forward_device(out, up, batch * dn)
        torch.cuda.synchronize()
        return _from_dev(out, bits, (batch, dn, M, n))


def _compose_mac(torch, n, ext, a_hat, b_hat, ks):
    """forward(hoist_ntt(a_hat, b_hat, k)) on the device, two calls."""
    bits, (batch, terms) = 8 * a_hat.dtype.itemsize, a_hat.shape[:2]
    rots, comps = b_hat.shape[:2]
    with _ctx(n)(n, ext) as ctx:
        c = torch.empty(batch * rots * comps * len(ext) * n, dtype=_tdt(torch, bits), device="cuda")
        out = torch.empty_like(c)
        ctx.hoist_ntt_device(c, _to_dev(torch, a_hat, bits), _to_dev(torch, b_hat, bits), ks, batch,
                             terms, comps)
        ctx.forward_device(out, c, batch * rots * comps)
        torch.cuda.synchronize()
        return _from_dev(out, bits, (batch, rots, comps, len(ext), n))


def _modup(torch, kn, x_hat, stream=0):
    """One device call out of a guarded arena: both operands between sentinel guards, aligned to
    their word only, the output preset to the sentinel; after the call no guard word and no input
    word has changed and every output word is written."""
    bits, batch = kn.word_bits, x_hat.shape[0]
    shape = (batch, kn.digits, kn.limbs, kn.n)
    arena = G.DeviceArena(torch, bits, G.guard_words(kn.digits * kn.limbs * kn.n),
                          out=int(np.prod(shape)), x=x_hat)
    kn.modup_device(arena["out"], arena["x"], batch, stream=stream)
    torch.cuda.synchronize()
    arena.check()
    return arena.get("out", shape)


def _mac(torch, kn, a_hat, b_hat, ks, stream=0):
    bits, (batch, terms) = kn.word_bits, a_hat.shape[:2]
    rots, comps = b_hat.shape[:2]
    shape = (batch, rots, comps, kn.limbs, kn.n)
    arena = G.DeviceArena(torch, bits, G.guard_words(max(terms, rots * comps) * kn.limbs * kn.n),
                          out=int(np.prod(shape)), a=a_hat, b=b_hat)
    kn.mac_device(arena["out"], arena["a"], arena["b"], ks, batch, terms, comps, stream=stream)
    torch.cuda.synchronize()
    arena.check()
    return arena.get("out", shape)


def _x(case, seed):
    q, _ = C.moduli_of(case)
    return B.random_words(np.random.default_rng(seed), q, case.batch, case.n, _dt(case.bits))


def _ab(case, seed):
    q, p = C.moduli_of(case)
    ext, rng = q + p, np.random.default_rng(seed)
    M, rots = len(ext), len(case.ks)
    a = B.random_words(rng, ext * case.terms, case.batch, case.n, _dt(case.bits))
    b = B.random_words(rng, ext * (case.terms * case.comps), rots, case.n, _dt(case.bits))
    return (a.reshape(case.batch, case.terms, M, case.n),
            b.reshape(rots, case.comps, case.terms, M, case.n))


def _up_id(c):
    return f"u{c.bits}-n{c.n}x{c.batch}-{c.L}.{c.K}.{c.alpha}"


def _mac_id(c):
    return f"u{c.bits}-n{c.n}x{c.batch}-t{c.terms}c{c.comps}r{len(c.ks)}"


@pytest.mark.parametrize("case", C.modup_cases(), ids=_up_id)
def test_modup_parity(case, torch_cuda):
    """(A): grid and pairs (batch 3 and 33), the digit shapes with short last digits, alpha over
    the fold cadence, every degree."""
    q, p = C.moduli_of(case)
    x = _x(case, 1000 * case.L + 10 * case.K + case.alpha + case.n)
    with nttmul.NttKeySwitch(case.n, q, p, case.alpha) as kn:
        assert (kn.q_limbs, kn.p_limbs, kn.word_bits) == (case.L, case.K, case.bits)
        assert (kn.digit_limbs, kn.digits) == (case.alpha, C.dnum(case))
        assert (kn.info.n, 1 << kn.info.logn, kn.info.ndev, kn.info.scratch_mb) == \
            (case.n, case.n, 1, C.DEFAULT_SCRATCH_MB)
        assert kn.kernel_name("modup") == C.kernel_name("modup", case.n, case.bits)
        got = _modup(torch_cuda, kn, x)
    assert np.array_equal(got, _compose_modup(torch_cuda, case.n, q, p, case.alpha, x))
    for d, D in enumerate(ks_ref.digits(case.L, case.alpha)):     # the own limbs are copies
        assert np.array_equal(got[:, d, D.start:D.stop], x[:, D.start:D.stop])
    F.assert_equal(got, F.reference("ksntt", "modup", x, q, p, case.alpha), _up_id(case))


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n", C.RANGE_N)
@pytest.mark.parametrize("fill", C.RANGE_FILLS)
def test_modup_worst_case_ranges(fill, n, bits, torch_cuda):
    """Every word at its modulus - 1; the x_hat whose coefficient-order digits are
    ks_ref.worst_case (every y_i = q_i - 1 in every sum); all zero."""
    L, K, alpha = C.RANGE_SHAPE
    case = C.Up(bits, n, 2, L, K, alpha)
    q, p = C.moduli_of(case)
    if fill == "top":
        x = np.empty((2, L, n), dtype=_dt(bits))
        for l, m in enumerate(q):
            x[:, l, :] = m - 1
    elif fill == "worst":
        flat = np.empty((2, L, n), dtype=_dt(bits))
        for i, v in enumerate(ks_ref.worst_case(q, alpha)):
            flat[:, i, :] = v
        with _ctx(n)(n, q) as low:
            x = low.forward(flat)
    else:
        x = np.zeros((2, L, n), dtype=_dt(bits))
    with nttmul.NttKeySwitch(n, q, p, alpha) as kn:
        got = _modup(torch_cuda, kn, x)
    assert np.array_equal(got, _compose_modup(torch_cuda, n, q, p, alpha, x))
    if fill == "zero":
        assert not got.any()
    if fill == "worst":
        assert np.array_equal(x, ref.worst_x_hat(q, alpha, 2, n, _dt(bits)))
    F.assert_equal(got, F.reference("ksntt", "modup", x, q, p, alpha), (fill, n, bits))


def test_modup_sub_batches_and_two_streams(torch_cuda):
    """scratch_mb = 1: three sub-batches with a short last one at n = 4096 and at n = 65536; then,
    on the grown scratch, two calls on two streams with no synchronisation between them."""
    torch = torch_cuda
    for case, (*_, want) in zip(C.subbatch_cases(), C.SUBBATCH):
        assert C.chunks(case) == list(want) and len(want) == 3 and want[-1] < want[0]
        q, p = C.moduli_of(case)
        bits = case.bits
        with nttmul.NttKeySwitch(case.n, q, p, case.alpha, scratch_mb=1) as kn:
            assert kn.info.scratch_mb == 1
            small = _x(case._replace(batch=1), 3)
            got = _modup(torch, kn, small)
            assert np.array_equal(got, _compose_modup(torch, case.n, q, p, case.alpha, small))
            F.assert_equal(got, F.reference("ksntt", "modup", small, q, p, case.alpha),
                           (case, "one polynomial"))
            x = _x(case, 4)                     # the scratch grows to a whole sub-batch
            want_x = _compose_modup(torch, case.n, q, p, case.alpha, x)
            assert np.array_equal(_modup(torch, kn, x), want_x)
            F.assert_equal(want_x, F.reference("ksntt", "modup", x, q, p, case.alpha),
                           (case, "sub-batches"))
            y = _x(case, 5)
            want_y = _compose_modup(torch, case.n, q, p, case.alpha, y)
            F.assert_equal(want_y, F.reference("ksntt", "modup", y, q, p, case.alpha),
                           (case, "second stream"))
            dx, dy = _to_dev(torch, x, bits), _to_dev(torch, y, bits)
            ox = torch.full((want_x.size,), -1, dtype=_tdt(torch, bits), device="cuda")
            oy = torch.full((want_y.size,), -1, dtype=_tdt(torch, bits), device="cuda")
            torch.cuda.synchronize()
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            kn.modup_device(ox, dx, case.batch, stream=s1.cuda_stream)
            kn.modup_device(oy, dy, case.batch, stream=s2.cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(_from_dev(ox, bits, want_x.shape), want_x)
            assert np.array_equal(_from_dev(oy, bits, want_y.shape), want_y)


@pytest.mark.parametrize("case", C.mac_cases(), ids=_mac_id)
def test_mac_parity(case, torch_cuda):
    """(B): terms 1 and 3, comps 1 and 2, the plain mac, three rotations, sixteen."""
    q, p = C.moduli_of(case)
    ext = q + p
    a, b = _ab(case, case.n + case.terms + 10 * case.comps + len(case.ks))
    with nttmul.NttKeySwitch(case.n, q, p, 1) as kn:
        assert kn.kernel_name("mac", case.comps) == \
            C.kernel_name("mac", case.n, case.bits, case.comps)
        got = _mac(torch_cuda, kn, a, b, case.ks)
    assert np.array_equal(got, _compose_mac(torch_cuda, case.n, ext, a, b, case.ks))
    F.assert_equal(got, F.reference("ksntt", "mac", a, b, case.ks, ext), _mac_id(case))


@pytest.mark.parametrize("case", C.mac_worst_cases(), ids=_mac_id)
def test_mac_worst_case_input(case, torch_cuda):
    """Every word of both operands at its modulus - 1, sixteen terms: every sum is
    16 (m - 1)^2 mod m = 16 mod m, whatever the rotation."""
    q, p = C.moduli_of(case)
    ext = q + p
    M, rots = len(ext), len(case.ks)
    top = np.array([m - 1 for m in ext], dtype=_dt(case.bits))[:, None]
    a = np.broadcast_to(top, (case.batch, case.terms, M, case.n)).copy()
    b = np.broadcast_to(top, (rots, case.comps, case.terms, M, case.n)).copy()
    with nttmul.NttKeySwitch(case.n, q, p, 1) as kn:
        got = _mac(torch_cuda, kn, a, b, case.ks)
    assert (got == case.terms).all()
    assert np.array_equal(got, _compose_mac(torch_cuda, case.n, ext, a, b, case.ks))
    F.assert_equal(got, F.reference("ksntt", "mac", a, b, case.ks, ext), _mac_id(case))


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n", C.CHAIN_N)
def test_the_ntt_domain_key_switch(n, bits, torch_cuda):
    """(C): modup -> mac -> mdntt_moddown on hoist_ref.chain's inputs equals forward of the
    coefficient-order chain's output bit for bit, and therefore switches within the chain's bound."""
    torch = torch_cuda
    ch = H.chain(n, bits)
    q, p, alpha, ks = ch["q"], ch["p"], ch["alpha"], ch["ks"]
    batch, rots, L = ch["x"].shape[0], len(ks), len(q)
    assert rots == 3
    Ctx = _ctx(n)
    with Ctx(n, q) as low, nttmul.NttKeySwitch(n, q, p, alpha) as kn, \
            nttmul.NttModDown(n, q, p) as md:
        x_hat = low.forward(ch["x"])
        up_hat = _modup(torch, kn, x_hat)
        assert np.array_equal(up_hat, ch["up_hat"])
        mid_hat = _mac(torch, kn, up_hat, ch["key_hat"], ks)
        out_hat = md.moddown(mid_hat.reshape(batch * rots * 2, L + len(p), n))
        want = low.forward(ch["out"].reshape(batch * rots * 2, L, n))
        assert np.array_equal(out_hat, want)
        back = low.inverse(out_hat).reshape(batch, rots, 2, L, n)
    assert np.array_equal(back, ch["out"])
    assert max(H.chain_errors(ch, back)) <= H.chain_bound()


@pytest.mark.parametrize("bits", (32, 64))
def test_validate_flag_leaves_the_output_untouched(bits, torch_cuda):
    """A word equal to its own limb's modulus (in range for the limb before it: the primes
    descend) is NTTMUL_ERANGE and the output keeps its sentinel, in modup's x_hat and in either
    operand of mac; a clean input succeeds; without the flag there is no check."""
    torch = torch_cuda
    n, batch, (L, K, alpha) = C.VALIDATE
    up = C.Up(bits, n, batch, L, K, alpha)
    mac = C.Mac(bits, n, batch, L, K, 2, 1, (5,))
    q, p = C.moduli_of(up)
    ext = q + p
    assert all(a > b for a, b in zip(ext, ext[1:]))
    good = _x(up, 9)
    a, b = _ab(mac, 10)
    with nttmul.NttKeySwitch(n, q, p, alpha, validate=True) as strict, \
            nttmul.NttKeySwitch(n, q, p, alpha) as lax:
        got = _modup(torch, strict, good)
        assert np.array_equal(got, _compose_modup(torch, n, q, p, alpha, good))
        F.assert_equal(got, F.reference("ksntt", "modup", good, q, p, alpha), bits)
        got = _mac(torch, strict, a, b, mac.ks)
        assert np.array_equal(got, _compose_mac(torch, n, ext, a, b, mac.ks))
        F.assert_equal(got, F.reference("ksntt", "mac", a, b, mac.ks, ext), bits)
        bad = good.copy()
        bad[batch - 1, L - 1, n - 1] = q[L - 1]
        out = torch.full((batch * C.dnum(up) * (L + K) * n,), -1, dtype=_tdt(torch, bits),
                         device="cuda")
        with pytest.raises(nttmul.NttmulError) as ei:
            strict.modup_device(out, _to_dev(torch, bad, bits), batch)
        assert ei.value.status == nttmul.NTTMUL_ERANGE
        torch.cuda.synchronize()
        assert bool((out == -1).all())
        _modup(torch, lax, bad)
        for which in ("a", "b"):
            ba, bb = a.copy(), b.copy()
            (ba if which == "a" else bb).reshape(-1, L + K, n)[-1, L + K - 1, n - 1] = ext[-1]
            out = torch.full((batch * (L + K) * n,), -1, dtype=_tdt(torch, bits), device="cuda")
            with pytest.raises(nttmul.NttmulError) as ei:
                strict.mac_device(out, _to_dev(torch, ba, bits), _to_dev(torch, bb, bits), mac.ks,
                                  batch, mac.terms, mac.comps)
            assert ei.value.status == nttmul.NTTMUL_ERANGE, which
            torch.cuda.synchronize()
            assert bool((out == -1).all())
            _mac(torch, lax, ba, bb, mac.ks)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,batch", C.HOST)
def test_host_forms_equal_the_device_forms(n, batch, bits, torch_cuda):
    L, K, alpha = C.HOST_SHAPE
    up = C.Up(bits, n, batch, L, K, alpha)
    mac = C.Mac(bits, n, batch, L, K, 2, 2, (5, 1))
    q, p = C.moduli_of(up)
    x = _x(up, 77)
    a, b = _ab(mac, 78)
    with nttmul.NttKeySwitch(n, q, p, alpha) as kn:
        assert kn.io_dtype == _dt(bits)
        dev = _modup(torch_cuda, kn, x)
        host = kn.modup(x)
        assert host.dtype == _dt(bits) and np.array_equal(host, dev)
        assert kn.modup(x[:0]).shape == (0, C.dnum(up), L + K, n)
        with pytest.raises(ValueError):
            kn.modup(np.zeros((1, L + 1, n), dtype=_dt(bits)))
        dev_c = _mac(torch_cuda, kn, a, b, mac.ks)
        host_c = kn.mac(a, b, mac.ks)
        assert host_c.dtype == _dt(bits) and np.array_equal(host_c, dev_c)
        with pytest.raises(ValueError):
            kn.mac(a, b[:1], mac.ks)
    assert np.array_equal(dev, _compose_modup(torch_cuda, n, q, p, alpha, x))
    assert np.array_equal(dev_c, _compose_mac(torch_cuda, n, q + p, a, b, mac.ks))
    F.assert_equal(dev, F.reference("ksntt", "modup", x, q, p, alpha), (n, batch, bits))
    F.assert_equal(dev_c, F.reference("ksntt", "mac", a, b, mac.ks, q + p), (n, batch, bits))


def test_device_path_rules(torch_cuda):
    """A non-default stream; the empty batch; bad arguments on a live context, in the header's
    order."""
    torch = torch_cuda
    up = C.Up(32, C.N, 3, 3, 2, 2)
    mac = C.Mac(32, C.N, 3, 3, 2, 2, 1, (5,))
    q, p = C.moduli_of(up)
    EINVAL, OK = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_OK
    with nttmul.NttKeySwitch(C.N, q, p, 2) as kn:
        side = torch.cuda.Stream()
        x = _x(up, 5)
        assert np.array_equal(_modup(torch, kn, x, stream=side.cuda_stream),
                              ref.modup(x, q, p, 2))
        a, b = _ab(mac, 6)
        assert np.array_equal(_mac(torch, kn, a, b, mac.ks, stream=side.cuda_stream),
                              ref.mac(a, b, mac.ks, q + p))
        out = torch.full((5 * C.N,), 7, dtype=torch.int32, device="cuda")   # one b_hat polynomial
        kn.modup_device(out, out, 0)                                 # batch = 0: a no-op
        kn.mac_device(out, out, out, (5,), 0, 1, 1)
        torch.cuda.synchronize()
        assert bool((out == 7).all())
        ptr = out.data_ptr()
        fn = kn._lib.nttmul_ksntt_modup_device
        assert fn(kn._h, None, ptr, 1, 0, None) == EINVAL
        assert fn(kn._h, ptr, None, 1, 0, None) == EINVAL
        assert fn(kn._h, None, None, 0, 0, None) == OK
        assert fn(kn._h, ptr, ptr, 1, 99, None) == nttmul.NTTMUL_ENODEV
        host = kn._lib.nttmul_ksntt_modup
        assert host(kn._h, None, None, 0) == OK
        assert host(kn._h, None, ptr, 1) == EINVAL
        with pytest.raises(ValueError):                              # too small a tensor
            kn.modup_device(out, out, 2)
        import ctypes
        k5, k4, kbig = ((ctypes.c_uint32 * 1)(v) for v in (5, 4, 2 * C.N + 1))
        mfn = kn._lib.nttmul_ksntt_mac_device
        # terms, comps, rots, k, k[r], the operands: hoist_ntt's order
        assert mfn(kn._h, None, None, None, None, 0, 1, 0, 0, 0, None) == EINVAL
        assert mfn(kn._h, ptr, ptr, ptr, k5, 1, 1, 0, 1, 0, None) == EINVAL      # terms = 0
        assert mfn(kn._h, ptr, ptr, ptr, k5, 1, 1, 1, 0, 0, None) == EINVAL      # comps = 0
        assert mfn(kn._h, ptr, ptr, ptr, k5, 1, 1, 1, 3, 0, None) == EINVAL      # comps > 2
        assert mfn(kn._h, ptr, ptr, ptr, k5, 0, 1, 1, 1, 0, None) == EINVAL      # rots = 0
        assert mfn(kn._h, ptr, ptr, ptr, k5, 17, 1, 1, 1, 0, None) == EINVAL     # rots > 16
        assert mfn(kn._h, ptr, ptr, ptr, None, 1, 1, 1, 1, 0, None) == EINVAL    # NULL k
        assert mfn(kn._h, ptr, ptr, ptr, k4, 1, 1, 1, 1, 0, None) == EINVAL      # even
        assert mfn(kn._h, ptr, ptr, ptr, kbig, 1, 1, 1, 1, 0, None) == EINVAL    # >= 2n
        assert mfn(kn._h, ptr, ptr, ptr, k4, 1, 0, 1, 1, 0, None) == EINVAL      # k is read at batch 0
        assert mfn(kn._h, None, ptr, ptr, k5, 1, 1, 1, 1, 0, None) == EINVAL
        assert mfn(kn._h, ptr, None, ptr, k5, 1, 1, 1, 1, 0, None) == EINVAL
        assert mfn(kn._h, ptr, ptr, None, k5, 1, 1, 1, 1, 0, None) == EINVAL
        assert mfn(kn._h, None, None, None, k5, 1, 0, 1, 1, 0, None) == OK
        assert mfn(kn._h, None, None, None, k5, 1, 0, 1, 1, 99, None) == nttmul.NTTMUL_ENODEV
        name = kn._lib.nttmul_ksntt_kernel_name
        assert name(kn._h, 0, 1, None, 1) == EINVAL
        assert name(kn._h, 2, 1, None, 0) == EINVAL
        assert name(kn._h, 1, 0, None, 0) == EINVAL and name(kn._h, 1, 3, None, 0) == EINVAL
        assert name(kn._h, 0, 0, None, 0) == len(C.kernel_name("modup", C.N, 32))
        assert name(kn._h, 1, 2, None, 0) == len(C.kernel_name("mac", C.N, 32, 2))


def test_mirror_agrees_with_the_library_dispatch(torch_cuda):
    """tests/ksntt_cases.py kernel_name against nttmul_ksntt_kernel_name at every degree, and the
    names are kernels the library holds."""
    held = nttmul.kernel_hashes(nttmul.KSNTT_LIB_PATH)
    for bits in (32, 64):
        for n in C.ALL_N:
            q, p = C.moduli_of(C.Up(bits, n, 1, 2, 1, 1))
            with nttmul.NttKeySwitch(n, q, p, 1) as kn:
                names = [kn.kernel_name("modup"), kn.kernel_name(0)]
                assert names[0] == names[1] == C.kernel_name("modup", n, bits)
                for comps in (1, 2):
                    names.append(kn.kernel_name("mac", comps))
                    assert names[-1] == C.kernel_name("mac", n, bits, comps)
                for name in names:
                    for part in name.split(" + "):
                        assert nttmul.dispatch_key(part) in held
