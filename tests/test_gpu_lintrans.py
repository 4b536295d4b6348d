"""GPU parity of the weighted sum of rotations before ModDown (include/nttmul_lintrans.h,
lib/libnttmul_lintrans.so, csrc/lintrans_dev.hpp k_lintrans).

Every case is compared bit for bit with the device composition of existing calls it replaces:
m = ksntt_mac(a_hat, b_hat, k); m permuted to [batch comps][rots][M][n] and passed through
ksntt_mac against w_hat as [1][1][rots][M][n] with k = {1}, terms = rots; the c_0 term padded with
zero P limbs, passed through ksntt_mac against the host-computed w_hat (P mod m_l), summed over r
the same way and added to component 0 mod m_l on the host in uint64.  And, on every output word at
every degree, with the CPU reference (tests/full_ref.py over tests/lintrans_ref.py), which shares
no code with the device: the composition beside it says which side is wrong.  Operands are device-resident, every output is
preset to the sentinel (tests/guarded.py).  The shapes are the smallest at which the kernel can go
wrong (tests/lintrans_cases.py).  Any canonical vector is a transform of something, so the inputs
are seeded canonical words."""
import ctypes

import numpy as np
import pytest

import bconv_ref as B
import full_ref as F
import guarded as G
import hoist_ref as H
import lintrans_cases as C
import lintrans_ref as ref
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


def _apply(torch, lt, a, b, ks, w=None, c0=None, stream=0):
    """One device call out of a guarded arena: every operand between sentinel guards, aligned to
    its word only, the output preset to the sentinel; after the call no guard word and no input
    word has changed and every output word is written."""
    bits, (batch, terms) = lt.word_bits, a.shape[:2]
    rots, comps = b.shape[:2]
    shape = (batch, comps, lt.limbs, lt.n)
    operands = dict(out=int(np.prod(shape)), a=a, b=b)
    if w is not None:
        operands["w"] = w
    if c0 is not None:
        operands["z"] = c0
    arena = G.DeviceArena(torch, bits, G.guard_words(max(terms, comps) * lt.limbs * lt.n),
                          **operands)
    lt.apply_device(arena["out"], arena["a"], arena["b"], ks, batch, terms, comps,
                    w_hat=arena["w"] if w is not None else None,
                    c0_hat=arena["z"] if c0 is not None else None, stream=stream)
    torch.cuda.synchronize()
    arena.check()
    return arena.get("out", shape)


def _operands(case, seed):
    q, p = C.moduli_of(case)
    ext, rng = q + p, np.random.default_rng(seed)
    M, rots, dt = len(ext), len(case.ks), _dt(case.bits)
    a = B.random_words(rng, ext * case.terms, case.batch, case.n, dt)
    b = B.random_words(rng, ext * (case.terms * case.comps), rots, case.n, dt)
    w = B.random_words(rng, ext, rots, case.n, dt) if case.weighted else None
    c0 = B.random_words(rng, q, case.batch, case.n, dt) if case.c0 else None
    return (a.reshape(case.batch, case.terms, M, case.n),
            b.reshape(rots, case.comps, case.terms, M, case.n), w, c0)


def _id(c):
    return (f"u{c.bits}-n{c.n}x{c.batch}-{c.L}.{c.K}-t{c.terms}c{c.comps}r{len(c.ks)}"
            f"{'w' if c.weighted else ''}{'z' if c.c0 else ''}")


@pytest.mark.parametrize("case", C.parity_cases(), ids=_id)
def test_apply_parity(case, torch_cuda):
    q, p = C.moduli_of(case)
    a, b, w, c0 = _operands(case, case.n + case.terms + 10 * case.comps + len(case.ks))
    with nttmul.NttLinTrans(case.n, q, p) as lt, nttmul.NttKeySwitch(case.n, q, p, 1) as kn:
        assert (lt.q_limbs, lt.p_limbs, lt.word_bits, lt.n) == (case.L, case.K, case.bits, case.n)
        assert (lt.info.n, 1 << lt.info.logn, lt.info.ndev) == (case.n, case.n, 1)
        assert lt.limbs == case.L + case.K
        assert lt.kernel_name(case.comps, case.weighted) == \
            C.kernel_name(case.bits, case.comps, case.weighted)
        got = _apply(torch_cuda, lt, a, b, case.ks, w, c0)
        assert np.array_equal(got, ref.composition(kn, a, b, case.ks, q, p, w, c0))
    F.assert_equal(got, F.reference("lintrans", "apply", a, b, case.ks, q, p, w, c0), _id(case))


@pytest.mark.parametrize("case", C.worst_cases(), ids=_id)
@pytest.mark.parametrize("fill", ("top", "zero"))
def test_worst_case_ranges(fill, case, torch_cuda):
    """Every word of every operand at its modulus - 1, sixteen rotations of sixteen terms, weights
    and c_0 on: per limb (-1)^3 rots terms + (-1)^2 rots (P mod q_l) on component 0 of Q, whatever
    the rotations.  And all zero."""
    q, p = C.moduli_of(case)
    ext, L = q + p, len(q)
    M, rots, n, dt = len(ext), len(case.ks), case.n, _dt(case.bits)
    top = np.array([m - 1 if fill == "top" else 0 for m in ext], dtype=dt)[:, None]
    a = np.broadcast_to(top, (case.batch, case.terms, M, n)).copy()
    b = np.broadcast_to(top, (rots, case.comps, case.terms, M, n)).copy()
    w = np.broadcast_to(top, (rots, M, n)).copy()
    c0 = np.broadcast_to(top[:L], (case.batch, L, n)).copy()
    with nttmul.NttLinTrans(n, q, p) as lt:
        got = _apply(torch_cuda, lt, a, b, case.ks, w, c0)
    F.assert_equal(got, F.reference("lintrans", "apply", a, b, case.ks, q, p, w, c0), _id(case))
    if fill == "zero":
        assert not got.any()
        return
    pq = ref.p_mod(q, p)
    for l, m in enumerate(ext):
        for i in range(case.comps):
            want = -rots * case.terms + (rots * pq[l] if i == 0 and l < L else 0)
            assert (got[:, i, l] == want % m).all(), (l, i)


@pytest.mark.parametrize("bits", (32, 64))
def test_identities(bits, torch_cuda):
    """One rotation, unweighted, no c_0: NttKeySwitch.mac.  Unweighted: weighted by ones."""
    case = C.Case(bits, 256, C.V + 1, 3, 2, 2, 2, (5, 25, 5), True, True)
    q, p = C.moduli_of(case)
    a, b, _, c0 = _operands(case, 31)
    ones = np.ones((3, 5, 256), dtype=_dt(bits))
    with nttmul.NttLinTrans(256, q, p) as lt, nttmul.NttKeySwitch(256, q, p, 1) as kn:
        for r, k in enumerate(case.ks):
            got = _apply(torch_cuda, lt, a, b[r:r + 1], (k,))
            assert np.array_equal(got, kn.mac(a, b[r:r + 1], (k,))[:, 0])
            F.assert_equal(got, F.reference("ksntt", "mac", a, b[r:r + 1], (k,), q + p)[:, 0], r)
        for z in (None, c0):
            got = _apply(torch_cuda, lt, a, b, case.ks, None, z)
            assert np.array_equal(got, _apply(torch_cuda, lt, a, b, case.ks, ones, z))
            F.assert_equal(got, F.reference("lintrans", "apply", a, b, case.ks, q, p, None, z))


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n", C.CHAIN_N)
def test_the_linear_transform_end_to_end(n, bits, torch_cuda):
    """NttKeySwitch.modup -> NttLinTrans.apply -> NttModDown.moddown over batch 2 polynomials on
    lintrans_ref.chain's keys, c_0 and weights: at both n every stage bit for bit the CPU chain's,
    in the NTT domain, and within hoist_ref.chain_bound() (the derivation is
    tests/test_lintrans_ref.py's)."""
    torch = torch_cuda
    ch = ref.chain(n, bits)
    q, p, alpha, ks = ch["q"], ch["p"], ch["alpha"], ch["ks"]
    batch, L, M = ch["x"].shape[0], len(q), len(q) + len(p)
    Ctx = nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext
    with Ctx(n, q) as low, nttmul.NttKeySwitch(n, q, p, alpha) as kn, \
            nttmul.NttLinTrans(n, q, p) as lt, nttmul.NttModDown(n, q, p) as md:
        assert np.array_equal(low.forward(ch["c0"]), ch["c0_hat"])
        up_hat = kn.modup(low.forward(ch["x"]))
        assert np.array_equal(up_hat, ch["up_hat"])
        mid = _apply(torch, lt, up_hat, ch["key_hat"], ks, ch["w_hat"], ch["c0_hat"])
        out_hat = md.moddown(mid.reshape(batch * 2, M, n))
        back = low.inverse(out_hat).reshape(batch, 2, L, n)
        F.assert_equal(mid, ch["mid_lt"], "apply")
        F.assert_equal(out_hat, H.forward(ch["out_lt"].reshape(batch * 2, L, n), q), "moddown")
        assert np.array_equal(out_hat, low.forward(ch["out_lt"].reshape(batch * 2, L, n)))
        assert np.array_equal(back, ch["out_lt"])
    errs = ref.chain_errors(ch, back)
    print("lintrans chain errors", n, bits, errs, "bound", H.chain_bound())
    assert max(errs) <= H.chain_bound()


@pytest.mark.parametrize("bits", (32, 64))
def test_validate_flag_leaves_the_output_untouched(bits, torch_cuda):
    """A word equal to its own limb's modulus (in range for the limb before it: the primes
    descend) in each of the four operands in turn is NTTMUL_ERANGE and the output keeps its
    sentinel; clean operands succeed; without the flag there is no check."""
    torch = torch_cuda
    n, batch, (L, K) = C.VALIDATE
    case = C.Case(bits, n, batch, L, K, 2, 1, (5,), True, True, True)
    q, p = C.moduli_of(case)
    ext = q + p
    assert all(x > y for x, y in zip(ext, ext[1:]))
    ops = dict(zip("abwz", _operands(case, 10)))
    with nttmul.NttLinTrans(n, q, p, validate=True) as strict, nttmul.NttLinTrans(n, q, p) as lax:
        want = ref.apply(ops["a"], ops["b"], case.ks, q, p, ops["w"], ops["z"])
        assert np.array_equal(_apply(torch, strict, ops["a"], ops["b"], case.ks, ops["w"],
                                     ops["z"]), want)
        for which in "abwz":
            bad = {k: v.copy() for k, v in ops.items()}
            limbs = L if which == "z" else L + K
            bad[which].reshape(-1, limbs, n)[-1, limbs - 1, n - 1] = (q if which == "z" else ext)[-1]
            out = torch.full((batch * (L + K) * n,), -1, dtype=_tdt(torch, bits), device="cuda")
            dev = {k: _to_dev(torch, v, bits) for k, v in bad.items()}
            with pytest.raises(nttmul.NttmulError) as ei:
                strict.apply_device(out, dev["a"], dev["b"], case.ks, batch, case.terms, case.comps,
                                    w_hat=dev["w"], c0_hat=dev["z"])
            assert ei.value.status == nttmul.NTTMUL_ERANGE, which
            torch.cuda.synchronize()
            assert bool((out == -1).all()), which
            _apply(torch, lax, bad["a"], bad["b"], case.ks, bad["w"], bad["z"])
        # an operand that is not given is not checked
        assert np.array_equal(_apply(torch, strict, ops["a"], ops["b"], case.ks),
                              ref.apply(ops["a"], ops["b"], case.ks, q, p))


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,batch", C.HOST)
def test_host_form_equals_the_device_form(n, batch, bits, torch_cuda):
    L, K = C.HOST_SHAPE
    case = C.Case(bits, n, batch, L, K, 2, 2, (5, 1), True, True)
    q, p = C.moduli_of(case)
    a, b, w, c0 = _operands(case, 78)
    with nttmul.NttLinTrans(n, q, p) as lt, nttmul.NttKeySwitch(n, q, p, 1) as kn:
        assert lt.io_dtype == _dt(bits)
        for ww, zz in C.FP_OPTIONAL:
            wv, zv = (w if ww else None), (c0 if zz else None)
            dev = _apply(torch_cuda, lt, a, b, case.ks, wv, zv)
            host = lt.apply(a, b, case.ks, wv, zv)
            assert host.dtype == _dt(bits) and np.array_equal(host, dev)
            assert np.array_equal(dev, ref.composition(kn, a, b, case.ks, q, p, wv, zv))
            F.assert_equal(dev, F.reference("lintrans", "apply", a, b, case.ks, q, p, wv, zv),
                           (n, batch, bits, ww, zz))
        assert lt.apply(a[:0], b, case.ks, w, c0[:0]).shape == (0, 2, L + K, n)
        with pytest.raises(ValueError):
            lt.apply(a, b[:1], case.ks)
        with pytest.raises(ValueError):
            lt.apply(a, b, case.ks, w[:1])
        with pytest.raises(ValueError):
            lt.apply(a, b, case.ks, None, c0[:, :1])


def test_device_path_rules(torch_cuda):
    """A call on a non-default stream followed by a dependent call on the same stream without a
    host synchronise; the empty batch; bad arguments on a live context, in the header's order."""
    torch = torch_cuda
    n = 256
    case = C.Case(32, n, C.V + 1, 3, 2, 2, 1, (5, 25), True, True)
    q, p = C.moduli_of(case)
    EINVAL, OK = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_OK
    a, b, w, c0 = _operands(case, 6)
    with nttmul.NttLinTrans(n, q, p) as lt:
        side = torch.cuda.Stream()
        first = ref.apply(a, b, case.ks, q, p, w, c0)               # [batch, 1, M, n]
        assert np.array_equal(_apply(torch, lt, a, b, case.ks, w, c0, stream=side.cuda_stream),
                              first)
        # the second call reads the first's output as its a_hat (terms = 1), same stream
        da, db, dw, dz = (_to_dev(torch, x, 32) for x in (a, b, w, c0))
        mid = torch.full((first.size,), -1, dtype=torch.int32, device="cuda")
        out = torch.full((first.size,), -1, dtype=torch.int32, device="cuda")
        b2 = b[:1, :, :1]
        db2 = _to_dev(torch, b2, 32)
        torch.cuda.synchronize()
        lt.apply_device(mid, da, db, case.ks, case.batch, case.terms, 1, w_hat=dw, c0_hat=dz,
                        stream=side.cuda_stream)
        lt.apply_device(out, mid, db2, (2 * n - 1,), case.batch, 1, 1, stream=side.cuda_stream)
        side.synchronize()
        assert np.array_equal(_from_dev(out, 32, first.shape),
                              ref.apply(first, b2, (2 * n - 1,), q, p))
        keep = torch.full((5 * n,), 7, dtype=torch.int32, device="cuda")   # one polynomial
        lt.apply_device(keep, keep, keep, (5,), 0, 1, 1, w_hat=keep, c0_hat=keep)   # batch = 0
        torch.cuda.synchronize()
        assert bool((keep == 7).all())
        ptr = keep.data_ptr()
        with pytest.raises(ValueError):                              # too small a tensor
            lt.apply_device(keep, keep, keep, (5,), 2, 1, 1)
        k5, k4, kbig = ((ctypes.c_uint32 * 1)(v) for v in (5, 4, 2 * n + 1))
        fn = lt._lib.nttmul_lintrans_apply_device
        # terms, comps, rots, k, k[r], the operands: nttmul_ksntt_mac_device's order
        assert fn(lt._h, None, None, None, None, None, None, 0, 1, 0, 0, 0, None) == EINVAL
        assert fn(lt._h, ptr, ptr, ptr, None, None, k5, 1, 1, 0, 1, 0, None) == EINVAL   # terms = 0
        assert fn(lt._h, ptr, ptr, ptr, None, None, k5, 1, 1, 1, 0, 0, None) == EINVAL   # comps = 0
        assert fn(lt._h, ptr, ptr, ptr, None, None, k5, 1, 1, 1, 3, 0, None) == EINVAL   # comps > 2
        assert fn(lt._h, ptr, ptr, ptr, None, None, k5, 0, 1, 1, 1, 0, None) == EINVAL   # rots = 0
        assert fn(lt._h, ptr, ptr, ptr, None, None, k5, 17, 1, 1, 1, 0, None) == EINVAL  # rots > 16
        assert fn(lt._h, ptr, ptr, ptr, None, None, None, 1, 1, 1, 1, 0, None) == EINVAL # NULL k
        assert fn(lt._h, ptr, ptr, ptr, None, None, k4, 1, 1, 1, 1, 0, None) == EINVAL   # even
        assert fn(lt._h, ptr, ptr, ptr, None, None, kbig, 1, 1, 1, 1, 0, None) == EINVAL # >= 2n
        assert fn(lt._h, ptr, ptr, ptr, None, None, k4, 1, 0, 1, 1, 0, None) == EINVAL   # at batch 0
        assert fn(lt._h, None, ptr, ptr, None, None, k5, 1, 1, 1, 1, 0, None) == EINVAL
        assert fn(lt._h, ptr, None, ptr, None, None, k5, 1, 1, 1, 1, 0, None) == EINVAL
        assert fn(lt._h, ptr, ptr, None, None, None, k5, 1, 1, 1, 1, 0, None) == EINVAL
        assert fn(lt._h, None, None, None, None, None, k5, 1, 0, 1, 1, 0, None) == OK
        assert fn(lt._h, None, None, None, None, None, k5, 1, 0, 1, 1, 99, None) == \
            nttmul.NTTMUL_ENODEV
        host = lt._lib.nttmul_lintrans_apply
        assert host(lt._h, None, None, None, None, None, k5, 1, 0, 1, 1) == OK
        assert host(lt._h, None, ptr, ptr, None, None, k5, 1, 1, 1, 1) == EINVAL
        name = lt._lib.nttmul_lintrans_kernel_name
        assert name(lt._h, 1, 0, None, 1) == EINVAL
        assert name(lt._h, 0, 0, None, 0) == EINVAL and name(lt._h, 3, 1, None, 0) == EINVAL
        assert name(lt._h, 2, 1, None, 0) == len(C.kernel_name(32, 2, True))


def test_mirror_agrees_with_the_library_dispatch(torch_cuda):
    """tests/lintrans_cases.py kernel_name against nttmul_lintrans_kernel_name at every degree, and
    the names are kernels the library holds."""
    held = nttmul.kernel_hashes(nttmul.LINTRANS_LIB_PATH)
    for bits in (32, 64):
        for n in C.ALL_N:
            q, p = C.moduli_of(C.Case(bits, n, 1, 2, 1, 1, 1, (1,), False, False))
            with nttmul.NttLinTrans(n, q, p) as lt:
                for comps in (1, 2):
                    for weighted in (False, True):
                        name = lt.kernel_name(comps, weighted)
                        assert name == C.kernel_name(bits, comps, weighted)
                        assert nttmul.dispatch_key(name) in held
