"""GPU parity of the ciphertext product on NTT-domain limbs (include/nttmul_ctmul.h,
lib/libnttmul_ctmul.so, csrc/ctmul_dev.hpp k_ctmul_high and k_ctmul_relin).

Every case is compared bit for bit with the composition of existing calls it replaces
(tests/ctmul_ref.py composition): ksntt_mac with k = (1,) for the key sum, the per-limb pointwise
products of one plain context per limb of Q for the tensor terms, host modular additions.  And, on
every output word at every degree, with the CPU reference (tests/full_ref.py over
tests/ctmul_ref.py), which shares no code with the device: the composition beside it says which
side is wrong.  Operands are device-resident between sentinel
guards, aligned to their word only, every output preset to the sentinel (tests/guarded.py).  The
shapes are the smallest at which the kernels can go wrong (tests/ctmul_cases.py).  Any canonical
vector is a transform of something, so the inputs are seeded canonical words."""
import numpy as np
import pytest

import bconv_ref as B
import ctmul_cases as C
import ctmul_ref as ref
import full_ref as F
import guarded as G
import hoist_cases as HC
import mdntt_ref
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


def _guard(ct, x, terms=0):
    return G.guard_words(max(max(terms, 2) * ct.limbs, x.shape[1] * 2 * ct.q_limbs) * ct.n)


def _high(torch, ct, x, y, stream=0):
    """One device call out of a guarded arena: every operand between sentinel guards, aligned to
    its word only, the output preset to the sentinel; after the call no guard word and no input
    word has changed and every output word is written.  y is x: the square, one buffer."""
    batch, pairs = x.shape[:2]
    shape = (batch, ct.q_limbs, ct.n)
    operands = dict(out=int(np.prod(shape)), x=x)
    if y is not x:
        operands["y"] = y
    arena = G.DeviceArena(torch, ct.word_bits, _guard(ct, x), **operands)
    xd = arena["x"]
    ct.high_device(arena["out"], xd, xd if y is x else arena["y"], batch, pairs, stream=stream)
    torch.cuda.synchronize()
    arena.check()
    return arena.get("out", shape)


def _relin(torch, ct, up, key, x, y, stream=0):
    batch, pairs = x.shape[:2]
    terms = up.shape[1]
    shape = (batch, 2, ct.limbs, ct.n)
    operands = dict(out=int(np.prod(shape)), up=up, key=key, x=x)
    if y is not x:
        operands["y"] = y
    arena = G.DeviceArena(torch, ct.word_bits, _guard(ct, x, terms), **operands)
    xd = arena["x"]
    ct.relin_device(arena["out"], arena["up"], arena["key"], xd, xd if y is x else arena["y"],
                    batch, pairs, terms, stream=stream)
    torch.cuda.synchronize()
    arena.check()
    return arena.get("out", shape)


def _operands(case, seed):
    """(up, key, x, y) of a case; y is x for the square."""
    q, p = C.moduli_of(case)
    ext, rng = q + p, np.random.default_rng(seed)
    M, dt = len(ext), _dt(case.bits)
    up = B.random_words(rng, ext * case.terms, case.batch, case.n, dt)
    key = B.random_words(rng, ext * case.terms, 2, case.n, dt)
    shape = (case.batch, case.pairs, 2, case.L, case.n)
    x = B.random_words(rng, q * (2 * case.pairs), case.batch, case.n, dt).reshape(shape)
    y = x if case.square else B.random_words(rng, q * (2 * case.pairs), case.batch, case.n,
                                             dt).reshape(shape)
    return (up.reshape(case.batch, case.terms, M, case.n), key.reshape(2, case.terms, M, case.n),
            x, y)


class _Plain:
    """One plain context per limb of Q: the library's own per-limb pointwise products."""

    def __init__(self, n, q):
        self.ctx = [nttmul.Context(n, m) for m in q]

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        for c in self.ctx:
            c.close()


def _id(c):
    return (f"{c.op}-u{c.bits}-n{c.n}x{c.batch}-{c.L}.{c.K}-s{c.pairs}t{c.terms}"
            f"{'sq' if c.square else ''}")


@pytest.mark.parametrize("case", C.parity_cases(), ids=_id)
def test_parity(case, torch_cuda):
    q, p = C.moduli_of(case)
    up, key, x, y = _operands(case, case.n + case.terms + 10 * case.pairs + case.batch)
    with nttmul.NttCtMul(case.n, q, p) as ct, _Plain(case.n, q) as plain:
        assert (ct.q_limbs, ct.p_limbs, ct.word_bits, ct.n) == (case.L, case.K, case.bits, case.n)
        assert (ct.info.n, 1 << ct.info.logn, ct.info.ndev) == (case.n, case.n, 1)
        assert ct.limbs == case.L + case.K
        assert ct.kernel_name(case.op) == C.kernel_name(case.op, case.bits)
        if case.op == "high":
            got = _high(torch_cuda, ct, x, y)
            assert np.array_equal(got, ref.tensor_composition(plain, x, y, q)[2])
            F.assert_equal(got, F.reference("ctmul", "high", x, y, q), _id(case))
            return
        got = _relin(torch_cuda, ct, up, key, x, y)
        with nttmul.NttKeySwitch(case.n, q, p, 1) as kn:
            assert np.array_equal(got, ref.composition(kn, plain, up, key, x, y, q, p))
    F.assert_equal(got, F.reference("ctmul", "relin", up, key, x, y, q, p), _id(case))


@pytest.mark.parametrize("case", C.worst_cases(), ids=_id)
@pytest.mark.parametrize("fill", ("top", "zero"))
def test_worst_case_ranges(fill, case, torch_cuda):
    """Every word of every operand at its modulus - 1, sixteen pairs and sixteen terms: per limb
    d2 = pairs, e_0 = pairs, e_1 = 2 pairs, the key sum = terms, whatever the limb.  And all
    zero."""
    q, p = C.moduli_of(case)
    ext, L = q + p, len(q)
    M, n, dt = len(ext), case.n, _dt(case.bits)
    top = np.array([m - 1 if fill == "top" else 0 for m in ext], dtype=dt)[:, None]
    up = np.broadcast_to(top, (case.batch, case.terms, M, n)).copy()
    key = np.broadcast_to(top, (2, case.terms, M, n)).copy()
    x = np.broadcast_to(top[:L], (case.batch, case.pairs, 2, L, n)).copy()
    y = x.copy()
    with nttmul.NttCtMul(n, q, p) as ct:
        got = _high(torch_cuda, ct, x, y) if case.op == "high" else \
            _relin(torch_cuda, ct, up, key, x, y)
    F.assert_equal(got, F.reference("ctmul", "high", x, y, q) if case.op == "high" else
                   F.reference("ctmul", "relin", up, key, x, y, q, p), (_id(case), fill))
    if fill == "zero":
        assert not got.any()
        return
    if case.op == "high":
        for l, m in enumerate(q):
            assert (got[:, l] == case.pairs % m).all(), l
        return
    pq = ref.p_mod(q, p)
    for l, m in enumerate(ext):
        for i in range(2):
            want = case.terms + (pq[l] * (i + 1) * case.pairs if l < L else 0)
            assert (got[:, i, l] == want % m).all(), (l, i)


@pytest.mark.parametrize("bits", (32, 64))
def test_identities(bits, torch_cuda):
    """key_hat = 0 leaves 0 in the limbs of P and (P mod q_l) e_i in the limbs of Q; relin on x, y
    equals relin on y, x; pairs = 2 equals the modular sum of two pairs = 1 calls' tensor parts;
    high on x, y equals high on y, x."""
    case = C.Case("relin", bits, 256, C.V + 1, 3, 2, 2, 2, False)
    q, p = C.moduli_of(case)
    L = len(q)
    up, key, x, y = _operands(case, 31)
    zero = np.zeros_like(key)
    with nttmul.NttCtMul(256, q, p) as ct:
        plain = _relin(torch_cuda, ct, up, zero, x, y)
        assert not plain[:, :, L:].any()
        e0, e1, d2 = ref.tensor(x, y, q)
        for l, (m, pq) in enumerate(zip(q, ref.p_mod(q, p))):
            for i, e in enumerate((e0, e1)):
                assert (plain[:, i, l].astype(object) == e[:, l].astype(object) * pq % m).all()
        both = _relin(torch_cuda, ct, up, key, x, y)
        assert np.array_equal(both, _relin(torch_cuda, ct, up, key, y, x))
        assert np.array_equal(_high(torch_cuda, ct, x, y), d2)
        assert np.array_equal(_high(torch_cuda, ct, y, x), d2)
        parts = [_relin(torch_cuda, ct, up, zero, x[:, s:s + 1].copy(), y[:, s:s + 1].copy())
                 for s in range(2)]
        for l, m in enumerate(q):
            assert (plain[:, :, l].astype(object) ==
                    (parts[0][:, :, l].astype(object) + parts[1][:, :, l].astype(object)) % m).all()
        # the square through one pointer is the call on two equal buffers
        assert np.array_equal(_relin(torch_cuda, ct, up, key, x, x),
                              _relin(torch_cuda, ct, up, key, x, x.copy()))
        assert np.array_equal(_high(torch_cuda, ct, x, x), _high(torch_cuda, ct, x, x.copy()))


def _device_chain(torch, n, ch, pairs_of=None):
    """high -> ksntt_modup -> relin -> mdntt_moddown(q, p) on the device, and the d_i as the
    library's inverse of the pointwise products.  Returns every stage."""
    q, p, alpha = ch["q"], ch["p"], ch["alpha"]
    batch, L, M = ch["x"].shape[0], len(q), len(q) + len(p)
    Ctx = nttmul.RnsContext if n <= 4096 else nttmul.RnsMpContext
    with Ctx(n, q) as low, Ctx(n, q + p) as big, nttmul.NttCtMul(n, q, p) as ct, \
            nttmul.NttKeySwitch(n, q, p, alpha) as kn, nttmul.NttModDown(n, q, p) as md, \
            _Plain(n, q) as plain:
        x_hat = low.forward(ch["x"].reshape(-1, L, n)).reshape(ch["x"].shape)
        y_hat = low.forward(ch["y"].reshape(-1, L, n)).reshape(ch["y"].shape)
        key_hat = big.forward(ch["key"].reshape(-1, M, n)).reshape(ch["key"].shape)
        d2_hat = _high(torch, ct, x_hat, y_hat)
        up_hat = kn.modup(d2_hat)
        mid = _relin(torch, ct, up_hat, key_hat, x_hat, y_hat)
        out_hat = md.moddown(mid.reshape(batch * 2, M, n))
        out = low.inverse(out_hat).reshape(batch, 2, L, n)
        e0, e1, d2p = ref.tensor_composition(plain, x_hat, y_hat, q)
        assert np.array_equal(d2p, d2_hat)
        d = np.stack([low.inverse(e) for e in (e0, e1, d2_hat)])
    return dict(x_hat=x_hat, y_hat=y_hat, key_hat=key_hat, d2_hat=d2_hat, up_hat=up_hat, mid=mid,
                out_hat=out_hat, out=out, d=d)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n", C.CHAIN_N)
def test_the_multiplication_end_to_end(n, bits, torch_cuda):
    """high -> NttKeySwitch.modup -> relin -> NttModDown.moddown on hoist_cases.CHAIN_SHAPE with a
    ternary s of weight CHAIN_H and the zero-noise key for s s -> s: at both n every stage bit
    for bit the CPU chain's, the NTT-domain ones word for word; the result decrypts to d0 + d1 s + d2 s^2 within
    +-(K + 1)(1 + h) per limb, centred.  The bound is derived (tests/ctmul_ref.py chain_bound):
    with a zero-noise key c_hat[0] + c_hat[1] s = P (d0 + d1 s + d2 s^2) mod QP exactly, and
    ModDown's output is (Y_i - r_i) / P with 0 <= r_i < (K + 1) P: one key switch's rounding."""
    ch = ref.chain(n, bits)
    got = _device_chain(torch_cuda, n, ch)
    for stage in ("x_hat", "y_hat", "key_hat", "d2_hat", "up_hat", "mid", "out", "d"):
        F.assert_equal(got[stage], ch[stage], stage)
    F.assert_equal(got["out_hat"], mdntt_ref.forward(ch["out"].reshape(-1, len(ch["q"]), n),
                                                     ch["q"]), "out_hat")
    errs = ref.chain_errors(ch, got["out"], got["d"])
    L, K, _ = HC.CHAIN_SHAPE
    print("ctmul chain errors", n, bits, errs, "bound", ref.chain_bound())
    assert ref.chain_bound() == (K + 1) * (1 + HC.CHAIN_H)
    assert max(errs) <= ref.chain_bound()


@pytest.mark.parametrize("bits", (32, 64))
def test_lazy_relinearisation_keeps_one_key_switchs_bound(bits, torch_cuda):
    """pairs = 3: a dot product of ciphertexts through one relinearisation, same bound."""
    ch = ref.chain(256, bits, 3)
    got = _device_chain(torch_cuda, 256, ch)
    for stage in ("d2_hat", "up_hat", "mid", "out", "d"):
        assert np.array_equal(got[stage], ch[stage]), stage
    assert max(ref.chain_errors(ch, got["out"], got["d"])) <= ref.chain_bound()


@pytest.mark.parametrize("bits", (32, 64))
def test_the_merged_rescale(bits, torch_cuda):
    """NttModDown(n, q[:-1], (q[-1],) + p) reads the same c_hat and divides by P q_{L-1}: bit for
    bit mdntt_ref.formula, and every word is (floor(Y_i / (P q_{L-1})) - a) mod q_l for some
    0 <= a <= K with Y_i the CRT value of the reference c_hat: the conversion's alpha is below the
    K + 1 limbs it sums."""
    n = 256
    ch = ref.chain(n, bits)
    q, p = ch["q"], ch["p"]
    L, K, M = len(q), len(p), len(q) + len(p)
    assert L >= 2
    batch = ch["x"].shape[0]
    lo, hi = q[:-1], (q[-1],) + p
    with nttmul.NttCtMul(n, q, p) as ct, nttmul.NttModDown(n, lo, hi) as md:
        mid = _relin(torch_cuda, ct, ch["up_hat"], ch["key_hat"], ch["x_hat"], ch["y_hat"])
        assert np.array_equal(mid, ch["mid"])
        flat = mid.reshape(batch * 2, M, n)
        out_hat = md.moddown(flat)
    assert out_hat.shape == (batch * 2, L - 1, n)
    assert np.array_equal(out_hat, mdntt_ref.formula(flat, lo, hi))
    out = ref.coefficients(out_hat, lo)
    coeff = ref.coefficients(flat, q + p)
    D = int(np.prod([int(m) for m in hi], dtype=object))
    for u in range(batch * 2):
        Y = [B.crt(coeff[u][:, j], q + p) for j in range(n)]
        for l, m in enumerate(lo):
            diff = [(int(y) // D - int(v)) % m for y, v in zip(Y, out[u, l])]
            assert max(diff) <= K, (u, l, max(diff))


@pytest.mark.parametrize("bits", (32, 64))
def test_validate_flag_leaves_the_output_untouched(bits, torch_cuda):
    """A word equal to its own limb's modulus (in range for the limb before it: the primes
    descend) in each operand in turn is NTTMUL_ERANGE and the output keeps its sentinel; clean
    operands succeed; without the flag there is no check."""
    torch = torch_cuda
    n, batch, (L, K) = C.VALIDATE
    case = C.Case("relin", bits, n, batch, L, K, 2, 2, False, True)
    q, p = C.moduli_of(case)
    ext, M = q + p, L + K
    assert all(a > b for a, b in zip(ext, ext[1:]))
    names = ("up", "key", "x", "y")
    ops = dict(zip(names, _operands(case, 10)))
    with nttmul.NttCtMul(n, q, p, validate=True) as strict, nttmul.NttCtMul(n, q, p) as lax:
        assert np.array_equal(_relin(torch, strict, *ops.values()), ref.relin(*ops.values(), q, p))
        assert np.array_equal(_high(torch, strict, ops["x"], ops["y"]),
                              ref.high(ops["x"], ops["y"], q))
        assert np.array_equal(_relin(torch, strict, ops["up"], ops["key"], ops["x"], ops["x"]),
                              ref.relin(ops["up"], ops["key"], ops["x"], ops["x"], q, p))
        for which in names:
            bad = {k: v.copy() for k, v in ops.items()}
            limbs, mods = (L, q) if which in "xy" else (M, ext)
            bad[which].reshape(-1, limbs, n)[-1, limbs - 1, n - 1] = mods[-1]
            dev = {k: _to_dev(torch, v, bits) for k, v in bad.items()}
            out = torch.full((batch * 2 * M * n,), -1, dtype=_tdt(torch, bits), device="cuda")
            with pytest.raises(nttmul.NttmulError) as ei:
                strict.relin_device(out, dev["up"], dev["key"], dev["x"], dev["y"], batch,
                                    case.pairs, case.terms)
            assert ei.value.status == nttmul.NTTMUL_ERANGE, which
            if which in "xy":
                with pytest.raises(nttmul.NttmulError) as ei:
                    strict.high_device(out, dev["x"], dev["y"], batch, case.pairs)
                assert ei.value.status == nttmul.NTTMUL_ERANGE, which
            torch.cuda.synchronize()
            assert bool((out == -1).all()), which
            _relin(torch, lax, bad["up"], bad["key"], bad["x"], bad["y"])
            _high(torch, lax, bad["x"], bad["y"])


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,batch", C.HOST)
def test_host_form_equals_the_device_form(n, batch, bits, torch_cuda):
    L, K = C.HOST_SHAPE
    case = C.Case("relin", bits, n, batch, L, K, 2, 2, False)
    q, p = C.moduli_of(case)
    up, key, x, y = _operands(case, 78)
    with nttmul.NttCtMul(n, q, p) as ct, nttmul.NttKeySwitch(n, q, p, 1) as kn, \
            _Plain(n, q) as plain:
        assert ct.io_dtype == _dt(bits)
        for yy in (y, x):
            dev = _relin(torch_cuda, ct, up, key, x, yy)
            host = ct.relin(up, key, x, yy)
            assert host.dtype == _dt(bits) and np.array_equal(host, dev)
            assert np.array_equal(dev, ref.composition(kn, plain, up, key, x, yy, q, p))
            F.assert_equal(dev, F.reference("ctmul", "relin", up, key, x, yy, q, p), (n, bits))
            hd = _high(torch_cuda, ct, x, yy)
            hh = ct.high(x, yy)
            assert hh.dtype == _dt(bits) and np.array_equal(hh, hd)
            assert np.array_equal(hd, ref.tensor_composition(plain, x, yy, q)[2])
            F.assert_equal(hd, F.reference("ctmul", "high", x, yy, q), (n, bits))
        assert ct.relin(up[:0], key, x[:0], y[:0]).shape == (0, 2, L + K, n)
        assert ct.high(x[:0], y[:0]).shape == (0, L, n)
        with pytest.raises(ValueError):
            ct.relin(up, key[:1], x, y)
        with pytest.raises(ValueError):
            ct.relin(up, key, x, y[:, :1])
        with pytest.raises(ValueError):
            ct.relin(up[:1], key, x, y)
        with pytest.raises(ValueError):
            ct.high(x, y[:, :, :1])


def test_device_path_rules(torch_cuda):
    """A call on a non-default stream followed by a dependent call on the same stream without a
    host synchronise; the empty batch; bad arguments on a live context, in the header's order."""
    torch = torch_cuda
    n = 256
    case = C.Case("relin", 32, n, C.V + 1, 3, 2, 2, 2, False)
    q, p = C.moduli_of(case)
    L, M = case.L, case.L + case.K
    EINVAL, OK = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_OK
    up, key, x, y = _operands(case, 6)
    with nttmul.NttCtMul(n, q, p) as ct:
        side = torch.cuda.Stream()
        first = ref.relin(up, key, x, y, q, p)                      # [batch, 2, M, n]
        assert np.array_equal(_relin(torch, ct, up, key, x, y, stream=side.cuda_stream), first)
        assert np.array_equal(_high(torch, ct, x, y, stream=side.cuda_stream), ref.high(x, y, q))
        # the second call reads the first's output as its up_hat (terms = 2), same stream
        du, dk, dx, dy = (_to_dev(torch, v, 32) for v in (up, key, x, y))
        mid = torch.full((first.size,), -1, dtype=torch.int32, device="cuda")
        out = torch.full((first.size,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ct.relin_device(mid, du, dk, dx, dy, case.batch, case.pairs, case.terms,
                        stream=side.cuda_stream)
        ct.relin_device(out, mid, dk, dx, dx, case.batch, case.pairs, 2, stream=side.cuda_stream)
        side.synchronize()
        assert np.array_equal(_from_dev(out, 32, first.shape), ref.relin(first, key, x, x, q, p))
        keep = torch.full((2 * M * n,), 7, dtype=torch.int32, device="cuda")   # one term's key
        ct.relin_device(keep, keep, keep, keep, keep, 0, 1, 1)      # batch = 0
        ct.high_device(keep, keep, keep, 0, 1)
        torch.cuda.synchronize()
        assert bool((keep == 7).all())
        ptr = keep.data_ptr()
        with pytest.raises(ValueError):                              # too small a tensor
            ct.relin_device(keep, keep, keep, keep, keep, 2, 1, 1)
        with pytest.raises(ValueError):
            ct.high_device(keep, keep, keep, 2, 1)
        fn = ct._lib.nttmul_ctmul_relin_device
        # pairs, terms, the operands: the header's order
        assert fn(ct._h, ptr, ptr, ptr, ptr, ptr, 1, 0, 1, 0, None) == EINVAL     # pairs = 0
        assert fn(ct._h, ptr, ptr, ptr, ptr, ptr, 1, 1, 0, 0, None) == EINVAL     # terms = 0
        assert fn(ct._h, None, None, None, None, None, 0, 0, 1, 0, None) == EINVAL  # at batch 0
        assert fn(ct._h, None, None, None, None, None, 0, 1, 0, 0, None) == EINVAL
        for hole in range(5):
            args = [None if i == hole else ptr for i in range(5)]
            assert fn(ct._h, *args, 1, 1, 1, 0, None) == EINVAL
        assert fn(ct._h, None, None, None, None, None, 0, 1, 1, 0, None) == OK
        assert fn(ct._h, None, None, None, None, None, 0, 1, 1, 99, None) == nttmul.NTTMUL_ENODEV
        assert fn(ct._h, ptr, ptr, ptr, ptr, ptr, 1, 1, 1, 99, None) == nttmul.NTTMUL_ENODEV
        hi = ct._lib.nttmul_ctmul_high_device
        assert hi(ct._h, ptr, ptr, ptr, 1, 0, 0, None) == EINVAL                  # pairs = 0
        assert hi(ct._h, None, None, None, 0, 0, 0, None) == EINVAL
        for hole in range(3):
            args = [None if i == hole else ptr for i in range(3)]
            assert hi(ct._h, *args, 1, 1, 0, None) == EINVAL
        assert hi(ct._h, None, None, None, 0, 1, 0, None) == OK
        assert hi(ct._h, None, None, None, 0, 1, 99, None) == nttmul.NTTMUL_ENODEV
        assert ct._lib.nttmul_ctmul_relin(ct._h, None, None, None, None, None, 0, 1, 1) == OK
        assert ct._lib.nttmul_ctmul_relin(ct._h, None, ptr, ptr, ptr, ptr, 1, 1, 1) == EINVAL
        assert ct._lib.nttmul_ctmul_high(ct._h, None, None, None, 0, 1) == OK
        assert ct._lib.nttmul_ctmul_high(ct._h, None, ptr, ptr, 1, 1) == EINVAL
        name = ct._lib.nttmul_ctmul_kernel_name
        assert name(ct._h, 0, None, 1) == EINVAL
        assert name(ct._h, 2, None, 0) == EINVAL and name(ct._h, -1, None, 0) == EINVAL
        assert name(ct._h, 1, None, 0) == len(C.kernel_name("relin", 32))

def test_mirror_agrees_with_the_library_dispatch(torch_cuda):
    """tests/ctmul_cases.py kernel_name against nttmul_ctmul_kernel_name at every degree, and the
    names are kernels the library holds."""
    held = nttmul.kernel_hashes(nttmul.CTMUL_LIB_PATH)
    for bits in (32, 64):
        for n in C.ALL_N:
            q, p = C.moduli_of(C.Case("high", bits, n, 1, 2, 1, 1, 1, False))
            with nttmul.NttCtMul(n, q, p) as ct:
                for i, op in enumerate(C.OPS):
                    name = ct.kernel_name(op)
                    assert name == ct.kernel_name(i) == C.kernel_name(op, bits)
                    assert nttmul.dispatch_key(name) in held
