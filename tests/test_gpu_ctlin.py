"""GPU parity of the ciphertext sums, plaintext products and the full tensor product on NTT-domain
limbs (include/nttmul_ctlin.h, lib/libnttmul_ctlin.so, csrc/ctlin_dev.hpp k_ctlin_combine and
k_ctlin_tensor).

Every comparison is bit for bit.  At every degree the expected value of every output word is the
CPU reference (tests/full_ref.py over tests/ctlin_ref.py), which shares no code with the device;
above n = 512 the composition the call replaces -- one plain pointwise context per limb plus host
modular additions -- is compared beside it and says which side is wrong.  Operands are device-resident between sentinel guards, aligned
to their word only, every output preset to the sentinel (tests/guarded.py).  L = 3 on the
mixed-size chains of tests/basis_cases.py, both word classes; the shapes are the smallest at which
the kernels can go wrong (tests/ctlin_cases.py).  Any canonical vector is a transform of
something, so the inputs are seeded canonical words; the two chains at the end start from
zero-noise ciphertexts and decrypt exactly."""
import ctypes

import numpy as np
import pytest

import bconv_ref as B
import ctlin_cases as C
import ctlin_ref as ref
import full_ref as F
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


def _tdt(torch, bits):
    return torch.int32 if bits == 32 else torch.int64


def _to_dev(torch, x, bits):
    x = np.ascontiguousarray(x, dtype=_dt(bits))
    return torch.from_numpy(x.view(np.int32 if bits == 32 else np.int64).reshape(-1)).cuda()


def _shape(case):
    return (case.batch, case.comps, C.L, case.n)


def _operands(case, seed):
    """(xs, ws) of a combine case: the x buffers, and per term its w (None for ONE)."""
    q, dt, rng = C.moduli_of(case), _dt(case.bits), np.random.default_rng(seed)
    xs = [B.random_words(rng, q * case.comps, case.batch, case.n, dt).reshape(_shape(case))
          for _ in range(C.x_count(case))]
    ws = []
    for kind, _ in case.terms:
        if kind == C.SCALAR:
            ws.append(np.array([int(rng.integers(0, m, dtype=np.uint64)) for m in q], dtype=dt))
        elif kind == C.PLAIN:
            ws.append(B.random_words(rng, q, 1, case.n, dt)[0])
        else:
            ws.append(None)
    return xs, ws


def _ref_terms(case, xs, ws):
    return [(None if i is None else xs[i], w, C.KIND_CODE[kind])
            for (kind, i), w in zip(case.terms, ws)]


def _combine(torch, cl, case, xs, ws, stream=0):
    """One device call out of a guarded arena: every operand between sentinel guards, aligned to
    its word only, the output preset to the sentinel; after the call no guard word and no input
    word has changed and every output word is written.  case.inplace: out is that x."""
    operands = {}
    if not case.inplace:
        operands["out"] = int(np.prod(_shape(case)))
    operands.update({f"x{i}": x for i, x in enumerate(xs)})
    operands.update({f"w{t}": w for t, w in enumerate(ws) if w is not None})
    inplace = tuple(f"x{i}" for i in case.inplace)
    arena = G.DeviceArena(torch, case.bits, C.fp_guard_words(case), inplace=inplace, **operands)
    out = inplace[0] if inplace else "out"
    views = {name: arena[name] for name in operands}     # one view per buffer: the same pointer
    terms = [(None if i is None else views[f"x{i}"], None if w is None else views[f"w{t}"],
              C.KIND_CODE[kind]) for t, ((kind, i), w) in enumerate(zip(case.terms, ws))]
    cl.combine_device(views[out], terms, case.batch, case.comps, stream=stream)
    torch.cuda.synchronize()
    arena.check()
    return arena.get(out, _shape(case))


def _pairs(case, seed):
    q, dt, rng = C.moduli_of(case), _dt(case.bits), np.random.default_rng(seed)
    shape = (case.batch, case.pairs, 2, C.L, case.n)
    x = B.random_words(rng, q * (2 * case.pairs), case.batch, case.n, dt).reshape(shape)
    y = x if case.square else B.random_words(rng, q * (2 * case.pairs), case.batch, case.n,
                                             dt).reshape(shape)
    return x, y


def _tensor(torch, cl, x, y, stream=0):
    batch, pairs = x.shape[:2]
    shape = (batch, 3, cl.limbs, cl.n)
    operands = dict(out=int(np.prod(shape)), x=x)
    if y is not x:
        operands["y"] = y
    guard = G.guard_words(max(3, 2 * pairs) * cl.limbs * cl.n)
    arena = G.DeviceArena(torch, cl.word_bits, guard, **operands)
    xd = arena["x"]
    cl.tensor_device(arena["out"], xd, xd if y is x else arena["y"], batch, pairs, stream=stream)
    torch.cuda.synchronize()
    arena.check()
    return arena.get("out", shape)


class _Plain:
    """One plain context per limb: the library's own per-limb pointwise products."""

    def __init__(self, n, q):
        self.ctx = [nttmul.Context(n, m) for m in q]

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        for c in self.ctx:
            c.close()


def _want_combine(case, xs, ws):
    """The CPU reference of every output word (tests/full_ref.py) at every n; above n = 512 the
    composition a caller runs today is held to it as well, which says which side is wrong."""
    q, terms = C.moduli_of(case), _ref_terms(case, xs, ws)
    want = F.reference("ctlin", "combine", terms, q, _shape(case), _dt(case.bits))
    if case.n > 512:
        with _Plain(case.n, q) as plain:
            F.assert_equal(ref.composition(plain, terms, q, _shape(case), _dt(case.bits)), want,
                           ("the composition", _id(case)))
    return want


def _id(c):
    if c.op == "tensor":
        return f"tensor-u{c.bits}-n{c.n}x{c.batch}-s{c.pairs}{'sq' if c.square else ''}"
    kinds = "".join(k[0] if i is not None else k[0].upper() for k, i in c.terms)
    return f"combine-u{c.bits}-n{c.n}x{c.batch}-c{c.comps}-{kinds}{'-inplace' if c.inplace else ''}"


@pytest.mark.parametrize("case", C.parity_cases(), ids=_id)
def test_parity(case, torch_cuda):
    q = C.moduli_of(case)
    with nttmul.NttCtLin(case.n, q) as cl:
        assert (cl.limbs, cl.word_bits, cl.n, cl.q) == (C.L, case.bits, case.n, q)
        assert (cl.info.n, 1 << cl.info.logn, cl.info.ndev) == (case.n, case.n, 1)
        assert cl.kernel_name(case.op, case.comps) == C.kernel_name(case)
        if case.op == "combine":
            xs, ws = _operands(case, case.n + case.batch + 7 * case.comps + len(case.terms))
            got = _combine(torch_cuda, cl, case, xs, ws)
            assert np.array_equal(got, _want_combine(case, xs, ws))
            return
        x, y = _pairs(case, case.n + case.batch + case.pairs)
        got = _tensor(torch_cuda, cl, x, y)
    F.assert_equal(got, F.reference("ctlin", "tensor", x, y, q), _id(case))
    if case.n > 512:
        with _Plain(case.n, q) as plain:
            assert np.array_equal(got, ref.tensor_composition(plain, x, y, q))
    # d_2 is nttmul_ctmul_high's output bit for bit
    with nttmul.NttCtMul(case.n, q, C.special_of(case.bits)) as ct:
        d2 = torch_cuda.full((case.batch * C.L * case.n,), -1, dtype=_tdt(torch_cuda, case.bits),
                             device="cuda")
        xd = _to_dev(torch_cuda, x, case.bits)
        ct.high_device(d2, xd, xd if y is x else _to_dev(torch_cuda, y, case.bits), case.batch,
                       case.pairs)
        torch_cuda.cuda.synchronize()
    assert np.array_equal(got[:, 2], d2.cpu().numpy().view(_dt(case.bits)).reshape(got[:, 2].shape))


@pytest.mark.parametrize("case", C.worst_cases(), ids=_id)
def test_worst_case_fill(case, torch_cuda):
    """Every word of every operand at its modulus - 1 in sixteen terms: 16 products of -1 by -1
    sum to 16, 16 words -1 to -16, whatever the limb.  And all zero."""
    q, dt = C.moduli_of(case), _dt(case.bits)
    kind = case.terms[0][0]
    top = np.array([m - 1 for m in q], dtype=dt)[:, None]
    x = np.broadcast_to(top, _shape(case)).copy()
    w = np.broadcast_to(top, (C.L, case.n)).copy() if kind == C.PLAIN else None
    with nttmul.NttCtLin(case.n, q) as cl:
        got = _combine(torch_cuda, cl, case, [x] * 16, [w] * 16)
        zero = _combine(torch_cuda, cl, case, [np.zeros_like(x)] * 16, [w] * 16)
    assert not zero.any()
    terms = [(x, w if kind == C.PLAIN else None, C.KIND_CODE[kind])] * 16
    F.assert_equal(got, F.reference("ctlin", "combine", terms, q, _shape(case), dt), _id(case))
    for l, m in enumerate(q):
        assert (got[:, :, l] == (16 if kind == C.PLAIN else -16) % m).all(), l


@pytest.mark.parametrize("bits", (32, 64))
def test_scalars_zero_one_and_minus_one(bits, torch_cuda):
    """0 x_0 + 1 x_1 + (q - 1) x_2 = x_1 - x_2; the constants 0 and q - 1 add 0 and -1 to
    component 0 alone; negation is one SCALAR term."""
    q, dt = C.moduli_of(bits), _dt(bits)
    terms = ((C.SCALAR, 0), (C.SCALAR, 1), (C.SCALAR, 2), (C.SCALAR, None), (C.SCALAR, None))
    case = C.Case("combine", bits, 256, 3, 2, terms)
    xs, _ = _operands(case, 41)
    zero, one = np.zeros(C.L, dtype=dt), np.ones(C.L, dtype=dt)
    minus = np.array([m - 1 for m in q], dtype=dt)
    ws = [zero, one, minus, zero, minus]
    with nttmul.NttCtLin(256, q) as cl:
        got = _combine(torch_cuda, cl, case, xs, ws)
        neg = _combine(torch_cuda, cl, case._replace(terms=((C.SCALAR, 0),)), xs[:1], [minus])
    assert np.array_equal(got, ref.combine(_ref_terms(case, xs, ws), q, _shape(case), dt))
    for l, m in enumerate(q):
        diff = (xs[1][:, :, l].astype(object) - xs[2][:, :, l].astype(object))
        assert (got[:, 1, l].astype(object) == diff[:, 1] % m).all()
        assert (got[:, 0, l].astype(object) == (diff[:, 0] - 1) % m).all()
        assert (neg[:, :, l].astype(object) == -xs[0][:, :, l].astype(object) % m).all()


@pytest.mark.parametrize("case", C.inplace_cases(), ids=_id)
def test_in_place_equals_out_of_place(case, torch_cuda):
    """out == x_0, and out == x_0 == x_3: every x vector of a lane is read before its output
    vector is stored."""
    xs, ws = _operands(case, case.n + 3)
    with nttmul.NttCtLin(case.n, C.moduli_of(case)) as cl:
        apart = _combine(torch_cuda, cl, case._replace(inplace=()), xs, ws)
        inplace = _combine(torch_cuda, cl, case, xs, ws)
    assert np.array_equal(inplace, apart)
    assert np.array_equal(apart, _want_combine(case, xs, ws))


@pytest.mark.parametrize("bits", (32, 64))
def test_validate_flag_leaves_the_output_untouched(bits, torch_cuda):
    """One word equal to its own limb's modulus in an x, in a plaintext and in a scalar in turn is
    NTTMUL_ERANGE and the output keeps its sentinel; clean operands succeed; without the flag
    there is no check.  The same for tensor's x_hat and y_hat."""
    torch = torch_cuda
    n, batch = C.VALIDATE
    case = C.Case("combine", bits, n, batch, 2, C.VALIDATE_TERMS, validate=True)
    q, dt = C.moduli_of(case), _dt(bits)
    xs, ws = _operands(case, 10)
    tcase = C.Case("tensor", bits, n, batch, 3, (), 2, False, validate=True)
    x, y = _pairs(tcase, 11)
    with nttmul.NttCtLin(n, q, validate=True) as strict, nttmul.NttCtLin(n, q) as lax:
        assert np.array_equal(_combine(torch, strict, case, xs, ws), _want_combine(case, xs, ws))
        assert np.array_equal(_tensor(torch, strict, x, y), ref.tensor(x, y, q))
        assert np.array_equal(_tensor(torch, strict, x, x), ref.tensor(x, x, q))
        out = torch.full((batch * 3 * C.L * n,), -1, dtype=_tdt(torch, bits), device="cuda")
        for which in ("x0", "x2", "plain", "scalar"):
            bx, bw = [v.copy() for v in xs], [None if w is None else w.copy() for w in ws]
            if which == "plain":
                bw[1][C.L - 1, n - 1] = q[-1]                       # the last word of the last limb
            elif which == "scalar":
                bw[2][1] = q[1]                                     # (in range for limb 0)
            else:
                bx[int(which[1])][-1, -1, 1, 0] = q[1]
            dx = [_to_dev(torch, v, bits) for v in bx]
            dw = [None if w is None else _to_dev(torch, w, bits) for w in bw]
            terms = [(None if i is None else dx[i], w, C.KIND_CODE[kind])
                     for (kind, i), w in zip(case.terms, dw)]
            with pytest.raises(nttmul.NttmulError) as ei:
                strict.combine_device(out, terms, batch, case.comps)
            assert ei.value.status == nttmul.NTTMUL_ERANGE, which
            torch.cuda.synchronize()
            assert bool((out == -1).all()), which
            _combine(torch, lax, case, bx, bw)
        for which in ("x", "y"):
            bad = dict(x=x.copy(), y=y.copy())
            bad[which][-1, -1, 1, C.L - 1, n - 1] = q[-1]
            with pytest.raises(nttmul.NttmulError) as ei:
                strict.tensor_device(out, _to_dev(torch, bad["x"], bits),
                                     _to_dev(torch, bad["y"], bits), batch, 2)
            assert ei.value.status == nttmul.NTTMUL_ERANGE, which
            torch.cuda.synchronize()
            assert bool((out == -1).all()), which
            _tensor(torch, lax, bad["x"], bad["y"])


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,batch", C.HOST)
def test_host_form_equals_the_device_form(n, batch, bits, torch_cuda):
    case = C.Case("combine", bits, n, batch, 2, C.HOST_TERMS)
    q, dt = C.moduli_of(case), _dt(bits)
    xs, ws = _operands(case, 78)
    tcase = C.Case("tensor", bits, n, batch, 3, (), 2, False)
    x, y = _pairs(tcase, 79)
    with nttmul.NttCtLin(n, q) as cl:
        assert cl.io_dtype == dt
        dev = _combine(torch_cuda, cl, case, xs, ws)
        terms = _ref_terms(case, xs, ws)
        host = cl.combine(terms)
        assert host.dtype == dt and np.array_equal(host, dev)
        assert np.array_equal(dev, _want_combine(case, xs, ws))
        # in place on the host: out is x_0, which two terms read
        mine = xs[0].copy()
        again = cl.combine([(mine if t[0] is xs[0] else t[0], t[1], t[2]) for t in terms], out=mine)
        assert again is mine and np.array_equal(mine, dev)
        for yy in (y, x):
            td = _tensor(torch_cuda, cl, x, yy)
            th = cl.tensor(x, yy)
            assert th.dtype == dt and np.array_equal(th, td)
            F.assert_equal(td, F.reference("ctlin", "tensor", x, yy, q), (n, batch, bits))
        assert cl.tensor(x[:0], y[:0]).shape == (0, 3, C.L, n)
        assert cl.combine([(xs[0][:0], None, 0)]).shape == (0, 2, C.L, n)
        with pytest.raises(ValueError):
            cl.combine([(xs[0], None, 0), (xs[1][:1], None, 0)])
        with pytest.raises(ValueError):
            cl.combine([(xs[0], ws[0][:, :1], 2)])
        with pytest.raises(ValueError):
            cl.combine([(None, ws[3], 1)])                          # no shape without an x or out
        with pytest.raises(ValueError):
            cl.tensor(x, y[:, :1])


def test_device_path_rules(torch_cuda):
    """A call on a non-default stream followed by a dependent call on the same stream without a
    host synchronise; the empty batch; bad arguments on a live context, in the header's order."""
    torch = torch_cuda
    n, bits = 256, 32
    case = C.Case("combine", bits, n, 5, 2, ((C.PLAIN, 0), (C.ONE, 1)))
    q, dt = C.moduli_of(case), _dt(bits)
    EINVAL, OK, ENODEV = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_OK, nttmul.NTTMUL_ENODEV
    xs, ws = _operands(case, 6)
    with nttmul.NttCtLin(n, q) as cl:
        side = torch.cuda.Stream()
        first = ref.combine(_ref_terms(case, xs, ws), q, _shape(case), dt)
        assert np.array_equal(_combine(torch, cl, case, xs, ws, stream=side.cuda_stream), first)
        # the second call adds the first's output to itself in place, same stream
        d0, d1, dw = (_to_dev(torch, v, bits) for v in (xs[0], xs[1], ws[0]))
        mid = torch.full((first.size,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        cl.combine_device(mid, [nttmul.ctlin_plain(d0, dw), nttmul.ctlin_one(d1)], 5, 2,
                          stream=side.cuda_stream)
        cl.combine_device(mid, [nttmul.ctlin_one(mid), nttmul.ctlin_one(mid)], 5, 2,
                          stream=side.cuda_stream)
        side.synchronize()
        twice = ref.combine([(first, None, 0)] * 2, q, _shape(case), dt)
        assert np.array_equal(mid.cpu().numpy().view(dt).reshape(first.shape), twice)
        keep = torch.full((2 * C.L * n,), 7, dtype=torch.int32, device="cuda")
        cl.combine_device(keep, [nttmul.ctlin_one(keep)], 0, 2)     # batch = 0
        cl.tensor_device(keep, keep, keep, 0, 1)
        torch.cuda.synchronize()
        assert bool((keep == 7).all())
        with pytest.raises(ValueError):                              # too small a tensor
            cl.combine_device(keep, [nttmul.ctlin_one(keep)], 2, 2)
        with pytest.raises(ValueError):
            cl.tensor_device(keep, keep, keep, 1, 1)
        ptr = keep.data_ptr()
        fn = cl._lib.nttmul_ctlin_combine_device
        T = nttmul.CtLinTerm

        def arr(*terms):
            return (T * len(terms))(*terms)

        good = arr(T(ptr, None, 0, 0), T(ptr, ptr, 1, 0), T(None, ptr, 2, 0))
        worst = T(None, None, 3, 1)
        assert fn(cl._h, mid.data_ptr(), good, 3, 1, 1, 0, None) == OK  # (out overlaps no operand)
        torch.cuda.synchronize()
        for nterms in (0, 17):                                       # then comps, terms, out wrong too
            assert fn(cl._h, None, None, nterms, 1, 0, 0, None) == EINVAL
        for comps in (0, 4):
            assert fn(cl._h, None, None, 1, 1, comps, 0, None) == EINVAL
            assert fn(cl._h, ptr, good, 3, 0, comps, 0, None) == EINVAL           # at batch 0
        assert fn(cl._h, None, None, 1, 1, 1, 0, None) == EINVAL                  # NULL terms
        bad = (T(ptr, None, 3, 0), T(ptr, None, 0, 1), T(ptr, ptr, 0, 0), T(ptr, None, 1, 0),
               T(ptr, None, 2, 0), T(None, None, 0, 0))
        for b in bad:
            for at in range(3):
                terms = [good[i] if i < at else worst for i in range(3)]
                terms[at] = b
                assert fn(cl._h, None, arr(*terms), 3, 1, 1, 0, None) == EINVAL
                assert fn(cl._h, ptr, arr(*terms), 3, 0, 1, 0, None) == EINVAL    # at batch 0
        assert fn(cl._h, None, good, 3, 1, 1, 0, None) == EINVAL                  # NULL out
        assert fn(cl._h, None, good, 3, 0, 1, 0, None) == OK
        assert fn(cl._h, None, good, 3, 0, 1, 99, None) == ENODEV
        assert fn(cl._h, ptr, good, 3, 1, 1, 99, None) == ENODEV
        assert cl._lib.nttmul_ctlin_combine(cl._h, None, good, 3, 0, 1) == OK
        assert cl._lib.nttmul_ctlin_combine(cl._h, None, good, 3, 1, 1) == EINVAL
        te = cl._lib.nttmul_ctlin_tensor_device
        assert te(cl._h, ptr, ptr, ptr, 1, 0, 0, None) == EINVAL                  # pairs = 0
        assert te(cl._h, None, None, None, 0, 0, 0, None) == EINVAL
        for hole in range(3):
            args = [None if i == hole else ptr for i in range(3)]
            assert te(cl._h, *args, 1, 1, 0, None) == EINVAL
        assert te(cl._h, None, None, None, 0, 1, 0, None) == OK
        assert te(cl._h, None, None, None, 0, 1, 99, None) == ENODEV
        assert cl._lib.nttmul_ctlin_tensor(cl._h, None, None, None, 0, 1) == OK
        assert cl._lib.nttmul_ctlin_tensor(cl._h, None, ptr, ptr, 1, 1) == EINVAL
        name = cl._lib.nttmul_ctlin_kernel_name
        assert name(cl._h, 0, 1, None, 1) == EINVAL
        assert name(cl._h, 2, 1, None, 0) == EINVAL and name(cl._h, -1, 1, None, 0) == EINVAL
        assert name(cl._h, 0, 0, None, 0) == EINVAL and name(cl._h, 0, 4, None, 0) == EINVAL
        assert name(cl._h, 1, 0, None, 0) == len("k_ctlin_tensor<Arith32P,u32>")  # comps ignored
        small = ctypes.create_string_buffer(8)
        assert name(cl._h, 0, 3, small, 8) == len("k_ctlin_combine<Arith32P,u32,3>")
        assert small.value == b"k_ctlin"


def _library_transforms(n, q, x):
    """The library's forward transform of [.., L, n] coefficient-order limbs."""
    with nttmul.RnsContext(n, q) as low:
        return low.forward(np.ascontiguousarray(x).reshape(-1, len(q), n)).reshape(x.shape)


def _library_coefficients(n, q, x_hat):
    with nttmul.RnsContext(n, q) as low:
        return low.inverse(np.ascontiguousarray(x_hat).reshape(-1, len(q), n)).reshape(x_hat.shape)


@pytest.mark.parametrize("bits", (32, 64))
def test_plaintext_product_plus_ciphertext_decrypts_exactly(bits, torch_cuda):
    """combine(pt o ct + ct') on zero-noise ciphertexts, inverted with the library's transforms
    and lifted by CRT in Python integers, decrypts to pt m + m' mod Q exactly."""
    n, q, dt = C.CHAIN_N, C.moduli_of(bits), _dt(bits)
    ch = ref.chain_setup(bits, q, 2, 17 + bits)
    Q, s = ch["Q"], ch["s"]
    rng = np.random.default_rng(bits + 1)
    pt = [ref.uniform(rng, Q) for _ in range(n)]
    ct_hat = _library_transforms(n, q, ch["cts"])                   # [2, 2, L, n]
    pt_hat = _library_transforms(n, q, ref.residues(pt, q, dt)[None])[0]
    case = C.Case("combine", bits, n, 1, 2, ((C.PLAIN, 0), (C.ONE, 1)))
    with nttmul.NttCtLin(n, q) as cl:
        out_hat = _combine(torch_cuda, cl, case, [ct_hat[0:1], ct_hat[1:2]], [pt_hat, None])
    out = _library_coefficients(n, q, out_hat)[0]
    got = ref.decrypt([ref.lift(out[c], q) for c in (0, 1)], s, Q)
    m1, m2 = ch["msgs"]
    want = [(u + v) % Q for u, v in zip(ref.negacyclic(pt, m1, Q), m2)]
    assert got == want


@pytest.mark.parametrize("bits", (32, 64))
def test_a_sum_of_two_tensors_decrypts_exactly(bits, torch_cuda):
    """tensor, then combine(comps = 3) of the two tensors: d_0 + d_1 s + d_2 s^2 is
    m_1 m_2 + m_3 m_4 mod Q exactly (the lazily relinearised sum before its one key switch)."""
    n, q, dt = C.CHAIN_N, C.moduli_of(bits), _dt(bits)
    ch = ref.chain_setup(bits, q, 4, 29 + bits)
    Q, s = ch["Q"], ch["s"]
    ct_hat = _library_transforms(n, q, ch["cts"])                   # [4, 2, L, n]
    x = np.ascontiguousarray(ct_hat[[0, 2]][:, None])               # [2, 1, 2, L, n]
    y = np.ascontiguousarray(ct_hat[[1, 3]][:, None])
    case = C.Case("combine", bits, n, 1, 3, ((C.ONE, 0), (C.ONE, 1)))
    with nttmul.NttCtLin(n, q) as cl:
        d = _tensor(torch_cuda, cl, x, y)                           # [2, 3, L, n]
        assert np.array_equal(d, ref.tensor(x, y, q))
        out_hat = _combine(torch_cuda, cl, case, [d[0:1], d[1:2]], [None, None])
    out = _library_coefficients(n, q, out_hat)[0]
    got = ref.decrypt([ref.lift(out[c], q) for c in (0, 1, 2)], s, Q)
    m1, m2, m3, m4 = ch["msgs"]
    want = [(u + v) % Q for u, v in zip(ref.negacyclic(m1, m2, Q), ref.negacyclic(m3, m4, Q))]
    assert got == want


def test_mirror_agrees_with_the_library_dispatch(torch_cuda):
    """tests/ctlin_cases.py kernel_name against nttmul_ctlin_kernel_name at every degree, and the
    names are kernels the library holds."""
    held = nttmul.kernel_hashes(nttmul.CTLIN_LIB_PATH)
    for bits in (32, 64):
        for n in C.ALL_N:
            with nttmul.NttCtLin(n, C.moduli_of(bits)) as cl:
                for comps in (1, 2, 3):
                    case = C.Case("combine", bits, n, 1, comps, ((C.ONE, 0),))
                    name = cl.kernel_name("combine", comps)
                    assert name == cl.kernel_name(0, comps) == C.kernel_name(case)
                    assert nttmul.dispatch_key(name) in held
                name = cl.kernel_name("tensor")
                assert name == C.kernel_name(C.Case("tensor", bits, n, 1, 3, ()))
                assert nttmul.dispatch_key(name) in held
