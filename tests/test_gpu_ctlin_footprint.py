"""The caller's memory around lib/libnttmul_ctlin.so's calls (include/nttmul_ctlin.h "Caller
memory"), in the style of tests/test_gpu_ctmul_footprint.py and on tests/guarded.py as it stands:
the `_device` entry points and the host forms run between sentinel guards at addresses aligned to
the word and to nothing larger; afterwards no guard word has changed, every input is bit-identical
to the copy taken before the call, exactly the output's words are written (the arena's output is
that long, every word after it is a guard, and no word of it keeps the sentinel), and the result
is right bit for bit.

The rows are tests/ctlin_cases.py footprint_cases(): n = 256 with batch 5 (a partial last
workgroup) and n = 8192 with batch 3, L = 3, both word classes; combine out of place and in place
(out is x_0, which is then held to the output rule and every other operand to the input rule),
tensor with y_hat a buffer of its own and x_hat itself.  The no-GPU half holds the rows to the
header: every exported nttmul_ctlin_* function has a row or a reason in EXEMPT."""
import numpy as np
import pytest

import bconv_ref as B
import ctlin_cases as C
import ctlin_ref as ref
import full_ref as F
import guarded as G
import nttmul

# exported functions that write no caller memory beyond a small result of fixed size
EXEMPT = {
    "nttmul_ctlin_create": "writes the handle only",
    "nttmul_ctlin_destroy": "writes no caller memory",
    "nttmul_ctlin_last_error": "returns a pointer into the context",
    "nttmul_ctlin_get_info": "writes one nttmul_ctlin_info",
    "nttmul_ctlin_kernel_name": "writes at most cap bytes of a name",
}


def groups():
    out = {}
    for f in C.footprint_cases():
        out.setdefault((f.case.op, f.case.bits, f.case.n), []).append(f)
    return out


GROUPS = groups()


def test_every_exported_function_has_a_row_or_a_reason():
    named = {f.entry for f in C.footprint_cases()}
    exported = set(nttmul.ctlin_exported_symbols())
    assert named <= exported and set(EXEMPT) <= exported
    assert not named & set(EXEMPT)
    assert sorted(exported - named - set(EXEMPT)) == []
    assert all(EXEMPT.values())
    for entry in named:
        for host in ("", "host"):
            assert any(f.entry == entry and f.host == host for f in C.footprint_cases()) == \
                (entry.endswith("_device") != bool(host))


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _ptr(view, host):
    return view.ctypes.data if host else view.data_ptr()


def _reference(case, terms, x, y, q, dt):
    """The CPU reference of every output word (tests/full_ref.py) at every n; above n = 512 the
    composition of existing calls is held to it as well, which says which side is wrong."""
    shape = (case.batch, case.comps, C.L, case.n)
    want = F.reference("ctlin", "combine", terms, q, shape, dt) if case.op == "combine" else \
        F.reference("ctlin", "tensor", x, y, q)
    if case.n <= 512:
        return want
    plain = [nttmul.Context(case.n, m) for m in q]
    try:
        if case.op == "combine":
            comp = ref.composition(plain, terms, q, shape, dt)
        else:
            comp = ref.tensor_composition(plain, x, y, q)
    finally:
        for c in plain:
            c.close()
    F.assert_equal(comp, want, ("the composition", case))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("param", sorted(GROUPS), ids=lambda p: f"{p[0]}-u{p[1]}-n{p[2]}")
def test_calls(param, torch_cuda):
    torch = torch_cuda
    op, bits, n = param
    rows = GROUPS[param]
    first = rows[0].case
    q, dt, batch = C.moduli_of(first), G.dtype_of(bits), first.batch
    rng = np.random.default_rng(n + bits + 1)
    shape = (batch, first.comps, C.L, n)
    tail_dev = (0, torch.cuda.current_stream().cuda_stream or None)
    with nttmul.NttCtLin(n, q) as cl:
        assert cl.word_bits == bits
        if op == "tensor":
            pshape = (batch, first.pairs, 2, C.L, n)
            x = B.random_words(rng, q * (2 * first.pairs), batch, n, dt).reshape(pshape)
            y = B.random_words(rng, q * (2 * first.pairs), batch, n, dt).reshape(pshape)
            want = {}
            for f in rows:
                c, host = f.case, bool(f.host)
                assert f.entry == "nttmul_ctlin_tensor" + ("" if host else "_device")
                if c.square not in want:
                    want[c.square] = _reference(c, None, x, x if c.square else y, q, dt)
                operands = dict(out=int(np.prod(shape)), x=x)
                if not c.square:
                    operands["y"] = y
                guard = C.fp_guard_words(c)
                arena = G.HostArena(bits, guard, **operands) if host else \
                    G.DeviceArena(torch, bits, guard, **operands)
                xp = _ptr(arena["x"], host)
                yp = xp if c.square else _ptr(arena["y"], host)
                cl._check(getattr(cl._lib, f.entry)(cl._h, _ptr(arena["out"], host), xp, yp, batch,
                                                    c.pairs, *(() if host else tail_dev)))
                if not host:
                    torch.cuda.synchronize()
                arena.check()
                assert np.array_equal(arena.get("out", shape), want[c.square]), f
            return
        count = C.x_count(first)
        xs = [B.random_words(rng, q * first.comps, batch, n, dt).reshape(shape)
              for _ in range(count)]
        ws = [None if kind == C.ONE else
              np.array([int(rng.integers(0, m, dtype=np.uint64)) for m in q], dtype=dt)
              if kind == C.SCALAR else B.random_words(rng, q, 1, n, dt)[0]
              for kind, _ in first.terms]
        terms = [(None if i is None else xs[i], w, C.KIND_CODE[kind])
                 for (kind, i), w in zip(first.terms, ws)]
        want = _reference(first, terms, None, None, q, dt)
        for f in rows:
            c, host = f.case, bool(f.host)
            assert f.entry == "nttmul_ctlin_combine" + ("" if host else "_device")
            assert c.terms == first.terms and c.batch == batch
            operands = {} if c.inplace else dict(out=int(np.prod(shape)))
            operands.update({f"x{i}": v for i, v in enumerate(xs)})
            operands.update({f"w{t}": w for t, w in enumerate(ws) if w is not None})
            inplace = tuple(f"x{i}" for i in c.inplace)
            guard = C.fp_guard_words(c)
            arena = G.HostArena(bits, guard, inplace=inplace, **operands) if host else \
                G.DeviceArena(torch, bits, guard, inplace=inplace, **operands)
            out = inplace[0] if inplace else "out"
            arr = (nttmul.CtLinTerm * len(c.terms))()
            for t, ((kind, i), w) in zip(arr, zip(c.terms, range(len(c.terms)))):
                t.x = None if i is None else _ptr(arena[f"x{i}"], host)
                t.w = None if kind == C.ONE else _ptr(arena[f"w{w}"], host)
                t.kind, t.reserved = C.KIND_CODE[kind], 0
            cl._check(getattr(cl._lib, f.entry)(cl._h, _ptr(arena[out], host), arr, len(c.terms),
                                                batch, c.comps, *(() if host else tail_dev)))
            if not host:
                torch.cuda.synchronize()
            arena.check()
            assert np.array_equal(arena.get(out, shape), want), f
