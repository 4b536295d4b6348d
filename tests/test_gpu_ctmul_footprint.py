"""The caller's memory around lib/libnttmul_ctmul.so's calls (include/nttmul_ctmul.h "Caller
memory"), in the style of tests/test_gpu_lintrans_footprint.py and on tests/guarded.py as it
stands: the `_device` entry points and the host forms run between sentinel guards at addresses
aligned to the word and to nothing larger; afterwards no guard word has changed, every input is
bit-identical to the copy taken before the call, exactly the output's words are written (the
arena's output is that long, every word after it is a guard, and no word of it keeps the
sentinel), and the result is right bit for bit.

The rows are tests/ctmul_cases.py footprint_cases(): n = 256 and n = 8192 with batch V + 1 (a
partial last workgroup), (L, K) = (3, 2), y_hat a buffer of its own and x_hat itself in turn, both
word classes.  The no-GPU half holds the rows to the header: every exported nttmul_ctmul_* function
has a row or a reason in EXEMPT."""
import numpy as np
import pytest

import bconv_ref as B
import ctmul_cases as C
import ctmul_ref as ref
import full_ref as F
import guarded as G
import nttmul

# exported functions that write no caller memory beyond a small result of fixed size
EXEMPT = {
    "nttmul_ctmul_create": "writes the handle only",
    "nttmul_ctmul_destroy": "writes no caller memory",
    "nttmul_ctmul_last_error": "returns a pointer into the context",
    "nttmul_ctmul_get_info": "writes one nttmul_ctmul_info",
    "nttmul_ctmul_kernel_name": "writes at most cap bytes of a name",
}


def groups():
    out = {}
    for f in C.footprint_cases():
        out.setdefault((f.case.op, f.case.bits, f.case.n), []).append(f)
    return out


GROUPS = groups()


def test_every_exported_function_has_a_row_or_a_reason():
    named = {f.entry for f in C.footprint_cases()}
    exported = set(nttmul.ctmul_exported_symbols())
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


@pytest.mark.gpu
@pytest.mark.parametrize("param", sorted(GROUPS), ids=lambda p: f"{p[0]}-u{p[1]}-n{p[2]}")
def test_calls(param, torch_cuda):
    torch = torch_cuda
    op, bits, n = param
    rows = GROUPS[param]
    first = rows[0].case
    q, p = C.moduli_of(first)
    L, K, M = first.L, first.K, first.L + first.K
    pairs, terms, batch = first.pairs, first.terms, first.batch
    rng, dt = np.random.default_rng(n + bits + 1), G.dtype_of(bits)
    up = B.random_words(rng, (q + p) * terms, batch, n, dt).reshape(batch, terms, M, n)
    key = B.random_words(rng, (q + p) * terms, 2, n, dt).reshape(2, terms, M, n)
    x = B.random_words(rng, q * (2 * pairs), batch, n, dt).reshape(batch, pairs, 2, L, n)
    y = B.random_words(rng, q * (2 * pairs), batch, n, dt).reshape(batch, pairs, 2, L, n)
    shape = (batch, L, n) if op == "high" else (batch, 2, M, n)
    want = {}
    with nttmul.NttCtMul(n, q, p) as ct:
        assert ct.word_bits == bits
        for f in rows:
            c = f.case
            assert (c.pairs, c.terms, c.batch, c.op) == (pairs, terms, batch, op)
            assert f.entry == f"nttmul_ctmul_{op}" + ("" if f.host else "_device")
            yy = x if c.square else y
            if c.square not in want:             # the reference once per form of the call
                want[c.square] = _reference(op, n, up, key, x, yy, q, p)
            operands = dict(out=int(np.prod(shape)))
            if op == "relin":
                operands.update(up=up, key=key)
            operands["x"] = x
            if not c.square:
                operands["y"] = y
            guard = C.fp_guard_words(c)
            host = bool(f.host)
            arena = G.HostArena(bits, guard, **operands) if host else \
                G.DeviceArena(torch, bits, guard, **operands)
            xp = _ptr(arena["x"], host)
            yp = xp if c.square else _ptr(arena["y"], host)
            fn = getattr(ct._lib, f.entry)
            tail = () if host else (0, torch.cuda.current_stream().cuda_stream or None)
            if op == "high":
                ct._check(fn(ct._h, _ptr(arena["out"], host), xp, yp, batch, pairs, *tail))
            else:
                ct._check(fn(ct._h, _ptr(arena["out"], host), _ptr(arena["up"], host),
                             _ptr(arena["key"], host), xp, yp, batch, pairs, terms, *tail))
            if not host:
                torch.cuda.synchronize()
            arena.check()
            assert np.array_equal(arena.get("out", shape), want[c.square]), f


def _reference(op, n, up, key, x, y, q, p):
    """The CPU reference of every output word (tests/full_ref.py) at every n; above n = 512 the
    composition of existing calls is held to it as well, which says which side is wrong."""
    want = F.reference("ctmul", "high", x, y, q) if op == "high" else \
        F.reference("ctmul", "relin", up, key, x, y, q, p)
    if n <= 512:
        return want
    plain = [nttmul.Context(n, m) for m in q]
    try:
        if op == "high":
            comp = ref.tensor_composition(plain, x, y, q)[2]
        else:
            with nttmul.NttKeySwitch(n, q, p, 1) as kn:
                comp = ref.composition(kn, plain, up, key, x, y, q, p)
    finally:
        for c in plain:
            c.close()
    F.assert_equal(comp, want, ("the composition", op, n))
    return want
