"""The caller's memory around lib/libnttmul_lintrans.so's call (include/nttmul_lintrans.h "Caller
memory"), in the style of tests/test_gpu_ksntt_footprint.py and on tests/guarded.py as it stands:
the `_device` entry point and the host form run between sentinel guards at addresses aligned to
the word and to nothing larger; afterwards no guard word has changed, every input is bit-identical
to the copy taken before the call, exactly the output's words are written (the arena's output is
that long, every word after it is a guard, and no word of it keeps the sentinel), and the result
is right bit for bit: the CPU reference of every output word (tests/full_ref.py) at both degrees.

The rows are tests/lintrans_cases.py footprint_cases(): n = 256 and n = 8192 with batch V + 1 (a
partial last workgroup), (L, K) = (3, 2), w_hat and c0_hat given and NULL in turn, both word
classes.  The no-GPU half holds the rows to the header: every exported nttmul_lintrans_* function
has a row or a reason in EXEMPT."""
import ctypes

import numpy as np
import pytest

import bconv_ref as B
import full_ref as F
import guarded as G
import lintrans_cases as C
import lintrans_ref as ref
import nttmul

# exported functions that write no caller memory beyond a small result of fixed size
EXEMPT = {
    "nttmul_lintrans_create": "writes the handle only",
    "nttmul_lintrans_destroy": "writes no caller memory",
    "nttmul_lintrans_last_error": "returns a pointer into the context",
    "nttmul_lintrans_get_info": "writes one nttmul_lintrans_info",
    "nttmul_lintrans_kernel_name": "writes at most cap bytes of a name",
}


def groups():
    out = {}
    for f in C.footprint_cases():
        out.setdefault((f.case.bits, f.case.n), []).append(f)
    return out


GROUPS = groups()


def test_every_exported_function_has_a_row_or_a_reason():
    named = {f.entry for f in C.footprint_cases()}
    exported = set(nttmul.lintrans_exported_symbols())
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


@pytest.mark.gpu
@pytest.mark.parametrize("param", sorted(GROUPS), ids=lambda p: f"u{p[0]}-n{p[1]}")
def test_apply(param, torch_cuda):
    torch = torch_cuda
    bits, n = param
    rows = GROUPS[param]
    first = rows[0].case
    q, p = C.moduli_of(first)
    L, K, M = first.L, first.K, first.L + first.K
    terms, comps, ks, batch = first.terms, first.comps, first.ks, first.batch
    rng, dt = np.random.default_rng(n + bits + 1), G.dtype_of(bits)
    a = B.random_words(rng, (q + p) * terms, batch, n, dt).reshape(batch, terms, M, n)
    b = B.random_words(rng, (q + p) * (terms * comps), len(ks), n, dt).reshape(
        len(ks), comps, terms, M, n)
    w = B.random_words(rng, q + p, len(ks), n, dt)
    c0 = B.random_words(rng, q, batch, n, dt)
    karr = (ctypes.c_uint32 * len(ks))(*ks)
    shape = (batch, comps, M, n)
    want = {}
    with nttmul.NttLinTrans(n, q, p) as lt, nttmul.NttKeySwitch(n, q, p, 1) as kn:
        assert lt.word_bits == bits
        for f in rows:
            c = f.case
            assert (c.terms, c.comps, c.ks, c.batch) == (terms, comps, ks, batch)
            assert f.entry == "nttmul_lintrans_apply" + ("" if f.host else "_device")
            wv, zv = (w if c.weighted else None), (c0 if c.c0 else None)
            if (c.weighted, c.c0) not in want:   # the reference once per form of the call
                want[c.weighted, c.c0] = F.reference("lintrans", "apply", a, b, ks, q, p, wv, zv)
                if n > 512:                      # the composition beside it: which side is wrong
                    F.assert_equal(ref.composition(kn, a, b, ks, q, p, wv, zv),
                                   want[c.weighted, c.c0], ("the composition", f))
            operands = dict(out=int(np.prod(shape)), a=a, b=b)
            if c.weighted:
                operands["w"] = w
            if c.c0:
                operands["z"] = c0
            guard = C.fp_guard_words(c)
            if f.host:
                arena = G.HostArena(bits, guard, **operands)
                fn = getattr(lt._lib, f.entry)
                lt._check(fn(lt._h, arena["out"].ctypes.data, arena["a"].ctypes.data,
                             arena["b"].ctypes.data,
                             arena["w"].ctypes.data if c.weighted else None,
                             arena["z"].ctypes.data if c.c0 else None, karr, len(ks), batch,
                             terms, comps))
            else:
                arena = G.DeviceArena(torch, bits, guard, **operands)
                s = torch.cuda.current_stream().cuda_stream
                lt.apply_device(arena["out"], arena["a"], arena["b"], ks, batch, terms, comps,
                                w_hat=arena["w"] if c.weighted else None,
                                c0_hat=arena["z"] if c.c0 else None, stream=s)
                torch.cuda.synchronize()
            arena.check()
            assert np.array_equal(arena.get("out", shape), want[c.weighted, c.c0]), f
