"""The caller's memory around lib/libnttmul_ksntt.so's calls (include/nttmul_ksntt.h "Caller
memory"), in the style of tests/test_gpu_mdntt_footprint.py and on tests/guarded.py as it stands:
the `_device` entry points and the host forms of both operations run between sentinel guards at
addresses aligned to the word and to nothing larger; afterwards no guard word has changed, every
input is bit-identical to the copy taken before the call, exactly the output's words are written
(the arena's output is that long, every word after it is a guard, and no word of it keeps the
sentinel), and the result is right bit for bit at every degree (tests/full_ref.py).

The rows are tests/ksntt_cases.py footprint_cases(): n = 256 with batch 1 and 33 (a half-empty
pair, partial workgroups), n = 4096 and n = 8192 with batch 1, (L, K, alpha) = (3, 2, 2) and
(5, 1, 5), both word classes.  The no-GPU half holds the rows to the header: every exported
nttmul_ksntt_* function has a row or a reason in EXEMPT."""
import ctypes

import numpy as np
import pytest

import bconv_ref as B
import full_ref as F
import guarded as G
import ksntt_cases as C
import nttmul

# exported functions that write no caller memory beyond a small result of fixed size
EXEMPT = {
    "nttmul_ksntt_create": "writes the handle only",
    "nttmul_ksntt_destroy": "writes no caller memory",
    "nttmul_ksntt_last_error": "returns a pointer into the context",
    "nttmul_ksntt_get_info": "writes one nttmul_ksntt_info",
    "nttmul_ksntt_kernel_name": "writes at most cap bytes of a name",
}


def groups():
    out = {}
    for f in C.footprint_cases():
        c = f.case
        out.setdefault((C.op_of(c), c.bits, c.n, (c.L, c.K)), []).append(f)
    return out


GROUPS = groups()


def test_every_exported_function_has_a_row_or_a_reason():
    named = {f.entry for f in C.footprint_cases()}
    exported = set(nttmul.ksntt_exported_symbols())
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


def _ids(p):
    return f"{p[0]}-u{p[1]}-n{p[2]}-{p[3][0]}.{p[3][1]}"


@pytest.mark.gpu
@pytest.mark.parametrize("param", sorted(g for g in GROUPS if g[0] == "modup"), ids=_ids)
def test_modup(param, torch_cuda):
    torch = torch_cuda
    _, bits, n, (L, K) = param
    rows = GROUPS[param]
    alpha = rows[0].case.alpha
    q, p = C.moduli_of(rows[0].case)
    B_ = max(f.case.batch for f in rows)
    x = B.random_words(np.random.default_rng(n + bits + L), q, B_, n, G.dtype_of(bits))
    # the CPU reference once, on the rows' largest batch, at every degree; above n = 512 the
    # coefficient-order chain on the device beside it, which says which side is wrong
    want = F.reference("ksntt", "modup", x, q, p, alpha)
    with nttmul.NttKeySwitch(n, q, p, alpha) as kn:
        assert kn.word_bits == bits
        if n > 512:
            Ctx = nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext
            with Ctx(n, q) as low, Ctx(n, q + p) as ext, \
                    nttmul.KeySwitchBasis(n, q, p, alpha) as ks:
                up = ks.modup(low.inverse(x))
                chain = ext.forward(up.reshape(-1, L + K, n)).reshape(up.shape)
            F.assert_equal(chain, want, ("the coefficient-order chain", param))
        for f in rows:
            c = f.case
            assert f.entry == "nttmul_ksntt_modup" + ("" if f.host else "_device")
            shape = (c.batch, C.dnum(c), L + K, n)
            operands = dict(out=int(np.prod(shape)), x=x[:c.batch])
            guard = C.fp_guard_words(c)
            if f.host:
                arena = G.HostArena(bits, guard, **operands)
                fn = getattr(kn._lib, f.entry)
                kn._check(fn(kn._h, arena["out"].ctypes.data, arena["x"].ctypes.data, c.batch))
            else:
                arena = G.DeviceArena(torch, bits, guard, **operands)
                s = torch.cuda.current_stream().cuda_stream
                kn.modup_device(arena["out"], arena["x"], c.batch, stream=s)
                torch.cuda.synchronize()
            arena.check()
            assert np.array_equal(arena.get("out", shape), want[:c.batch]), f


@pytest.mark.gpu
@pytest.mark.parametrize("param", sorted(g for g in GROUPS if g[0] == "mac"), ids=_ids)
def test_mac(param, torch_cuda):
    torch = torch_cuda
    _, bits, n, (L, K) = param
    rows = GROUPS[param]
    c0 = rows[0].case
    q, p = C.moduli_of(c0)
    ext, M = q + p, L + K
    terms, comps, ks = c0.terms, c0.comps, c0.ks
    B_ = max(f.case.batch for f in rows)
    rng = np.random.default_rng(n + bits + L + 1)
    a = B.random_words(rng, ext * terms, B_, n, G.dtype_of(bits)).reshape(B_, terms, M, n)
    b = B.random_words(rng, ext * (terms * comps), len(ks), n, G.dtype_of(bits)).reshape(
        len(ks), comps, terms, M, n)
    want = F.reference("ksntt", "mac", a, b, ks, ext)
    karr = (ctypes.c_uint32 * len(ks))(*ks)
    with nttmul.NttKeySwitch(n, q, p, 1) as kn:
        for f in rows:
            c = f.case
            assert (c.terms, c.comps, c.ks) == (terms, comps, ks)
            assert f.entry == "nttmul_ksntt_mac" + ("" if f.host else "_device")
            shape = (c.batch, len(ks), comps, M, n)
            operands = dict(out=int(np.prod(shape)), a=a[:c.batch], b=b)
            guard = C.fp_guard_words(c)
            if f.host:
                arena = G.HostArena(bits, guard, **operands)
                fn = getattr(kn._lib, f.entry)
                kn._check(fn(kn._h, arena["out"].ctypes.data, arena["a"].ctypes.data,
                             arena["b"].ctypes.data, karr, len(ks), c.batch, terms, comps))
            else:
                arena = G.DeviceArena(torch, bits, guard, **operands)
                s = torch.cuda.current_stream().cuda_stream
                kn.mac_device(arena["out"], arena["a"], arena["b"], ks, c.batch, terms, comps,
                              stream=s)
                torch.cuda.synchronize()
            arena.check()
            assert np.array_equal(arena.get("out", shape), want[:c.batch]), f
