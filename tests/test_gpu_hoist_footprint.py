"""The caller's memory around lib/libnttmul_hoist.so's calls (include/nttmul_hoist.h "Caller
memory"), in the manner of tests/test_gpu_macn_footprint.py and on tests/guarded.py as it stands:
the two `_device` entry points and the two host forms run between sentinel guards at addresses
aligned to the word and to nothing larger; afterwards no guard word and no input has changed,
exactly batch * rots * comps * limbs * n words of c are written (the arena's output is that long
and every word after it is a guard), and every result equals tests/hoist_ref.py's Python integers
bit for bit.

The rows are tests/hoist_cases.py footprint_cases(): n = 256 with batch 1 and 5 (both end in a
partial workgroup) and n = 4096 with batch 1 on nttmul_rns, n = 8192 with batch 1 and 5 on
nttmul_rnsmp, three limbs, three terms, two components, three rotations, both word classes.  The
no-GPU half holds the rows to the header: every function it declares has a row or a reason in
EXEMPT."""
import ctypes

import numpy as np
import pytest

import bconv_ref as B
import guarded as G
import hoist_cases as C
import hoist_ref as H
import nttmul

# exported functions that write no caller memory beyond a small result of fixed size
EXEMPT = {
    "nttmul_rns_hoist_kernel_name": "writes at most cap bytes of a name",
    "nttmul_rnsmp_hoist_kernel_name": "writes at most cap bytes of a name",
}


def groups():
    out = {}
    for f in C.footprint_cases():
        out.setdefault((C.word_bits(f.case.moduli), f.case.n), []).append(f)
    return out


GROUPS = groups()


def test_every_exported_function_has_a_row_or_a_reason():
    named = {f.entry for f in C.footprint_cases()}
    exported = set(nttmul.hoist_exported_symbols())
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
def test_hoist(param, torch_cuda):
    torch = torch_cuda
    bits, n = param
    rows = GROUPS[param]
    moduli, ks = rows[0].case.moduli, rows[0].case.ks
    L, terms, rots, dt = len(moduli), C.FP_TERMS, C.FP_ROTS, G.dtype_of(bits)
    B_ = max(f.case.batch for f in rows)
    rng = np.random.default_rng(n + bits)
    a = B.random_words(rng, moduli, B_ * terms, n, dt).reshape(B_, terms, L, n)
    bh = B.random_words(rng, moduli, rots * 2 * terms, n, dt).reshape(rots, 2, terms, L, n)
    want = H.hoist(a, bh, ks, moduli)                     # once, shared by the rows
    assert not np.array_equal(want[:, 0], want[:, 1])
    karr = (ctypes.c_uint32 * rots)(*ks)
    cls = nttmul.RnsHoistContext if C.family(n) == "rns" else nttmul.RnsMpHoistContext
    with cls(n, moduli) as ctx:
        assert ctx.word_bits == bits
        for f in rows:
            c = f.case
            assert f.entry == f"nttmul_{C.family(n)}_hoist_ntt" + ("" if f.host else "_device")
            assert (c.terms, c.comps, c.moduli, c.ks) == (terms, 2, moduli, ks)
            batch = c.batch
            shape = (batch, rots, 2, L, n)
            operands = dict(c=int(np.prod(shape)), a=a[:batch], b=bh)
            guard = C.fp_guard_words(c)
            if f.host:
                arena = G.HostArena(bits, guard, **operands)
                fn = getattr(ctx._lib, f.entry)
                ctx._check(fn(ctx._h, arena["c"].ctypes.data, arena["a"].ctypes.data,
                              arena["b"].ctypes.data, karr, rots, batch, terms, 2))
            else:
                arena = G.DeviceArena(torch, bits, guard, **operands)
                s = torch.cuda.current_stream().cuda_stream
                ctx.hoist_ntt_device(arena["c"], arena["a"], arena["b"], ks, batch, terms, 2,
                                     stream=s)
                torch.cuda.synchronize()
            arena.check()
            assert np.array_equal(arena.get("c", shape), want[:batch]), f
