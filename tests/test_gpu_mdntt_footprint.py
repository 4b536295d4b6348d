"""The caller's memory around lib/libnttmul_mdntt.so's calls (include/nttmul_mdntt.h "Caller
memory"), in the style of tests/test_gpu_ks_footprint.py and on tests/guarded.py as it stands: the
`_device` entry point and the host form run between sentinel guards at addresses aligned to the
word and to nothing larger; afterwards no guard word has changed, x_hat is bit-identical to the
copy taken before the call, exactly batch * L * n words of out are written (the arena's output is
that long and every word after it is a guard), and the result is right bit for bit
(tests/mdntt_ref.py).

The rows are tests/mdntt_cases.py footprint_cases(): n = 256 with batch 1 and 33 (a half-empty
pair, partial workgroups), n = 4096 and n = 8192 with batch 1, (L, K) = (3, 2) and (5, 1), both
word classes.  The no-GPU half holds the rows to the header: every exported nttmul_mdntt_*
function has a row or a reason in EXEMPT."""
import numpy as np
import pytest

import bconv_ref as B
import guarded as G
import mdntt_cases as C
import mdntt_ref as ref
import nttmul

# exported functions that write no caller memory beyond a small result of fixed size
EXEMPT = {
    "nttmul_mdntt_create": "writes the handle only",
    "nttmul_mdntt_destroy": "writes no caller memory",
    "nttmul_mdntt_last_error": "returns a pointer into the context",
    "nttmul_mdntt_get_info": "writes one nttmul_mdntt_info",
    "nttmul_mdntt_kernel_name": "writes at most cap bytes of a name",
}


def groups():
    out = {}
    for f in C.footprint_cases():
        c = f.case
        out.setdefault((c.bits, c.n, (c.L, c.K)), []).append(f)
    return out


GROUPS = groups()


def test_every_exported_function_has_a_row_or_a_reason():
    named = {f.entry for f in C.footprint_cases()}
    exported = set(nttmul.mdntt_exported_symbols())
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
@pytest.mark.parametrize("param", sorted(GROUPS),
                         ids=lambda p: f"u{p[0]}-n{p[1]}-{p[2][0]}.{p[2][1]}")
def test_moddown(param, torch_cuda):
    torch = torch_cuda
    bits, n, (L, K) = param
    rows = GROUPS[param]
    q, p = C.moduli_of(rows[0].case)
    B_ = max(f.case.batch for f in rows)
    x = B.random_words(np.random.default_rng(n + bits + L), q + p, B_, n, G.dtype_of(bits))
    want = ref.moddown(x, q, p)
    with nttmul.NttModDown(n, q, p) as md:
        assert md.word_bits == bits
        for f in rows:
            c = f.case
            assert f.entry == "nttmul_mdntt_moddown" + ("" if f.host else "_device")
            shape = (c.batch, L, n)
            operands = dict(out=int(np.prod(shape)), x=x[:c.batch])
            guard = C.fp_guard_words(c)
            if f.host:
                arena = G.HostArena(bits, guard, **operands)
                fn = getattr(md._lib, f.entry)
                md._check(fn(md._h, arena["out"].ctypes.data, arena["x"].ctypes.data, c.batch))
            else:
                arena = G.DeviceArena(torch, bits, guard, **operands)
                s = torch.cuda.current_stream().cuda_stream
                md.moddown_device(arena["out"], arena["x"], c.batch, stream=s)
                torch.cuda.synchronize()
            arena.check()
            assert np.array_equal(arena.get("out", shape), want[:c.batch]), f
