"""The caller's memory around lib/libnttmul_ks.so's calls (include/nttmul_ks.h "Caller memory"), in
the style of tests/test_gpu_galois_footprint.py and on tests/guarded.py as it stands: the two
`_device` entry points and the two host forms run between sentinel guards at addresses aligned to
the word and to nothing larger; afterwards no guard word and no input has changed, exactly the
stated output words are written (batch * dnum * (L + K) * n for modup, batch * L * n for moddown:
the arena's output is that long and every word after it is a guard), and the result is right bit
for bit.

The rows are tests/ks_cases.py footprint_cases(): n = 256 with batch 1 and 5 (partial workgroups
on 32-bit words) and n = 4096 with batch 1, (L, K, alpha) = (3, 2, 2) and (5, 1, 5), both word
classes.  The no-GPU half holds the rows to the header: every exported nttmul_ks_* function has a
row or a reason in EXEMPT."""
import numpy as np
import pytest

import bconv_ref as B
import guarded as G
import ks_cases as C
import ks_ref as ref
import nttmul

# exported functions that write no caller memory beyond a small result of fixed size
EXEMPT = {
    "nttmul_ks_create": "writes the handle only",
    "nttmul_ks_destroy": "writes no caller memory",
    "nttmul_ks_last_error": "returns a pointer into the context",
    "nttmul_ks_get_info": "writes one nttmul_ks_info",
    "nttmul_ks_plan": "host-only tables of stated sizes: test_ks_abi.py, sanitize/ks_san.cpp",
    "nttmul_ks_kernel_name": "writes at most cap bytes of a name",
}


def groups():
    out = {}
    for f in C.footprint_cases():
        c = f.case
        out.setdefault((c.bits, c.n, (c.L, c.K, c.alpha)), []).append(f)
    return out


GROUPS = groups()


def test_every_exported_function_has_a_row_or_a_reason():
    named = {f.entry for f in C.footprint_cases()}
    exported = set(nttmul.ks_exported_symbols())
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
                         ids=lambda p: f"u{p[0]}-n{p[1]}-{p[2][0]}.{p[2][1]}.{p[2][2]}")
def test_ks(param, torch_cuda):
    torch = torch_cuda
    bits, n, (L, K, alpha) = param
    rows = GROUPS[param]
    q, p = ref.bases(bits, L, K)
    M, dn = L + K, -(-L // alpha)
    B_ = max(f.case.batch for f in rows)
    x = {"modup": B.random_words(np.random.default_rng(n + bits), q, B_, n, G.dtype_of(bits)),
         "moddown": B.random_words(np.random.default_rng(n + bits + 1), q + p, B_, n,
                                   G.dtype_of(bits))}
    want = {"modup": ref.modup(x["modup"], q, p, alpha), "moddown": B.moddown(x["moddown"], p, q)}
    with nttmul.KeySwitchBasis(n, q, p, alpha) as ks:
        assert ks.word_bits == bits and ks.digits == dn
        for f in rows:
            c = f.case
            assert f.entry == f"nttmul_ks_{c.op}" + ("" if f.host else "_device")
            batch = c.batch
            shape = (batch, dn, M, n) if c.op == "modup" else (batch, L, n)
            operands = dict(out=int(np.prod(shape)), x=x[c.op][:batch])
            guard = C.fp_guard_words(c)
            if f.host:
                arena = G.HostArena(bits, guard, **operands)
                fn = getattr(ks._lib, f.entry)
                ks._check(fn(ks._h, arena["out"].ctypes.data, arena["x"].ctypes.data, batch))
            else:
                arena = G.DeviceArena(torch, bits, guard, **operands)
                s = torch.cuda.current_stream().cuda_stream
                getattr(ks, f"{c.op}_device")(arena["out"], arena["x"], batch, stream=s)
                torch.cuda.synchronize()
            arena.check()
            assert np.array_equal(arena.get("out", shape), want[c.op][:batch]), f
