"""The caller's memory around lib/libnttmul_galois.so's calls (include/nttmul_galois.h "Caller
memory"), in the style of tests/test_gpu_rnsmp_footprint.py and on tests/guarded.py as it stands:
the three `_device` entry points and the two host forms run between sentinel guards at addresses
aligned to the word and to nothing larger; afterwards no guard word and no input has changed, every
output word is written, and the result is right bit for bit.

The rows are tests/galois_cases.py footprint_cases(): n = 256 and 65536, both word classes, L = 3,
batch 1 and 5.  At n = 256 a workgroup holds four polynomials of a limb: batch 5 is one whole
workgroup and a partial one, batch 1 a partial one alone.  tests/test_galois_ledger.py holds the
rows to the header without a GPU."""
import numpy as np
import pytest

import galois_cases as C
import galois_ref as ref
import guarded as G
import nttmul


def groups():
    out = {}
    for f in C.footprint_cases():
        out.setdefault((f.case.n, C.word_bits(f.case.moduli)), []).append(f)
    return out


GROUPS = groups()


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.gpu
@pytest.mark.parametrize("param", sorted(GROUPS), ids=lambda p: f"{p[0]}-u{p[1]}")
def test_galois(param, torch_cuda):
    torch = torch_cuda
    n, bits = param
    rows = GROUPS[param]
    moduli = rows[0].case.moduli
    L = len(moduli)
    B_ = max(f.case.batch for f in rows)
    x = ref.random_words(np.random.default_rng(n + bits), moduli, B_, n, G.dtype_of(bits))
    want = {}
    with nttmul.GaloisContext(n, moduli) as ctx:
        assert ctx.word_bits == bits
        for f in rows:
            c = f.case
            assert c.moduli == moduli and f.entry == C.ENTRY[c.op] + ("" if f.host else "_device")
            batch, count = c.batch, len(c.ks)
            for k in c.ks:
                if (c.op == "coeff", k) not in want:
                    want[(c.op == "coeff", k)] = (ref.coeff(x, k, moduli) if c.op == "coeff"
                                                  else ref.ntt(x, k))
            exp = np.stack([want[(c.op == "coeff", k)][:batch] for k in c.ks])
            operands = dict(out=count * batch * L * n, x=x[:batch])
            guard = C.fp_guard_words(c)
            if f.host:
                arena = G.HostArena(bits, guard, **operands)
                fn = getattr(ctx._lib, f.entry)
                ctx._check(fn(ctx._h, arena["out"].ctypes.data, arena["x"].ctypes.data, c.ks[0],
                              batch))
            else:
                arena = G.DeviceArena(torch, bits, guard, **operands)
                s = torch.cuda.current_stream().cuda_stream
                if c.op == "ntt_many":
                    ctx.ntt_many_device(arena["out"], arena["x"], c.ks, batch, stream=s)
                else:
                    getattr(ctx, f"{c.op}_device")(arena["out"], arena["x"], c.ks[0], batch,
                                                   stream=s)
                torch.cuda.synchronize()
            arena.check()
            got = arena.get("out", (count, batch, L, n))
            assert np.array_equal(got, exp), f
