"""What the GPU tests of include/nttmul_xconv.h share (tests/test_gpu_xconv*.py): one call out of
a guarded arena, and the two comparisons every result gets at every degree -- the NTT-domain output
against the CPU reference of every word (tests/full_ref.py over tests/xconv_ref.py and the oracle's
transforms, which share no code with the device), and beside it the device composition on every
coefficient: the library's own inverse transforms over the input's limbs, the same reference
arithmetic, the library's inverse over Q of the output.  The composition says which side is wrong
when the first comparison fails."""
import numpy as np

import full_ref as F
import guarded as G
import nttmul


def dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def to_dev(torch, x, bits):
    x = np.ascontiguousarray(x, dtype=dt(bits))
    return torch.from_numpy(x.view(np.int32 if bits == 32 else np.int64).reshape(-1)).cuda()


def ctx(n):
    return nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext


def call(torch, xc, op, src, stream=0):
    """One device call on a numpy operand, out of a guarded arena: both operands between sentinel
    guards, aligned to their word only, the output preset to the sentinel; after the call no guard
    word and no input word has changed and every output word is written."""
    bits, batch = xc.word_bits, src.shape[0]
    shape = (batch, xc.q_limbs, xc.n)
    arena = G.DeviceArena(torch, bits, G.guard_words(max(src.shape[1], xc.q_limbs) * xc.n),
                          out=int(np.prod(shape)), x=src)
    getattr(xc, f"{op}_device")(arena["out"], arena["x"], batch, stream=stream)
    torch.cuda.synchronize()
    arena.check()
    return arena.get("out", shape)


def check(op, n, q, p, t, src, got):
    """got [batch, L, n] against the CPU reference on every word of the NTT-domain output, bit for
    bit, at every n; then the composition through the library's transforms, on every coefficient:
    the library's inverse of the input is the oracle's, and its inverse of the output is the
    reference's coefficients."""
    src_coef, want_coef, want = F.conversion("xconv", op, src, q, p, t, with_input=True)
    F.assert_equal(got, want, (op, n, t))
    Ctx = ctx(n)
    with Ctx(n, tuple(p) if op == "extend" else tuple(q) + tuple(p)) as wide, Ctx(n, q) as low:
        coef = wide.inverse(src)
        back = low.inverse(got)
    assert np.array_equal(coef, src_coef), "the library's inverse of the input"
    assert np.array_equal(back, want_coef), "the library's inverse of the output"
