"""What the GPU tests of include/nttmul_xconv.h share (tests/test_gpu_xconv*.py): one call out of
a guarded arena, and the device composition the library is compared with where Python integers do
not reach every coefficient -- the library's own inverse transforms over the input's limbs, the
reference arithmetic of tests/xconv_ref.py on a sample of coefficients (first, last, one per 1/64),
the library's inverse over Q of the output."""
import numpy as np

import guarded as G
import nttmul
import xconv_cases as C
import xconv_ref as ref


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


def want_sampled(op, coef, q, p, t, idx):
    """The reference on the coefficients idx of coef [batch, limbs, n] (coefficient order)."""
    fn = ref.extend_coeff if op == "extend" else ref.moddown_coeff
    return fn(coef[:, :, idx], q, p, t)


def check_composition(op, n, q, p, t, src, got):
    """got against the reference on the sampled coefficients, through the library's transforms."""
    idx = C.sample_indices(n)
    Ctx = ctx(n)
    with Ctx(n, tuple(p) if op == "extend" else tuple(q) + tuple(p)) as wide, Ctx(n, q) as low:
        coef = wide.inverse(src)
        back = low.inverse(got)
    assert np.array_equal(back[:, :, idx], want_sampled(op, coef, q, p, t, idx))


def check(op, n, q, p, t, src, got):
    """The composition at every n, and every coefficient bit for bit up to REF_MAX_N."""
    check_composition(op, n, q, p, t, src, got)
    if n <= C.REF_MAX_N:
        assert np.array_equal(got, getattr(ref, op)(src, q, p, t))
