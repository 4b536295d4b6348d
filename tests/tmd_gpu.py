"""What the GPU tests of include/nttmul_tmd.h share (tests/test_gpu_tmd*.py): one call out of a
guarded arena (tests/xconv_gpu.py call), the CPU reference of every output word at every degree
(tests/full_ref.py), and the identity the library is compared with beside it:

    out = nttmul_mdntt_moddown(x_hat) - forward_Q(u mod q_l)       bit for bit

with u from the library's own inverse transforms of the P limbs and tests/tmd_ref.py's Python
integers, the floor form from lib/libnttmul_mdntt.so and the forward transform the library's."""
import numpy as np

import full_ref as F
import nttmul
import tmd_ref as ref
from xconv_gpu import ctx, dt, to_dev  # noqa: F401


def call(torch, tm, src, stream=0):
    from xconv_gpu import call as _call
    return _call(torch, tm, "moddown", src, stream)


def u_residues(coef_p, q, p, t, dtype):
    """[batch, L, n]: u mod q_l of the P limbs' coefficients coef_p [batch, K, n]."""
    u = ref.u_of(coef_p, p, t)
    return np.stack([u % m for m in q], axis=1).astype(dtype)


def identity_want(n, q, p, t, x):
    """The right-hand side of the identity for x [batch, L + K, n]."""
    L = len(q)
    Ctx = ctx(n)
    with Ctx(n, p) as cp, Ctx(n, q) as cq, nttmul.NttModDown(n, q, p) as md:
        coef_p = cp.inverse(np.ascontiguousarray(x[:, L:]))
        floor_hat = md.moddown(x)
        u_hat = cq.forward(u_residues(coef_p, q, p, t, x.dtype))
    mods = np.array(q, dtype=x.dtype)[None, :, None]
    return (floor_hat + (mods - u_hat)) % mods                    # all below 2^63


def check(n, q, p, t, x, got):
    """Every word of the NTT-domain output against the CPU reference (tests/full_ref.py over
    tests/tmd_ref.py and the oracle's transforms), bit for bit, at every n; and the identity
    beside it, which says which side is wrong when the two disagree."""
    F.assert_equal(got, F.reference("tmd", "moddown", x, q, p, t), (n, t))
    assert np.array_equal(got, identity_want(n, q, p, t, x))
