"""Standalone transforms through run_device's sub-batch loop (csrc/nttmul.cpp): contexts with
scratch_mb = 1, so a small batch already runs in several sub-batches with a ragged last one --
the bit-reversal into the scratch's perm buffer, the transform, the in-place bit-reversal of the
output, and for n > 4096 the column / row passes through the 1 MiB scratch buffers.  Every row
is compared with the oracle transform of that row."""
import numpy as np
import pytest

import dispatch_cases as D
import nttmul
from oracle import oracle as O
from test_gpu_parity import _as_np, _check_whole_batch, _xf_expected, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


def _filled(torch, ctx, n, q, bits, batch, p0=0):
    """Counter-based device inputs with the edge rows where sub-batches begin and end: row 0 all
    q - 1, the last row (the ragged sub-batch) a unit impulse at n - 1."""
    dt = torch.int32 if bits == 32 else torch.int64
    a = torch.empty(batch * n, dtype=dt, device="cuda")
    b = torch.empty_like(a)
    ctx.fill_random_device(a, b, p0, batch, bits, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bits == 64 or q < (1 << 31)             # (q - 1 fits the signed torch word)
    a[:n] = q - 1
    a[(batch - 1) * n:] = 0
    a[batch * n - 1] = 1
    return a, b


def _check_rows(P, n, q, bits, batch, mode, x, got):
    hx = _as_np(x, bits).reshape(batch, n).astype(np.uint64)
    hg = _as_np(got, bits).reshape(batch, n).astype(np.uint64)
    bad = [i for i in range(batch)
           if not np.array_equal(hg[i], _xf_expected(P, hx[i], mode, False, n, q))]
    assert not bad, (n, q, bits, mode, bad[:8])


@pytest.mark.parametrize("n,q,bits,batch,modes", D.SUBBATCH)
def test_transforms_in_sub_batches(n, q, bits, batch, modes, torch_cuda):
    """(4096, u32, 129): 64 + 64 + 1 through the perm buffer only (the reordered modes);
    (8192, u32, 65) and (8192, u64, 65): 32 + 32 + 1, the u64 case with scratch in 4-byte and perm
    in 8-byte words; (65536, Q62, 5): 2 + 2 + 1 through the square split's single-polynomial
    forward column pass.  The sub-batch sizes follow from scratch_mb = 1 and are asserted here."""
    torch = torch_cuda
    w_poly, io_poly = n * D.native_bits(q) // 8, n * bits // 8
    chunk = (1 << 20) // (w_poly if n > 4096 else io_poly)
    assert 1 < chunk < batch and batch % chunk == 1
    P = O.Plan(n, q)
    ctx = nttmul.Context(n, q, scratch_mb=1)
    x, _ = _filled(torch, ctx, n, q, bits, batch)
    out = torch.empty_like(x)
    s = torch.cuda.current_stream().cuda_stream
    for mode in modes:
        out.fill_(-1)
        ctx.transform_device(out, x, mode, batch, bits, stream=s)
        torch.cuda.synchronize()
        _check_rows(P, n, q, bits, batch, mode, x, out)


def test_product_in_sub_batches_u64_words(torch_cuda):
    """multiply_device in 32 + 32 + 1 sub-batches on u64 words of a 32-bit modulus: the operand
    and result strides are 8-byte words, the scratch 4-byte words."""
    torch = torch_cuda
    n, q, bits, batch = D.SUBBATCH_PRODUCT
    ctx = nttmul.Context(n, q, scratch_mb=1)
    a = torch.empty(batch * n, dtype=torch.int64, device="cuda")
    b, c = torch.empty_like(a), torch.empty_like(a)
    s = torch.cuda.current_stream().cuda_stream
    ctx.fill_random_device(a, b, 0, batch, bits, stream=s)
    ctx.multiply_device(c, a, b, batch, bits, stream=s)
    torch.cuda.synchronize()
    assert _check_whole_batch(n, q, bits, 0, batch, a, b, c) == batch


def test_sub_batched_transforms_on_two_streams(torch_cuda):
    """Two sub-batched transforms enqueued back to back on two different streams share the
    context's scratch and perm buffers (event-ordered, nttmul.cpp Scratch): a reordered forward
    on one stream, an inverse on the other, three rounds, u64 words on a 32-bit modulus."""
    torch = torch_cuda
    n, q, bits, batch = D.SUBBATCH_PRODUCT
    P = O.Plan(n, q)
    ctx = nttmul.Context(n, q, scratch_mb=1)
    x1, x2 = _filled(torch, ctx, n, q, bits, batch, p0=batch)
    o1, o2 = torch.empty_like(x1), torch.empty_like(x2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        ctx.transform_device(o1, x1, nttmul.XF_REV2STD, batch, bits, stream=s1.cuda_stream)
        ctx.transform_device(o2, x2, nttmul.XF_INVERSE | nttmul.XF_REV2STD, batch, bits,
                             stream=s2.cuda_stream)
    torch.cuda.synchronize()
    _check_rows(P, n, q, bits, batch, nttmul.XF_REV2STD, x1, o1)
    _check_rows(P, n, q, bits, batch, nttmul.XF_INVERSE | nttmul.XF_REV2STD, x2, o2)
