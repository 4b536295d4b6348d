"""combine and tensor under full occupancy, by the rule of tests/scale_cases.py: the launch of a
scale case (tests/ctlin_cases.py scale_cases: n = 256, L = 3, one row per kernel: combine at comps
1, 2 and 3 with a plaintext product, a plain term, a scalar and both constants, tensor with two
pairs, both word classes) holds at least 2 * 8192 waves, with the smallest batch that meets it and
ends in a partial last workgroup (at n = 256 a workgroup takes 4 batch entries on 32-bit words and
2 on 64-bit words).  Inputs are made on the device, the output is preset to a sentinel no
canonical word equals, every word is compared on the device with the per-limb composition (the
plain contexts' pointwise products, device additions) and the structural sample of scale_cases
with tests/ctlin_ref.py in Python integers.

The batches here exist to fill the machine (at least 16384 waves per launch), so an integer
reference of every output word would be minutes of CPU: this file keeps its sampled check.  The CPU
reference of every output word, at every degree, is held in test_gpu_ctlin.py (tests/full_ref.py)."""
import numpy as np
import pytest

import ctlin_cases as C
import ctlin_ref as ref
import nttmul
import scale_cases as S

pytestmark = pytest.mark.gpu
SAMPLE_PARTS = 24


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _tdt(torch, bits):
    return torch.int32 if bits == 32 else torch.int64


def _random_device(torch, moduli, shape, bits, seed):
    """Canonical words [*shape, len(moduli), n] made on the device, limb l below moduli[l]."""
    *lead, n = shape
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    x = torch.empty((*lead, len(moduli), n), dtype=_tdt(torch, bits), device="cuda")
    for l, m in enumerate(moduli):
        x[..., l, :] = torch.randint(0, m, (*lead, n), dtype=torch.int64, device="cuda",
                                     generator=gen).to(x.dtype)
    return x


def _host(t, bits):
    return t.cpu().numpy().view(np.uint32 if bits == 32 else np.uint64)


def _addmod(torch, x, y, m):
    """x + y mod m on the device for canonical words (m < 2^62: the sum fits int64)."""
    s = x.to(torch.int64) + y.to(torch.int64)
    return torch.where(s >= m, s - m, s).to(x.dtype)


def _product(torch, ctx, a, b, bits):
    """a o b mod the plain context's modulus, [.., n] device tensors (made contiguous)."""
    a, b = a.contiguous(), b.contiguous()
    c = torch.empty_like(a)
    ctx.pointwise_device(c, a, b, a.numel() // ctx.n, bits)
    torch.cuda.synchronize()
    return c


def _combine_device(torch, plain, case, xs, ws, q):
    """The composition on the device: per limb the pointwise products, then additions."""
    out = torch.empty_like(xs[0])
    for l, (ctx, m) in enumerate(zip(plain, q)):
        acc = torch.zeros_like(xs[0][:, :, l])
        for (kind, i), w in zip(case.terms, ws):
            if kind == C.SCALAR:
                wl = w[l].expand(case.n)
            elif kind == C.PLAIN:
                wl = w[l]
            if i is None:
                t = torch.zeros_like(acc)
                t[:, 0] = wl
            elif kind == C.ONE:
                t = xs[i][:, :, l]
            else:
                t = _product(torch, ctx, xs[i][:, :, l], wl.expand_as(acc), case.bits)
            acc = _addmod(torch, acc, t, m)
        out[:, :, l] = acc
    return out


def _tensor_device(torch, plain, x, y, q, bits):
    """[batch, 3, L, n] on the device from per-limb pointwise products and additions."""
    batch, pairs, _, L, n = x.shape
    out = torch.empty((batch, 3, L, n), dtype=x.dtype, device="cuda")
    for l, (ctx, m) in enumerate(zip(plain, q)):
        x0, x1, y0, y1 = x[:, :, 0, l], x[:, :, 1, l], y[:, :, 0, l], y[:, :, 1, l]
        sums = []
        for a, b in ((x0, y0), (x0, y1), (x1, y0), (x1, y1)):
            pr = _product(torch, ctx, a, b, bits)
            acc = pr[:, 0]
            for s in range(1, pairs):
                acc = _addmod(torch, acc, pr[:, s], m)
            sums.append(acc)
        out[:, 0, l], out[:, 2, l] = sums[0], sums[3]
        out[:, 1, l] = _addmod(torch, sums[1], sums[2], m)
    return out


def _launch(case):
    (key, (per, units, _)), = C.units_per_block(case).items()
    return S.Launch(key, per, units, C.grid_rows(case)[key], 256, C.bpu(case), 1, 0)


def _id(c):
    return f"{c.op}-u{c.bits}-c{c.comps}-n{c.n}x{c.batch}"


@pytest.mark.parametrize("case", C.scale_cases(), ids=_id)
def test_full_occupancy(case, torch_cuda):
    torch = torch_cuda
    bits, n, batch = case.bits, case.n, case.batch
    l = _launch(case)
    assert S.waves(l) == C.launch_waves(case)[l.key] >= S.MIN_WAVES and C.ends_partial(case)
    assert l.per > 1 and l.key == C.kernel_name(case)
    q = C.moduli_of(case)
    # the sample held to Python integers: entry 0, the last entry, the partial last workgroup, the
    # first workgroup past RESIDENT_WAVES waves, and one entry from each 1 / SAMPLE_PARTS of the
    # batch; object-array arithmetic on 64-bit words pays per entry
    x2 = S.second_wave_block(l)
    polys = sorted({0, batch - 1} | set(range(batch - batch % l.per, batch))
                   | (set(S.block_polys(l, x2)) if x2 is not None else set())
                   | {i * batch // SAMPLE_PARTS for i in range(SAMPLE_PARTS)})
    assert SAMPLE_PARTS <= len(polys) <= SAMPLE_PARTS + 2 * l.per + 2 and polys[-1] == batch - 1
    idx = torch.tensor(polys, device="cuda")
    plain = [nttmul.Context(n, m) for m in q]
    try:
        with nttmul.NttCtLin(n, q) as cl:
            if case.op == "tensor":
                x = _random_device(torch, q, (batch, case.pairs, 2, n), bits, n + bits + 2)
                y = _random_device(torch, q, (batch, case.pairs, 2, n), bits, n + bits + 3)
                out = torch.full((batch, 3, C.L, n), -1, dtype=x.dtype, device="cuda")
                cl.tensor_device(out, x, y, batch, case.pairs)
                torch.cuda.synchronize()
                want = _tensor_device(torch, plain, x, y, q, bits)
                want_s = ref.tensor(_host(x[idx], bits), _host(y[idx], bits), q)
            else:
                xs = [_random_device(torch, q, (batch, case.comps, n), bits, n + bits + i)
                      for i in range(C.x_count(case))]
                ws = [None if kind == C.ONE else
                      _random_device(torch, q, (1,) if kind == C.SCALAR else (n,), bits,
                                     n + bits + 10 + t)
                      for t, (kind, _) in enumerate(case.terms)]
                ws = [w if w is None or w.shape[-1] == n else w[:, 0].contiguous() for w in ws]
                out = torch.full((batch, case.comps, C.L, n), -1, dtype=xs[0].dtype, device="cuda")
                terms = [(None if i is None else xs[i], w, C.KIND_CODE[kind])
                         for (kind, i), w in zip(case.terms, ws)]
                cl.combine_device(out, terms, batch, case.comps)
                torch.cuda.synchronize()
                want = _combine_device(torch, plain, case, xs, ws, q)
                hterms = [(None if i is None else _host(xs[i][idx], bits),
                           None if w is None else _host(w, bits), C.KIND_CODE[kind])
                          for (kind, i), w in zip(case.terms, ws)]
                want_s = ref.combine(hterms, q, (len(polys), case.comps, C.L, n),
                                     np.uint32 if bits == 32 else np.uint64)
        torch.cuda.synchronize()
    finally:
        for c in plain:
            c.close()
    bad = torch.nonzero((out != want).reshape(batch, -1).any(dim=1)).reshape(-1)
    assert bad.numel() == 0, f"{bad.numel()} entries differ, first {int(bad[0])}"
    assert S.mismatching(_host(out[idx], bits), want_s, polys) == []
