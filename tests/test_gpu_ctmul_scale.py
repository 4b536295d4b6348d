"""The ciphertext product under full occupancy and past 4 GiB, by the rule of
tests/scale_cases.py: the launch of a scale case (tests/ctmul_cases.py scale_cases: n = 4096,
(L, K) = (2, 1), two pairs and two terms, both kernels, both word classes) holds at least 2 * 8192
waves, with the smallest batch that meets it and, for k_ctmul_relin, which takes V entries per
workgroup, ends in a partial last workgroup (k_ctmul_high takes one part of one polynomial per
workgroup at this n).  Inputs are made on the device, the output is preset to a sentinel no
canonical word equals, every word is compared on the device with the composition of existing
calls (ksntt_mac with k = (1,), the plain contexts' pointwise products, device additions) and the
structural sample of scale_cases with tests/ctmul_ref.py.  A further test passes an up_hat just
over 4 GiB and compares with the same call in chunks below 1 GiB.

The batches here exist to fill the machine (at least 16384 waves per launch), so an integer
reference of every output word would be minutes of CPU: this file keeps its sampled check.  The CPU
reference of every output word, at every degree, is held in test_gpu_ctmul.py (tests/full_ref.py)."""
import numpy as np
import pytest

import ctmul_cases as C
import ctmul_ref as ref
import nttmul
import scale_cases as S

pytestmark = pytest.mark.gpu
GIB = 1 << 30
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
    return c


def _tensor_device(torch, plain, x, y, q, bits):
    """(e_0, e_1, d2) [batch, L, n] on the device from per-limb pointwise products and additions."""
    batch, pairs, _, L, n = x.shape
    out = [torch.empty((batch, L, n), dtype=x.dtype, device="cuda") for _ in range(3)]
    for l, (ctx, m) in enumerate(zip(plain, q)):
        x0, x1, y0, y1 = x[:, :, 0, l], x[:, :, 1, l], y[:, :, 0, l], y[:, :, 1, l]
        prods = [_product(torch, ctx, a, b, bits) for a, b in ((x0, y0), (x0, y1), (x1, y0),
                                                               (x1, y1))]
        torch.cuda.synchronize()
        sums = []
        for pr in prods:                                            # over the pairs
            acc = pr[:, 0]
            for s in range(1, pairs):
                acc = _addmod(torch, acc, pr[:, s], m)
            sums.append(acc)
        out[0][:, l], out[2][:, l] = sums[0], sums[3]
        out[1][:, l] = _addmod(torch, sums[1], sums[2], m)
    return out


def _compose_device(torch, kn, plain, up, key, x, y, q, p, bits):
    """ctmul_ref.composition with device-resident operands."""
    batch, terms, M, n = up.shape
    out = torch.full((batch, 1, 2, M, n), -2, dtype=up.dtype, device="cuda")
    kn.mac_device(out, up, key, (1,), batch, terms, 2)
    out = out[:, 0]
    e0, e1, _ = _tensor_device(torch, plain, x, y, q, bits)
    for l, (ctx, m, pq) in enumerate(zip(plain, q, ref.p_mod(q, p))):
        const = torch.full((batch, n), pq, dtype=torch.int64, device="cuda").to(up.dtype)
        for i, e in enumerate((e0, e1)):
            scaled = _product(torch, ctx, e[:, l], const, bits)
            torch.cuda.synchronize()
            out[:, i, l] = _addmod(torch, out[:, i, l], scaled, m)
    return out


def _launch(case):
    (key, (per, units, _)), = C.units_per_block(case).items()
    return S.Launch(key, per, units, C.grid_rows(case)[key], 256, C.bpu(case), 1, 0)


def _differing(torch, out, want, batch):
    return torch.nonzero((out != want).reshape(batch, -1).any(dim=1)).reshape(-1)


def _id(c):
    return f"{c.op}-u{c.bits}-n{c.n}x{c.batch}"


@pytest.mark.parametrize("case", C.scale_cases(), ids=_id)
def test_full_occupancy(case, torch_cuda):
    torch = torch_cuda
    bits, n, batch, L, K = case.bits, case.n, case.batch, case.L, case.K
    l = _launch(case)
    assert S.waves(l) == C.launch_waves(case)[l.key] >= S.MIN_WAVES and C.ends_partial(case)
    assert (l.per > 1) == (case.op == "relin")
    q, p = C.moduli_of(case)
    ext, M = q + p, L + K
    # the sample held to Python integers: the structural places of scale_cases.sample (entry 0,
    # the last entry, the partial last run, the first run past RESIDENT_WAVES in this kernel's
    # own order, where the bpu workgroups of a run of units are adjacent) and one entry from each
    # 1 / SAMPLE_PARTS of the batch; object-array arithmetic on 64-bit words pays per entry
    runs = -(-batch // l.per)
    g = -(-S.RESIDENT_WAVES // 4) // C.bpu(case) % runs
    x2 = S.second_wave_block(l)
    polys = sorted({0, batch - 1} | set(range(batch - max(1, batch % l.per), batch))
                   | set(range(g * l.per, min(batch, g * l.per + l.per)))
                   | (set(S.block_polys(l, x2)) if x2 is not None else set())
                   | {i * batch // SAMPLE_PARTS for i in range(SAMPLE_PARTS)})
    assert SAMPLE_PARTS <= len(polys) <= SAMPLE_PARTS + 3 * C.V + 2 and polys[-1] == batch - 1
    idx = torch.tensor(polys, device="cuda")
    up = _random_device(torch, ext, (batch, case.terms, n), bits, n + bits)
    key = _random_device(torch, ext, (2, case.terms, n), bits, n + bits + 1)
    x = _random_device(torch, q, (batch, case.pairs, 2, n), bits, n + bits + 2)
    y = _random_device(torch, q, (batch, case.pairs, 2, n), bits, n + bits + 3)
    plain = [nttmul.Context(n, m) for m in q]
    try:
        with nttmul.NttCtMul(n, q, p) as ct:
            if case.op == "high":
                out = torch.full((batch, L, n), -1, dtype=x.dtype, device="cuda")
                ct.high_device(out, x, y, batch, case.pairs)
            else:
                out = torch.full((batch, 2, M, n), -1, dtype=x.dtype, device="cuda")
                ct.relin_device(out, up, key, x, y, batch, case.pairs, case.terms)
            torch.cuda.synchronize()
        if case.op == "high":
            want = _tensor_device(torch, plain, x, y, q, bits)[2]
        else:
            with nttmul.NttKeySwitch(n, q, p, 1) as kn:
                want = _compose_device(torch, kn, plain, up, key, x, y, q, p, bits)
        torch.cuda.synchronize()
    finally:
        for c in plain:
            c.close()
    bad = _differing(torch, out, want, batch)
    assert bad.numel() == 0, f"{bad.numel()} entries differ, first {int(bad[0])}"
    got = _host(out[idx], bits)
    xs, ys = _host(x[idx], bits), _host(y[idx], bits)
    if case.op == "high":
        want_s = ref.high(xs, ys, q)
    else:
        want_s = ref.relin(_host(up[idx], bits), _host(key, bits), xs, ys, q, p)
    assert S.mismatching(got, want_s, polys) == []


def test_up_hat_past_4_gib_equals_the_call_in_chunks(torch_cuda):
    """Every offset is 64-bit: an up_hat just over 4 GiB, against the same context's call on
    chunks whose every operand stays below 1 GiB."""
    torch = torch_cuda
    case = C.large_case()
    bits, n, batch, L, K = case.bits, case.n, case.batch, case.L, case.K
    q, p = C.moduli_of(case)
    ext, M = q + p, L + K
    per = case.terms * M * n * (bits // 8)
    assert batch * per > 4 * GIB >= (batch - 1) * per
    step = (GIB - 1) // per
    assert step >= 1 and step * per < GIB
    up = _random_device(torch, ext, (batch, case.terms, n), bits, n + bits + 1)
    key = _random_device(torch, ext, (2, case.terms, n), bits, n + bits + 2)
    x = _random_device(torch, q, (batch, case.pairs, 2, n), bits, n + bits + 3)
    y = _random_device(torch, q, (batch, case.pairs, 2, n), bits, n + bits + 4)
    assert up.numel() * up.element_size() > 4 * GIB
    out = torch.full((batch, 2, M, n), -1, dtype=up.dtype, device="cuda")
    want = torch.full_like(out, -2)
    with nttmul.NttCtMul(n, q, p) as ct:
        ct.relin_device(out, up, key, x, y, batch, case.pairs, case.terms)
        for p0 in range(0, batch, step):
            cnt = min(step, batch - p0)
            ct.relin_device(want[p0:p0 + cnt], up[p0:p0 + cnt], key, x[p0:p0 + cnt],
                            y[p0:p0 + cnt], cnt, case.pairs, case.terms)
        torch.cuda.synchronize()
    bad = _differing(torch, out, want, batch)
    assert bad.numel() == 0, f"{bad.numel()} entries differ, first {int(bad[0])}"
    # the ends against the Python-integer reference
    ends = [0, batch - 1]
    idx = torch.tensor(ends, device="cuda")
    expect = ref.relin(_host(up[idx], bits), _host(key, bits), _host(x[idx], bits),
                       _host(y[idx], bits), q, p)
    assert S.mismatching(_host(out[idx], bits), expect, ends) == []
