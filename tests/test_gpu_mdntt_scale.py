"""ModDown on NTT-domain limbs under full occupancy and past 4 GiB, by the rule of
tests/scale_cases.py: every launch of a scale case (tests/mdntt_cases.py scale_cases, one per new
kernel template and word class, n = 4096 and n = 8192, (L, K) = (2, 1)) holds at least 2 * 8192
waves and ends in a partial last workgroup where the kernel takes several units per workgroup.
Inputs are made on the device, the output is preset to a sentinel no canonical word equals, every
word is compared with the device composition (inverse over Q u P, KeySwitchBasis.moddown, forward
over Q) and the scale_cases sample with tests/mdntt_ref.py.  Two further tests pass an x_hat just
over 4 GiB and compare with the same call in chunks below 1 GiB.

The batches here exist to fill the machine (at least 16384 waves per launch), so an integer
reference of every output word would be minutes of CPU: this file keeps its sampled check.  The CPU
reference of every output word, at every degree, is held in test_gpu_mdntt.py (tests/full_ref.py)."""
import numpy as np
import pytest

import mdntt_cases as C
import mdntt_ref as ref
import nttmul
import scale_cases as S

pytestmark = pytest.mark.gpu
GIB = 1 << 30


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _tdt(torch, bits):
    return torch.int32 if bits == 32 else torch.int64


def _random_device(torch, moduli, batch, n, bits, seed):
    """Canonical words [batch, len(moduli), n] made on the device, limb l below moduli[l]."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    x = torch.empty((batch, len(moduli), n), dtype=_tdt(torch, bits), device="cuda")
    for l, m in enumerate(moduli):
        x[:, l, :] = torch.randint(0, m, (batch, n), dtype=torch.int64, device="cuda",
                                   generator=gen).to(x.dtype)
    return x


def _host(t, bits):
    return t.cpu().numpy().view(np.uint32 if bits == 32 else np.uint64)


def launches(case):
    """The launches of the case as scale_cases.Launch rows.  The forward kernels' grid is
    one-dimensional with the limb fastest: L workgroups per unit group (`bpu`), one grid row."""
    rows, upb, out = C.grid_rows(case), C.units_per_block(case), []
    inverse = C.sequence(case.n, case.bits)[:1 if case.n <= 4096 else 2]
    for key, (per, units, _) in upb.items():
        fast = key not in inverse
        out.append(S.Launch(key, per, units, 1 if fast else rows[key], 256,
                            C.bpu(key) * (rows[key] if fast else 1), units // case.batch, 0))
    return out


@pytest.mark.parametrize("case", C.scale_cases(), ids=lambda c: f"u{c.bits}-n{c.n}x{c.batch}")
def test_full_occupancy(case, torch_cuda):
    torch = torch_cuda
    bits, n, batch, L, K = case.bits, case.n, case.batch, case.L, case.K
    ls = launches(case)
    assert [S.waves(l) for l in ls] == list(C.launch_waves(case).values())
    assert all(S.waves(l) >= S.MIN_WAVES for l in ls)
    q, p = C.moduli_of(case)
    Ctx = nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext
    x = _random_device(torch, q + p, batch, n, bits, n + bits)
    out = torch.full((batch, L, n), -1, dtype=x.dtype, device="cuda")
    with nttmul.NttModDown(n, q, p) as md:
        md.moddown_device(out, x, batch)
        torch.cuda.synchronize()
    coef = torch.empty_like(x)
    down, want = torch.empty_like(out), torch.full_like(out, -2)
    with Ctx(n, q + p) as ext, Ctx(n, q) as low, nttmul.KeySwitchBasis(n, q, p, 1) as ks:
        ext.inverse_device(coef, x, batch)
        ks.moddown_device(down, coef, batch)
        low.forward_device(want, down, batch)
        torch.cuda.synchronize()
    bad = torch.nonzero((out != want).reshape(batch, -1).any(dim=1)).reshape(-1)
    assert bad.numel() == 0, f"{bad.numel()} polynomials differ, first {int(bad[0])}"
    polys = S.sample(ls, batch)
    assert len(polys) >= S.SAMPLE_LEAST and {0, batch - 1} <= set(polys)
    idx = torch.tensor(polys, device="cuda")
    got = _host(out[idx], bits)
    assert S.mismatching(got, ref.moddown(_host(x[idx], bits), q, p), polys) == []


@pytest.mark.parametrize("bits,n,L,K", C.LARGE, ids=lambda v: str(v))
def test_x_hat_past_4_gib_equals_the_call_in_chunks(bits, n, L, K, torch_cuda):
    """Every offset is 64-bit: an x_hat just over 4 GiB (several sub-batches of the default
    scratch), against the same context's call on chunks whose every operand stays below 1 GiB."""
    torch = torch_cuda
    batch = C.large_batch(bits, n, L, K)
    wb = bits // 8
    poly_in = (L + K) * n * wb
    assert batch * poly_in > 4 * GIB >= (batch - 1) * poly_in
    assert len(C.chunks(C.Case(bits, n, batch, L, K))) > 1
    q, p = C.moduli_of(C.Case(bits, n, batch, L, K))
    x = _random_device(torch, q + p, batch, n, bits, n + bits + 1)
    out = torch.full((batch, L, n), -1, dtype=x.dtype, device="cuda")
    want = torch.full_like(out, -2)
    step = (GIB - 1) // poly_in
    assert step >= 1 and step * poly_in < GIB
    with nttmul.NttModDown(n, q, p) as md:
        md.moddown_device(out, x, batch)
        for p0 in range(0, batch, step):
            cnt = min(step, batch - p0)
            md.moddown_device(want[p0:p0 + cnt], x[p0:p0 + cnt], cnt)
        torch.cuda.synchronize()
    bad = torch.nonzero((out != want).reshape(batch, -1).any(dim=1)).reshape(-1)
    assert bad.numel() == 0, f"{bad.numel()} polynomials differ, first {int(bad[0])}"
    # the ends against the Python-integer reference
    ends = [0, batch - 1]
    idx = torch.tensor(ends, device="cuda")
    assert S.mismatching(_host(out[idx], bits), ref.moddown(_host(x[idx], bits), q, p), ends) == []
