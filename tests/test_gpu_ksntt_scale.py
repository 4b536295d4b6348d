"""ModUp and the key mac on NTT-domain limbs under full occupancy and past 4 GiB, by the rule of
tests/scale_cases.py: every launch of a scale case (tests/ksntt_cases.py scale_cases: modup at
n = 4096 and n = 8192 with (L, K, alpha) = (2, 1, 1), mac at n = 4096, both word classes) holds at
least 2 * 8192 waves, with the smallest batch that meets it and a partial last workgroup where
one can exist.  Inputs are made on the device, the output is preset to a sentinel no canonical
word equals, every word is compared on the device with the composition (inverse, ks_modup,
forward; hoist_ntt, forward) and the scale_cases sample with tests/ksntt_ref.py.  Two further
tests pass an output just over 4 GiB and compare with the same call in chunks below 1 GiB.

The batches here exist to fill the machine (at least 16384 waves per launch), so an integer
reference of every output word would be minutes of CPU: this file keeps its sampled check.  The CPU
reference of every output word, at every degree, is held in test_gpu_ksntt.py (tests/full_ref.py)."""
import numpy as np
import pytest

import ksntt_cases as C
import ksntt_ref as ref
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


def _ctx(n):
    return nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext


def launches(case):
    """The launches of the case as scale_cases.Launch rows.  The forward kernels' grid is
    one-dimensional with the target fastest and the mac's has the rotation fastest: that many
    workgroups per unit group (`bpu`)."""
    rows, upb, out = C.grid_rows(case), C.units_per_block(case), []
    if isinstance(case, C.Mac):
        (key, (per, units, _)), = upb.items()
        return [S.Launch(key, per, units, case.L + case.K, 256, len(case.ks), units // case.batch, 0)]
    inverse = C.sequence("modup", case.n, case.bits)[:1 if case.n <= 4096 else 2]
    for key, (per, units, _) in upb.items():
        fast = key not in inverse
        out.append(S.Launch(key, per, units, 1 if fast else rows[key], 256,
                            C.bpu(key) * (rows[key] if fast else 1), units // case.batch, 0))
    return out


def _differing(torch, out, want, batch):
    return torch.nonzero((out != want).reshape(batch, -1).any(dim=1)).reshape(-1)


def _id(c):
    return f"{C.op_of(c)}-u{c.bits}-n{c.n}x{c.batch}"


@pytest.mark.parametrize("case", C.scale_cases(), ids=_id)
def test_full_occupancy(case, torch_cuda):
    torch = torch_cuda
    bits, n, batch, L, K = case.bits, case.n, case.batch, case.L, case.K
    ls = launches(case)
    assert [S.waves(l) for l in ls] == list(C.launch_waves(case).values())
    assert all(S.waves(l) >= S.MIN_WAVES for l in ls)
    q, p = C.moduli_of(case)
    ext, M = q + p, L + K
    polys = S.sample(ls, batch)
    assert len(polys) >= S.SAMPLE_LEAST and {0, batch - 1} <= set(polys)
    idx = torch.tensor(polys, device="cuda")
    Ctx = _ctx(n)
    if isinstance(case, C.Up):
        dn = C.dnum(case)
        x = _random_device(torch, q, (batch, n), bits, n + bits)
        out = torch.full((batch, dn, M, n), -1, dtype=x.dtype, device="cuda")
        with nttmul.NttKeySwitch(n, q, p, case.alpha) as kn:
            kn.modup_device(out, x, batch)
            torch.cuda.synchronize()
        coef, up = torch.empty_like(x), torch.empty_like(out)
        want = torch.full_like(out, -2)
        with Ctx(n, ext) as big, Ctx(n, q) as low, \
                nttmul.KeySwitchBasis(n, q, p, case.alpha) as ks:
            low.inverse_device(coef, x, batch)
            ks.modup_device(up, coef, batch)
            big.forward_device(want, up, batch * dn)
            torch.cuda.synchronize()
        bad = _differing(torch, out, want, batch)
        assert bad.numel() == 0, f"{bad.numel()} polynomials differ, first {int(bad[0])}"
        got = _host(out[idx], bits)
        want_s = ref.modup_composition(_host(x[idx], bits), q, p, case.alpha)
        assert S.mismatching(got, want_s, polys) == []
        return
    rots = len(case.ks)
    a = _random_device(torch, ext, (batch, case.terms, n), bits, n + bits)
    b = _random_device(torch, ext, (rots, case.comps, case.terms, n), bits, n + bits + 1)
    out = torch.full((batch, rots, case.comps, M, n), -1, dtype=a.dtype, device="cuda")
    with nttmul.NttKeySwitch(n, q, p, 1) as kn:
        kn.mac_device(out, a, b, case.ks, batch, case.terms, case.comps)
        torch.cuda.synchronize()
    c, want = torch.empty_like(out), torch.full_like(out, -2)
    with Ctx(n, ext) as big:
        big.hoist_ntt_device(c, a, b, case.ks, batch, case.terms, case.comps)
        big.forward_device(want, c, batch * rots * case.comps)
        torch.cuda.synchronize()
    bad = _differing(torch, out, want, batch)
    assert bad.numel() == 0, f"{bad.numel()} polynomials differ, first {int(bad[0])}"
    got = _host(out[idx], bits)
    assert S.mismatching(got, ref.mac(_host(a[idx], bits), _host(b, bits), case.ks, ext),
                         polys) == []


@pytest.mark.parametrize("case", C.large_cases(), ids=_id)
def test_output_past_4_gib_equals_the_call_in_chunks(case, torch_cuda):
    """Every offset is 64-bit: an output just over 4 GiB, against the same context's call on
    chunks whose every operand stays below 1 GiB."""
    torch = torch_cuda
    bits, n, batch, L, K = case.bits, case.n, case.batch, case.L, case.K
    q, p = C.moduli_of(case)
    ext, M = q + p, L + K
    poly_out = C.out_polys(case) * n * (bits // 8)
    assert batch * poly_out > 4 * GIB >= (batch - 1) * poly_out
    step = (GIB - 1) // poly_out
    assert step >= 1 and step * poly_out < GIB
    ends = [0, batch - 1]
    idx = torch.tensor(ends, device="cuda")
    if isinstance(case, C.Up):
        x = _random_device(torch, q, (batch, n), bits, n + bits + 1)
        out = torch.full((batch, C.dnum(case), M, n), -1, dtype=x.dtype, device="cuda")
        want = torch.full_like(out, -2)
        with nttmul.NttKeySwitch(n, q, p, case.alpha) as kn:
            kn.modup_device(out, x, batch)
            for p0 in range(0, batch, step):
                cnt = min(step, batch - p0)
                kn.modup_device(want[p0:p0 + cnt], x[p0:p0 + cnt], cnt)
            torch.cuda.synchronize()
        expect = ref.modup_composition(_host(x[idx], bits), q, p, case.alpha)
    else:
        rots = len(case.ks)
        a = _random_device(torch, ext, (batch, case.terms, n), bits, n + bits + 1)
        b = _random_device(torch, ext, (rots, case.comps, case.terms, n), bits, n + bits + 2)
        out = torch.full((batch, rots, case.comps, M, n), -1, dtype=a.dtype, device="cuda")
        want = torch.full_like(out, -2)
        with nttmul.NttKeySwitch(n, q, p, 1) as kn:
            kn.mac_device(out, a, b, case.ks, batch, case.terms, case.comps)
            for p0 in range(0, batch, step):
                cnt = min(step, batch - p0)
                kn.mac_device(want[p0:p0 + cnt], a[p0:p0 + cnt], b, case.ks, cnt, case.terms,
                              case.comps)
            torch.cuda.synchronize()
        expect = ref.mac(_host(a[idx], bits), _host(b, bits), case.ks, ext)
    bad = _differing(torch, out, want, batch)
    assert bad.numel() == 0, f"{bad.numel()} polynomials differ, first {int(bad[0])}"
    # the ends against the Python-integer reference
    assert S.mismatching(_host(out[idx], bits), expect, ends) == []
