"""The exact base extension and the rounded ModDown under full occupancy, by the rule of
tests/scale_cases.py: every launch of a scale case (tests/xconv_cases.py scale_cases, one per new
kernel template and word class -- k_xconv_fwd of either operation at n = 4096, k_xconv_cols_fwd
and k_xconv_rows at n = 8192 -- (L, K) = (2, 1), t = 65537) holds at least 2 * 8192 waves and ends
in a partial last workgroup where the kernel takes several units per workgroup.  Inputs are made
on the device and the output is preset to a sentinel no canonical word equals.  Every word is
compared with the same context's call on pieces of the batch that start at other workgroups (a
call's result is a function of its input alone, inside the guard band as well), and the
scale_cases sample of polynomials with the device composition below on xconv_cases.sample_indices,
the sampled polynomials holding no coefficient inside the band.

The batches here exist to fill the machine, so an integer reference of every word would be minutes
of CPU: this file keeps the sampled check.  The CPU reference of every output word, at every
degree, is test_gpu_xconv.py's (tests/full_ref.py)."""
import numpy as np
import pytest

import nttmul
import scale_cases as S
import xconv_cases as C
import xconv_ref as ref
from xconv_gpu import ctx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _random_device(torch, moduli, batch, n, bits, seed):
    """Canonical words [batch, len(moduli), n] made on the device, limb l below moduli[l]."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    x = torch.empty((batch, len(moduli), n), dtype=torch.int32 if bits == 32 else torch.int64,
                    device="cuda")
    for l, m in enumerate(moduli):
        x[:, l, :] = torch.randint(0, m, (batch, n), dtype=torch.int64, device="cuda",
                                   generator=gen).to(x.dtype)
    return x


def _host(t, bits):
    return t.cpu().numpy().view(np.uint32 if bits == 32 else np.uint64)


def check_composition(op, n, q, p, t, src, got):
    """got against the reference on the sampled coefficients, through the library's transforms:
    its inverse over the input's limbs, tests/xconv_ref.py's arithmetic on
    xconv_cases.sample_indices (first, last, one per 1/64), its inverse over Q of the output."""
    idx = C.sample_indices(n)
    Ctx = ctx(n)
    with Ctx(n, tuple(p) if op == "extend" else tuple(q) + tuple(p)) as wide, Ctx(n, q) as low:
        coef = wide.inverse(src)
        back = low.inverse(got)
    fn = ref.extend_coeff if op == "extend" else ref.moddown_coeff
    assert np.array_equal(back[:, :, idx], fn(coef[:, :, idx], q, p, t))


def launches(case):
    """The launches of the case as scale_cases.Launch rows.  The forward kernels' grid is
    one-dimensional with the limb fastest: L workgroups per unit group (`bpu`), one grid row."""
    rows, upb, out = C.grid_rows(case), C.units_per_block(case), []
    inverse = C.sequence(case.op, case.n, case.bits)[:1 if case.n <= 4096 else 2]
    for key, (per, units, _) in upb.items():
        fast = key not in inverse
        out.append(S.Launch(key, per, units, 1 if fast else rows[key], 256,
                            C.bpu(key) * (rows[key] if fast else 1), units // case.batch, 0))
    return out


@pytest.mark.parametrize("case", C.scale_cases(),
                         ids=lambda c: f"{c.op}-u{c.bits}-n{c.n}x{c.batch}")
def test_full_occupancy(case, torch_cuda):
    torch = torch_cuda
    op, bits, n, batch, L, K, t = case.op, case.bits, case.n, case.batch, case.L, case.K, case.t
    ls = launches(case)
    assert [S.waves(l) for l in ls] == list(C.launch_waves(case).values())
    assert all(S.waves(l) >= S.MIN_WAVES for l in ls)
    q, p = C.moduli_of(case)
    mods = p if op == "extend" else q + p
    x = _random_device(torch, mods, batch, n, bits, n + bits + C.OPS.index(op))
    out = torch.full((batch, L, n), -1, dtype=x.dtype, device="cuda")
    want = torch.full_like(out, -2)
    step = batch // 3 + 1                       # pieces that start inside other workgroups
    with nttmul.NttExactConv(n, q, p, t) as xc:
        fn = getattr(xc, f"{op}_device")
        fn(out, x, batch)
        for p0 in range(0, batch, step):
            cnt = min(step, batch - p0)
            fn(want[p0:p0 + cnt], x[p0:p0 + cnt], cnt)
        torch.cuda.synchronize()
    bad = torch.nonzero((out != want).reshape(batch, -1).any(dim=1)).reshape(-1)
    assert bad.numel() == 0, f"{bad.numel()} polynomials differ, first {int(bad[0])}"
    polys = S.sample(ls, batch)
    assert len(polys) >= S.SAMPLE_LEAST and {0, batch - 1} <= set(polys)
    idx = torch.tensor(polys, device="cuda")
    xs, got = _host(x[idx], bits), _host(out[idx], bits)
    with ctx(n)(n, p) as cp:
        coef_p = cp.inverse(np.ascontiguousarray(xs[:, -K:]))
    sampled = C.sample_indices(n)
    assert ref.count_in_band(coef_p[:, :, sampled], p, t, xc.eps) == 0
    check_composition(op, n, q, p, t, xs, got)
