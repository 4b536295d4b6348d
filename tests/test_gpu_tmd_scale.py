"""BGV's plaintext-preserving ModDown under full occupancy, by the rule of tests/scale_cases.py:
every launch of a scale case (tests/tmd_cases.py scale_cases, one per new kernel template and word
class -- k_tmd_fwd at n = 4096, k_tmd_cols_fwd at n = 8192 -- (L, K) = (2, 1), t = 65537) holds at
least 2 * 8192 waves and ends in a partial last workgroup where the kernel takes several units per
workgroup.  Inputs are made on the device and the output is preset to a sentinel no canonical word
equals.  Every word of the whole batch is compared with the identity
out = nttmul_mdntt_moddown(x_hat) - forward(u mod q_l), formed on the device: the library's own
inverse of the P limb, u in 64-bit integer arithmetic (K = 1: y = the coefficient itself, and
(y mod t) g < 2^64), the library's forward transform and the floor form of lib/libnttmul_mdntt.so.
A sample of polynomials (tests/scale_cases.py sample) is held to the Python integers of
tests/tmd_ref.py on top.

The batches here exist to fill the machine (at least 16384 waves per launch), so an integer
reference of every output word would be minutes of CPU: this file keeps its sampled check.  The CPU
reference of every output word, at every degree, is held in test_gpu_tmd.py (tests/full_ref.py)."""
import numpy as np
import pytest

import nttmul
import scale_cases as S
import tmd_cases as C
import tmd_ref as ref
from tmd_gpu import ctx

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
    bits, n, batch, L, K, t = case.bits, case.n, case.batch, case.L, case.K, case.t
    assert K == 1 and t < 1 << 31
    ls = launches(case)
    assert [S.waves(l) for l in ls] == list(C.launch_waves(case).values())
    assert all(S.waves(l) >= S.MIN_WAVES for l in ls)
    q, p = C.moduli_of(case)
    x = _random_device(torch, q + p, batch, n, bits, n + bits)
    out = torch.full((batch, L, n), -1, dtype=x.dtype, device="cuda")
    floor = torch.full_like(out, -2)
    g = -pow(p[0], -1, t) % t
    Ctx = ctx(n)
    with nttmul.NttPlainModDown(n, q, p, t) as tm, nttmul.NttModDown(n, q, p) as md, \
            Ctx(n, p) as cp, Ctx(n, q) as cq:
        tm.moddown_device(out, x, batch)
        md.moddown_device(floor, x, batch)
        xp = x[:, L:, :].contiguous()
        y = torch.empty_like(xp)
        cp.inverse_device(y, xp, batch)                # K = 1: Ph_0 = 1, y is the coefficient
        torch.cuda.synchronize()
        v = (y.to(torch.int64) % t) * g % t            # [batch, 1, n]
        neg = v > (t - 1) // 2
        u = torch.stack([torch.where(neg, m - (t - v), v)[:, 0, :] for m in q], dim=1).to(x.dtype)
        u_hat = torch.empty_like(u)
        cq.forward_device(u_hat, u.contiguous(), batch)
        torch.cuda.synchronize()
    mods = torch.tensor(q, dtype=torch.int64, device="cuda")[None, :, None]
    want = ((floor.to(torch.int64) - u_hat.to(torch.int64)) % mods).to(x.dtype)
    bad = torch.nonzero((out != want).reshape(batch, -1).any(dim=1)).reshape(-1)
    assert bad.numel() == 0, f"{bad.numel()} polynomials differ, first {int(bad[0])}"
    assert bool(neg.any()) and bool((~neg).any())
    polys = S.sample(ls, batch)
    assert len(polys) >= S.SAMPLE_LEAST and {0, batch - 1} <= set(polys)
    idx = torch.tensor(polys, device="cuda")
    coef_p, u_dev = _host(y[idx], bits), _host(u[idx], bits)
    uu = ref.u_of(coef_p[:, :, :64], p, t)             # the first 64 coefficients in Python integers
    for l, m in enumerate(q):
        assert (u_dev[:, l, :64].astype(object) == uu % m).all()
