"""The weighted sum of rotations under full occupancy and past 4 GiB, by the rule of
tests/scale_cases.py: the launch of a scale case (tests/lintrans_cases.py scale_cases: n = 4096,
(L, K) = (2, 1), two rotations of two terms and two components, weights and c_0 on, both word
classes) holds at least 2 * 8192 waves, with the smallest batch that meets it and ends in a partial
last workgroup.  Inputs are made on the device, the output is preset to a sentinel no canonical
word equals, every word is compared on the device with the composition of ksntt_mac calls and the
scale_cases sample with tests/lintrans_ref.py.  A further test passes an a_hat just over 4 GiB and
compares with the same call in chunks below 1 GiB.

The batches here exist to fill the machine (at least 16384 waves per launch), so an integer
reference of every output word would be minutes of CPU: this file keeps its sampled check.  The CPU
reference of every output word, at every degree, is held in test_gpu_lintrans.py (tests/full_ref.py)."""
import numpy as np
import pytest

import lintrans_cases as C
import lintrans_ref as ref
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


def _mulmod_const(torch, x, c, m, bits):
    """x c mod m on the device for canonical x and a constant c < m (64-bit words: on the host in
    Python integers; w_hat is rots polynomials)."""
    if bits == 32:
        return (x.to(torch.int64) * c % m).to(x.dtype)
    h = _host(x, bits).astype(object) * c % m
    return torch.from_numpy(h.astype(np.uint64).view(np.int64)).cuda()


def _addmod(torch, x, y, m, bits):
    """x + y mod m on the device for canonical words (m < 2^62: the sum fits int64)."""
    s = x.to(torch.int64) + y.to(torch.int64)
    return torch.where(s >= m, s - m, s).to(x.dtype)


def _compose_device(torch, kn, a, b, w, c0, ks, q, p, bits):
    """lintrans_ref.composition with device-resident operands: ksntt_mac four times, the
    permutation and the last addition on the device."""
    ext, L = q + p, len(q)
    batch, terms, M, n = a.shape
    rots, comps = b.shape[:2]
    m = torch.empty((batch, rots, comps, M, n), dtype=a.dtype, device="cuda")
    kn.mac_device(m, a, b, ks, batch, terms, comps)
    m2 = m.permute(0, 2, 1, 3, 4).contiguous()
    out = torch.full((batch, comps, M, n), -2, dtype=a.dtype, device="cuda")
    kn.mac_device(out, m2, w, (1,), batch * comps, rots, 1)
    pad = torch.zeros((batch, 1, M, n), dtype=a.dtype, device="cuda")
    pad[:, 0, :L] = c0
    wp = torch.zeros_like(w)
    for l, (mod, pq) in enumerate(zip(q, ref.p_mod(q, p))):
        wp[:, l] = _mulmod_const(torch, w[:, l], pq, mod, bits)
    z = torch.empty((batch, rots, 1, M, n), dtype=a.dtype, device="cuda")
    kn.mac_device(z, pad, wp, ks, batch, 1, 1)
    zs = torch.empty((batch, M, n), dtype=a.dtype, device="cuda")
    ones = torch.ones((rots, M, n), dtype=a.dtype, device="cuda")
    kn.mac_device(zs, z, ones, (1,), batch, rots, 1)
    torch.cuda.synchronize()
    for l, mod in enumerate(ext):
        out[:, 0, l] = _addmod(torch, out[:, 0, l], zs[:, l], mod, bits)
    return out


def _launch(case):
    (key, (per, units, _)), = C.units_per_block(case).items()
    return S.Launch(key, per, units, case.L + case.K, 256, C.bpu(case), 1, 0)


def _differing(torch, out, want, batch):
    return torch.nonzero((out != want).reshape(batch, -1).any(dim=1)).reshape(-1)


def _id(c):
    return f"u{c.bits}-n{c.n}x{c.batch}"


@pytest.mark.parametrize("case", C.scale_cases(), ids=_id)
def test_full_occupancy(case, torch_cuda):
    torch = torch_cuda
    bits, n, batch, L, K = case.bits, case.n, case.batch, case.L, case.K
    l = _launch(case)
    assert S.waves(l) == C.launch_waves(case)[l.key] >= S.MIN_WAVES and batch % C.V
    q, p = C.moduli_of(case)
    ext, M, rots = q + p, L + K, len(case.ks)
    # the sample of scale_cases: its Launch has this kernel's own order (the n / 256 workgroups
    # of a run of V entries are adjacent); the partial last run and the first run past
    # RESIDENT_WAVES spelled out as well
    g = -(-S.RESIDENT_WAVES // 4) // C.bpu(case) % C.grid(batch, n)["groups"]
    polys = sorted(set(S.sample([l], batch)) | set(range(batch - batch % C.V, batch))
                   | set(range(g * C.V, min(batch, g * C.V + C.V))))
    assert len(polys) >= S.SAMPLE_LEAST and {0, batch - 1} <= set(polys)
    idx = torch.tensor(polys, device="cuda")
    a = _random_device(torch, ext, (batch, case.terms, n), bits, n + bits)
    b = _random_device(torch, ext, (rots, case.comps, case.terms, n), bits, n + bits + 1)
    w = _random_device(torch, ext, (rots, n), bits, n + bits + 2)
    c0 = _random_device(torch, q, (batch, n), bits, n + bits + 3)
    out = torch.full((batch, case.comps, M, n), -1, dtype=a.dtype, device="cuda")
    with nttmul.NttLinTrans(n, q, p) as lt:
        lt.apply_device(out, a, b, case.ks, batch, case.terms, case.comps, w_hat=w, c0_hat=c0)
        torch.cuda.synchronize()
    with nttmul.NttKeySwitch(n, q, p, 1) as kn:
        want = _compose_device(torch, kn, a, b, w, c0, case.ks, q, p, bits)
    bad = _differing(torch, out, want, batch)
    assert bad.numel() == 0, f"{bad.numel()} entries differ, first {int(bad[0])}"
    got = _host(out[idx], bits)
    want_s = ref.apply(_host(a[idx], bits), _host(b, bits), case.ks, q, p, _host(w, bits),
                       _host(c0[idx], bits))
    assert S.mismatching(got, want_s, polys) == []


def test_a_hat_past_4_gib_equals_the_call_in_chunks(torch_cuda):
    """Every offset is 64-bit: an a_hat just over 4 GiB, against the same context's call on chunks
    whose every operand stays below 1 GiB."""
    torch = torch_cuda
    case = C.large_case()
    bits, n, batch, L, K = case.bits, case.n, case.batch, case.L, case.K
    q, p = C.moduli_of(case)
    ext, M, rots = q + p, L + K, len(case.ks)
    per = case.terms * M * n * (bits // 8)
    assert batch * per > 4 * GIB >= (batch - 1) * per
    step = (GIB - 1) // per
    assert step >= 1 and step * per < GIB
    a = _random_device(torch, ext, (batch, case.terms, n), bits, n + bits + 1)
    b = _random_device(torch, ext, (rots, case.comps, case.terms, n), bits, n + bits + 2)
    w = _random_device(torch, ext, (rots, n), bits, n + bits + 3)
    c0 = _random_device(torch, q, (batch, n), bits, n + bits + 4)
    assert a.numel() * a.element_size() > 4 * GIB
    out = torch.full((batch, case.comps, M, n), -1, dtype=a.dtype, device="cuda")
    want = torch.full_like(out, -2)
    with nttmul.NttLinTrans(n, q, p) as lt:
        lt.apply_device(out, a, b, case.ks, batch, case.terms, case.comps, w_hat=w, c0_hat=c0)
        for p0 in range(0, batch, step):
            cnt = min(step, batch - p0)
            lt.apply_device(want[p0:p0 + cnt], a[p0:p0 + cnt], b, case.ks, cnt, case.terms,
                            case.comps, w_hat=w, c0_hat=c0[p0:p0 + cnt])
        torch.cuda.synchronize()
    bad = _differing(torch, out, want, batch)
    assert bad.numel() == 0, f"{bad.numel()} entries differ, first {int(bad[0])}"
    # the ends against the Python-integer reference
    ends = [0, batch - 1]
    idx = torch.tensor(ends, device="cuda")
    expect = ref.apply(_host(a[idx], bits), _host(b, bits), case.ks, q, p, _host(w, bits),
                       _host(c0[idx], bits))
    assert S.mismatching(_host(out[idx], bits), expect, ends) == []
