"""Every kernel built on galois_slot (csrc/galois_dev.hpp) run on every element of
tests/galois_sweep.py S(n): every 2-adic valuation of k - 1 and k + 1, and at n = 256 every odd k.

The slot permutation of sigma_k is obtained once per (word class, n, k) by
galois_sweep.derived_perm from the library's own forward transform (held to the oracle by
tests/test_gpu_parity.py and test_gpu_rnsmp.py) of x and of sigma_k(x), the latter written on the
host from the definition: it is read off the data, not from galois_slot's formula or its mirror.
Then
  galois_coeff                == galois_ref.coeff (the scatter of the definition),
  galois_ntt, galois_ntt_many == index_select(x_hat, src_k),
  hoist_ntt, ksntt_mac        : result (r, .) of a 16-rotation call == the same context's call with
                                k = {1} on index_select(a_hat, src_{k_r}) against b_hat[r],
  lintrans_apply              : one rotation with weights and c_0 == k = {1} on the permuted a_hat
                                and c0_hat; 16 rotations without either == the sum mod m_l of the
                                16 single k = {1} results,
which holds each permuting path to the identity path, and that to the oracle by the parity tests.
Every run: rnsmp_cases.BASIS32 / BASIS64 cut to 2 limbs, batch 5, terms 2, comps 2, outputs preset
to the sentinel, every word compared, and the count of elements run asserted equal to |S(n)|."""
import numpy as np
import pytest

import bconv_ref as B
import galois_ref
import galois_sweep as W
import nttmul

pytestmark = pytest.mark.gpu

BATCH, TERMS, COMPS, LIMBS = W.BATCH, W.TERMS, W.COMPS, W.LIMBS


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _tdt(torch, bits):
    return torch.int32 if bits == 32 else torch.int64


def _to_dev(torch, x, bits):
    x = np.ascontiguousarray(x, dtype=_dt(bits))
    return torch.from_numpy(x.view(np.int32 if bits == 32 else np.int64)).cuda()


def _blank(torch, bits, *shape):
    """An output preset to the sentinel: all bits set, no canonical word."""
    return torch.full(shape, -1, dtype=_tdt(torch, bits), device="cuda")


def _hoist_ctx(n):
    return nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext


def _rows(op):
    return [pytest.param(r.bits, r.n, id=f"u{r.bits}-n{r.n}") for r in W.rows() if r.op == op]


_PERMS = {}


def _perms(torch, bits, n):
    """{k: src_k on the device} for every k of S(n), from the library's forward of x and of
    sigma_k(x); both limbs must give the same table."""
    if (bits, n) not in _PERMS:
        m, dt, ks = W.moduli(bits), _dt(bits), W.S(n)
        x = np.zeros((1, LIMBS, n), dtype=dt)
        x[0, :, 1] = 1
        imgs = np.stack([W.monomial_image(n, k, m, dt) for k in ks])
        with _hoist_ctx(n)(n, m) as ctx:
            fwd_x, fwd = ctx.forward(x)[0], ctx.forward(imgs)
        out = {}
        for i, k in enumerate(ks):
            src = W.derived_perm(fwd_x[0], fwd[i, 0])
            assert np.array_equal(fwd[i, 1], fwd_x[1][src]), (k, "limb 1 disagrees with limb 0")
            out[k] = torch.from_numpy(src).cuda()
        assert np.array_equal(out[1].cpu().numpy(), np.arange(n))
        _PERMS[(bits, n)] = out
    return _PERMS[(bits, n)]


def _words(torch, bits, seed, polys, n, moduli):
    """Seeded canonical words [polys, len(moduli), n] on the device, and on the host."""
    x = B.random_words(np.random.default_rng(seed), moduli, polys, n, _dt(bits))
    return _to_dev(torch, x, bits), x


def _permuted(t, src):
    return t.index_select(-1, src).contiguous()


@pytest.mark.parametrize("bits,n", _rows("coeff"))
def test_galois_coeff(bits, n, torch_cuda):
    torch = torch_cuda
    m = W.moduli(bits)
    x = galois_ref.random_words(np.random.default_rng(n + bits), m, BATCH, n, _dt(bits))
    dx = _to_dev(torch, x, bits)
    ran = 0
    with nttmul.GaloisContext(n, m) as g:
        assert g.kernel_name("coeff") in W.kernels_of(W.Row("coeff", bits, n))
        for k in W.S(n):
            out = _blank(torch, bits, BATCH, LIMBS, n)
            g.coeff_device(out, dx, k, BATCH)
            got = out.cpu().numpy().view(_dt(bits))
            assert np.array_equal(got, galois_ref.coeff(x, k, m)), k
            ran += 1
    assert ran == len(W.S(n))


@pytest.mark.parametrize("bits,n", _rows("ntt"))
def test_galois_ntt_and_ntt_many(bits, n, torch_cuda):
    torch = torch_cuda
    m = W.moduli(bits)
    perms = _perms(torch, bits, n)
    dx, _ = _words(torch, bits, n + bits + 1, BATCH, n, m)
    ran = many = 0
    with nttmul.GaloisContext(n, m) as g:
        assert g.kernel_name("ntt") in W.kernels_of(W.Row("ntt", bits, n))
        assert g.kernel_name("ntt_many", W.LIST) in W.kernels_of(W.Row("ntt_many", bits, n))
        for ks in W.lists(n):
            outs = _blank(torch, bits, len(ks), BATCH, LIMBS, n)
            g.ntt_many_device(outs, dx, ks, BATCH)
            for c, k in enumerate(ks):
                want = _permuted(dx, perms[k])
                out = _blank(torch, bits, BATCH, LIMBS, n)
                g.ntt_device(out, dx, k, BATCH)
                assert torch.equal(out, want), k
                assert torch.equal(outs[c], want), (k, "many")
                ran += 1
            many += len(ks)
    assert ran == many == len(W.S(n))


def _mac_operands(torch, bits, n, m, rots, seed):
    """a_hat [batch, terms, M, n] and b_hat [rots, comps, terms, M, n] on the device."""
    da, _ = _words(torch, bits, seed, BATCH, n, m * TERMS)
    db, _ = _words(torch, bits, seed + 1, rots, n, m * (TERMS * COMPS))
    return da.view(BATCH, TERMS, len(m), n), db.view(rots, COMPS, TERMS, len(m), n)


def _sweep_mac(torch, bits, n, call):
    """call(out, a_hat, b_hat, ks): result (r, .) of every list's call against the k = {1} call on
    the permuted a_hat and b_hat[r]; returns the number of elements run."""
    m = W.moduli(bits)
    perms = _perms(torch, bits, n)
    da, db = _mac_operands(torch, bits, n, m, W.LIST, n + bits + 2)
    ran = 0
    for ks in W.lists(n):
        assert ks[0] != 1 or len(ks) == 1
        b = db[:len(ks)]
        c = _blank(torch, bits, BATCH, len(ks), COMPS, LIMBS, n)
        call(c, da, b, ks)
        for r, k in enumerate(ks):
            want = _blank(torch, bits, BATCH, 1, COMPS, LIMBS, n)
            call(want, _permuted(da, perms[k]), b[r], (1,))
            assert torch.equal(c[:, r], want[:, 0]), k
            ran += 1
        del c
    return ran


@pytest.mark.parametrize("bits,n", _rows("hoist"))
def test_hoist_ntt(bits, n, torch_cuda):
    with _hoist_ctx(n)(n, W.moduli(bits)) as ctx:
        assert ctx.hoist_kernel_name(COMPS).split(" + ")[0] in W.kernels_of(W.Row("hoist", bits, n))
        ran = _sweep_mac(torch_cuda, bits, n, lambda c, a, b, ks: ctx.hoist_ntt_device(
            c, a, b, ks, BATCH, TERMS, COMPS))
        torch_cuda.cuda.synchronize()
    assert ran == len(W.S(n))


@pytest.mark.parametrize("bits,n", _rows("ksntt_mac"))
def test_ksntt_mac(bits, n, torch_cuda):
    m = W.moduli(bits)
    with nttmul.NttKeySwitch(n, m[:1], m[1:], 1) as kn:
        assert [kn.kernel_name("mac", COMPS)] == W.kernels_of(W.Row("ksntt_mac", bits, n))
        ran = _sweep_mac(torch_cuda, bits, n, lambda c, a, b, ks: kn.mac_device(
            c, a, b, ks, BATCH, TERMS, COMPS))
        torch_cuda.cuda.synchronize()
    assert ran == len(W.S(n))


@pytest.mark.parametrize("bits,n", _rows("lintrans_one"))
def test_lintrans_one_rotation_with_weights_and_c0(bits, n, torch_cuda):
    torch = torch_cuda
    m = W.moduli(bits)
    q, p = m[:1], m[1:]
    perms = _perms(torch, bits, n)
    da, db = _mac_operands(torch, bits, n, m, W.LIST, n + bits + 3)
    dw, _ = _words(torch, bits, n + bits + 4, W.LIST, n, m)          # [rots, M, n]
    dz, _ = _words(torch, bits, n + bits + 5, BATCH, n, q)           # [batch, L, n]
    ran = 0
    with nttmul.NttLinTrans(n, q, p) as lt:
        assert [lt.kernel_name(COMPS, True)] == W.kernels_of(W.Row("lintrans_one", bits, n))
        for i, k in enumerate(W.S(n)):
            r = i % W.LIST
            got = _blank(torch, bits, BATCH, COMPS, LIMBS, n)
            want = _blank(torch, bits, BATCH, COMPS, LIMBS, n)
            lt.apply_device(got, da, db[r], (k,), BATCH, TERMS, COMPS, w_hat=dw[r], c0_hat=dz)
            lt.apply_device(want, _permuted(da, perms[k]), db[r], (1,), BATCH, TERMS, COMPS,
                            w_hat=dw[r], c0_hat=_permuted(dz, perms[k]))
            assert torch.equal(got, want), k
            ran += 1
        torch.cuda.synchronize()
    assert ran == len(W.S(n))


@pytest.mark.parametrize("bits,n", _rows("lintrans_sum"))
def test_lintrans_sixteen_rotations_sum(bits, n, torch_cuda):
    """w_hat = NULL and c0_hat = NULL: the sum mod m_l of the single-rotation k = {1} results,
    formed in int64 with one conditional subtraction per addition (two canonical words stay below 2^63)."""
    torch = torch_cuda
    m = W.moduli(bits)
    q, p = m[:1], m[1:]
    perms = _perms(torch, bits, n)
    da, db = _mac_operands(torch, bits, n, m, W.LIST, n + bits + 6)
    mod = torch.tensor([int(v) for v in m], dtype=torch.int64, device="cuda").view(1, 1, LIMBS, 1)
    ran = 0
    with nttmul.NttLinTrans(n, q, p) as lt:
        assert [lt.kernel_name(COMPS, False)] == W.kernels_of(W.Row("lintrans_sum", bits, n))
        for ks in W.lists(n):
            assert ks[0] != 1 or len(ks) == 1
            got = _blank(torch, bits, BATCH, COMPS, LIMBS, n)
            lt.apply_device(got, da, db[:len(ks)], ks, BATCH, TERMS, COMPS)
            acc = torch.zeros((BATCH, COMPS, LIMBS, n), dtype=torch.int64, device="cuda")
            for r, k in enumerate(ks):
                one = _blank(torch, bits, BATCH, COMPS, LIMBS, n)
                lt.apply_device(one, _permuted(da, perms[k]), db[r], (1,), BATCH, TERMS, COMPS)
                assert bool((one >= 0).all()), "canonical words are below 2^62"
                acc = acc + one.to(torch.int64)
                acc = torch.where(acc >= mod, acc - mod, acc)
                ran += 1
            assert torch.equal(got.to(torch.int64), acc), ks
    assert ran == len(W.S(n))
