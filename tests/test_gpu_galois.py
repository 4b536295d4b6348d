"""GPU parity of the automorphism calls (include/nttmul_galois.h, lib/libnttmul_galois.so,
csrc/galois_dev.hpp k_galois_coeff / k_galois_ntt / k_galois_ntt_many): sigma_k over
[batch][limbs][n] operands, one launch per call.

Everything is bit-exact, with outputs preset to the sentinel (all bits set: no canonical word).
The reference is tests/galois_ref.py, Python integers from the definitions, held to the CPU oracle
by tests/test_galois_ref.py; the transforms and the mac are the library's own (nttmul_rns_* up to
n = 4096, nttmul_rnsmp_* above), the products the oracle's.  Shapes (tests/galois_cases.py): n = 256
(four polynomials per workgroup), 4096, 8192 (the first multi-pass n) and 65536 (index products wrap
32 bits; a 64-bit limb polynomial exceeds the LDS), both word classes, L in {1, 3}, batch 3 and 1.
Inputs are seeded random words with 0 and q_l - 1 planted in every limb."""
import ctypes

import numpy as np
import pytest

import galois_cases as C
import galois_ref as ref
import guarded as G
import nttmul
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _to_dev(torch, x, bits):
    x = np.ascontiguousarray(x, dtype=_dt(bits))
    return torch.from_numpy(x.view(np.int32 if bits == 32 else np.int64).reshape(-1)).cuda()


def _sentinels(torch, words, bits):
    return torch.full((words,), -1, dtype=torch.int32 if bits == 32 else torch.int64,
                      device="cuda")


def _from_dev(t, bits, shape):
    return t.cpu().numpy().view(_dt(bits)).reshape(shape)


def _inputs(n, moduli, batch, seed=0):
    bits = C.word_bits(moduli)
    return ref.random_words(np.random.default_rng(n + bits + seed), moduli, batch, n, _dt(bits))


def _single(torch, ctx, op, dx, k, batch, stream=0):
    out = _sentinels(torch, batch * ctx.limbs * ctx.n, ctx.word_bits)
    getattr(ctx, f"{op}_device")(out, dx, k, batch, stream=stream)
    return out


def _id(shape):
    n, moduli, batch = shape
    return f"{n}-u{C.word_bits(moduli)}-L{len(moduli)}-b{batch}"


@pytest.mark.parametrize("shape", C.shapes(), ids=_id)
def test_both_calls_and_many_against_the_reference(shape, torch_cuda):
    """coeff and ntt for every k of ks_at(n) (k = 1: a copy), then ntt_many with 1, 3 and 16
    automorphisms against that many single calls."""
    torch = torch_cuda
    n, moduli, batch = shape
    bits, L = C.word_bits(moduli), len(moduli)
    x = _inputs(n, moduli, batch)
    dx = _to_dev(torch, x, bits)
    with nttmul.GaloisContext(n, moduli) as ctx:
        assert (ctx.n, ctx.limbs, ctx.word_bits) == (n, L, bits)
        for k in C.ks_at(n):
            got = _from_dev(_single(torch, ctx, "coeff", dx, k, batch), bits, x.shape)
            assert np.array_equal(got, ref.coeff(x, k, moduli)), ("coeff", k)
            got = _from_dev(_single(torch, ctx, "ntt", dx, k, batch), bits, x.shape)
            assert np.array_equal(got, ref.ntt(x, k)), ("ntt", k)
        assert np.array_equal(_from_dev(_single(torch, ctx, "coeff", dx, 1, batch), bits, x.shape), x)
        singles = {}
        for count in C.COUNTS:
            ks = C.many_ks(n, count)
            out = _sentinels(torch, count * x.size, bits)
            ctx.ntt_many_device(out, dx, ks, batch)
            got = _from_dev(out, bits, (count,) + x.shape)
            for c, k in enumerate(ks):
                if k not in singles:
                    singles[k] = _from_dev(_single(torch, ctx, "ntt", dx, k, batch), bits, x.shape)
                    assert np.array_equal(singles[k], ref.ntt(x, k)), ("ntt", k)
                assert np.array_equal(got[c], singles[k]), ("ntt_many", count, c, k)
        torch.cuda.synchronize()
        assert np.array_equal(_from_dev(dx, bits, x.shape), x)      # the input is never written


@pytest.mark.parametrize("shape", C.split_shapes(), ids=_id)
def test_coeff_at_every_split(shape, torch_cuda):
    """The sizes between 8192 and 65536 at which the coefficient kernel splits a limb polynomial in
    more residue classes."""
    torch = torch_cuda
    n, moduli, batch = shape
    bits = C.word_bits(moduli)
    x = _inputs(n, moduli, batch, 7)
    dx = _to_dev(torch, x, bits)
    with nttmul.GaloisContext(n, moduli) as ctx:
        assert ctx.kernel_name("coeff") == C.kernel_name("coeff", n, moduli)
        for k in C.ks_at(n):
            got = _from_dev(_single(torch, ctx, "coeff", dx, k, batch), bits, x.shape)
            assert np.array_equal(got, ref.coeff(x, k, moduli)), k


def _transforms(n, moduli):
    """The library's own limb-aware transforms at n: nttmul_rns_* up to 4096, nttmul_rnsmp_* above."""
    return (nttmul.RnsContext if n <= 4096 else nttmul.RnsMpContext)(n, moduli)


@pytest.mark.parametrize("n", C.GALOIS_N)
@pytest.mark.parametrize("basis", C.BASES, ids=("u32", "u64"))
def test_commutes_with_the_librarys_transforms_and_serves_the_mac(n, basis, torch_cuda):
    """inverse(galois_ntt(forward(a), k)) == galois_coeff(a, k), and the rotation-key use:
    mac_ntt(a, galois_ntt(b_hat, k)) is the oracle's product of a with sigma_k(b)."""
    batch, moduli = 2, basis
    a, b = _inputs(n, moduli, batch, 1), _inputs(n, moduli, batch, 2)
    plans = [O.Plan(n, q) for q in moduli]
    with nttmul.GaloisContext(n, moduli) as g, _transforms(n, moduli) as t:
        a_hat, b_hat = t.forward(a), t.forward(b)
        for k in (nttmul.galois_element(n, 1), 2 * n - 1, nttmul.galois_element(n, -3)):
            sa = g.coeff(a, k)
            assert np.array_equal(sa, ref.coeff(a, k, moduli))
            assert np.array_equal(t.inverse(g.ntt(a_hat, k)), sa), k
            assert np.array_equal(t.forward(sa), g.ntt(a_hat, k)), k
            c = t.mac_ntt(a[:, None], g.ntt(b_hat, k)[:, None])
            sb = ref.coeff(b, k, moduli)
            want = np.stack([np.stack([plans[l].product_merged(a[p, l], sb[p, l])
                                       for l in range(len(moduli))]) for p in range(batch)])
            assert np.array_equal(c.astype(np.uint64), want), k


def test_a_non_default_stream(torch_cuda):
    torch = torch_cuda
    n, moduli = C.STREAM
    bits, batch = C.word_bits(moduli), 3
    x = _inputs(n, moduli, batch, 3)
    dx = _to_dev(torch, x, bits)
    side = torch.cuda.Stream()
    ks = C.many_ks(n, 3)
    with nttmul.GaloisContext(n, moduli) as ctx:
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            s = side.cuda_stream
            assert s != 0
            oc = _single(torch, ctx, "coeff", dx, 5, batch, stream=s)
            on = _single(torch, ctx, "ntt", dx, 5, batch, stream=s)
            om = _sentinels(torch, 3 * x.size, bits)
            ctx.ntt_many_device(om, dx, ks, batch, stream=s)
        side.synchronize()
        assert np.array_equal(_from_dev(oc, bits, x.shape), ref.coeff(x, 5, moduli))
        assert np.array_equal(_from_dev(on, bits, x.shape), ref.ntt(x, 5))
        assert np.array_equal(_from_dev(om, bits, (3,) + x.shape),
                              np.stack([ref.ntt(x, k) for k in ks]))


@pytest.mark.parametrize("row", C.VALIDATE, ids=lambda r: f"{r[0]}-u{C.word_bits(r[1])}")
def test_validate_checks_every_word_against_its_own_limb(row, torch_cuda):
    """One word equal to its own limb's modulus, in range for a neighbouring limb: NTTMUL_ERANGE
    from all three calls and nothing written; the same value in the neighbour's limb passes."""
    torch = torch_cuda
    n, moduli, limb, other = row
    bits, batch = C.word_bits(moduli), 3
    x = _inputs(n, moduli, batch, 4)
    bad, fine = x.copy(), x.copy()
    bad[batch - 1, limb, n - 1] = moduli[limb]
    fine[batch - 1, other, n - 1] = moduli[limb]
    with nttmul.GaloisContext(n, moduli, validate=True) as ctx:
        for op in C.OPS:
            ks = C.many_ks(n, 2) if op == "ntt_many" else (3,)
            call = (lambda out, dx: ctx.ntt_many_device(out, dx, ks, batch)) if op == "ntt_many" \
                else (lambda out, dx: getattr(ctx, f"{op}_device")(out, dx, ks[0], batch))
            out = _sentinels(torch, len(ks) * x.size, bits)
            with pytest.raises(nttmul.NttmulError) as ei:
                call(out, _to_dev(torch, bad, bits))
            assert ei.value.status == nttmul.NTTMUL_ERANGE
            torch.cuda.synchronize()
            assert (out == -1).all().item()
            call(out, _to_dev(torch, fine, bits))
            want = np.stack([ref.coeff(fine, k, moduli) if op == "coeff" else ref.ntt(fine, k)
                             for k in ks])
            assert np.array_equal(_from_dev(out, bits, want.shape), want)


@pytest.mark.parametrize("row", C.HOST, ids=lambda r: f"{r[0]}-u{C.word_bits(r[1])}")
def test_host_forms(row):
    n, moduli = row
    x = _inputs(n, moduli, C.HOST_BATCH, 5)
    k = nttmul.galois_element(n, 1)
    with nttmul.GaloisContext(n, moduli) as ctx:
        assert np.array_equal(ctx.coeff(x, k), ref.coeff(x, k, moduli))
        assert np.array_equal(ctx.ntt(x, k), ref.ntt(x, k))
        assert ctx.coeff(x[:0], k).shape == (0, len(moduli), n)


def test_call_refusals_and_sizes(torch_cuda):
    """With a live context: every refusal of the header is NTTMUL_EINVAL and leaves the output
    untouched; batch = 0 is a successful no-op."""
    torch = torch_cuda
    n, moduli = 256, C.BASES[0]
    x = _inputs(n, moduli, 1, 6)
    dx = _to_dev(torch, x, 32)
    out = _sentinels(torch, 17 * x.size, 32)
    EINVAL = nttmul.NTTMUL_EINVAL
    with nttmul.GaloisContext(n, moduli) as ctx:
        lib, h, po, pi = ctx._lib, ctx._h, out.data_ptr(), dx.data_ptr()
        for k in (0, 2, 2 * n, 2 * n + 1, (1 << 32) - 1):
            assert lib.nttmul_galois_coeff_device(h, po, pi, k, 1, 0, None) == EINVAL
            assert lib.nttmul_galois_ntt_device(h, po, pi, k, 1, 0, None) == EINVAL
            assert lib.nttmul_galois_coeff(h, po, pi, k, 1) == EINVAL
            assert lib.nttmul_galois_ntt(h, po, pi, k, 1) == EINVAL
            ks = (ctypes.c_uint32 * 2)(3, k)
            assert lib.nttmul_galois_ntt_many_device(h, po, pi, ks, 2, 1, 0, None) == EINVAL
        ks = (ctypes.c_uint32 * 17)(*([3] * 17))
        assert lib.nttmul_galois_ntt_many_device(h, po, pi, ks, 0, 1, 0, None) == EINVAL
        assert lib.nttmul_galois_ntt_many_device(h, po, pi, ks, 17, 1, 0, None) == EINVAL
        assert lib.nttmul_galois_ntt_many_device(h, po, pi, None, 1, 1, 0, None) == EINVAL
        assert lib.nttmul_galois_ntt_many_device(h, None, pi, ks, 1, 1, 0, None) == EINVAL
        assert lib.nttmul_galois_coeff_device(h, None, pi, 3, 1, 0, None) == EINVAL
        assert lib.nttmul_galois_ntt_device(h, po, None, 3, 1, 0, None) == EINVAL
        assert lib.nttmul_galois_ntt_device(h, po, pi, 3, 1, 99, None) == nttmul.NTTMUL_ENODEV
        # batch = 0: a no-op, NULL operands allowed
        assert lib.nttmul_galois_coeff_device(h, None, None, 3, 0, 0, None) == nttmul.NTTMUL_OK
        assert lib.nttmul_galois_ntt_device(h, po, pi, 3, 0, 0, None) == nttmul.NTTMUL_OK
        assert lib.nttmul_galois_ntt_many_device(h, po, pi, ks, 16, 0, 0, None) == nttmul.NTTMUL_OK
        assert lib.nttmul_galois_ntt(h, None, None, 3, 0) == nttmul.NTTMUL_OK
        buf = ctypes.create_string_buffer(64)
        assert lib.nttmul_galois_kernel_name(h, 3, 1, buf, len(buf)) == EINVAL
        assert lib.nttmul_galois_kernel_name(h, 2, 0, buf, len(buf)) == EINVAL
        assert lib.nttmul_galois_kernel_name(h, 2, 17, buf, len(buf)) == EINVAL
        assert lib.nttmul_galois_kernel_name(h, 0, 0, buf, 4) == len("k_galois_coeff<u32,0>")
        assert buf.value == b"k_g"
        torch.cuda.synchronize()
        assert (out == -1).all().item()
        for limb, q in enumerate(moduli):
            info = ctx.limb_info(limb)
            assert (info.n, info.q, info.word_bits) == (n, q, 32)
            assert info.psi == nttmul.smallest_psi(n, q)


@pytest.mark.parametrize("n", C.ALL_N)
def test_mirror_agrees_with_the_library_dispatch(n):
    for basis in C.BASES:
        for L in C.LIMBS:
            with nttmul.GaloisContext(n, basis[:L]) as ctx:
                for op in C.OPS:
                    assert ctx.kernel_name(op, 3) == C.kernel_name(op, n, basis[:L])
    assert G.sentinel(32) >= max(C.BASES[0]) and G.sentinel(64) >= max(C.BASES[1])
