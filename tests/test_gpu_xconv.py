"""GPU parity of the exact base extension and the rounded ModDown (include/nttmul_xconv.h,
lib/libnttmul_xconv.so, csrc/xconv_dev.hpp k_xconv_*): two launches per sub-batch up to n = 4096,
four above.

Every case is compared, on every word of the NTT-domain output and at every degree, with the CPU
reference (tests/full_ref.py over tests/xconv_ref.py and the oracle's transforms), which shares no
code with the device; and beside it with the device composition on every coefficient -- the
library's own inverse transforms over the input's limbs, the same reference arithmetic, the
library's inverse over Q of the output (tests/xconv_gpu.py check).  Every output is preset to the
sentinel in a guarded arena (tests/guarded.py).  The seeded inputs hold no coefficient inside the
guard band (tests/test_xconv_ref.py), so every comparison is exact; the band itself is the edge
polynomial's test."""
from fractions import Fraction
from math import prod

import numpy as np
import pytest

import full_ref as F
import hoist_ref as H
import nttmul
import xconv_cases as C
import xconv_ref as ref
from xconv_gpu import (call as _call, check as _check, ctx as _ctx,
                       dt as _dt, to_dev as _to_dev)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _id(case):
    return f"{case.op}-u{case.bits}-n{case.n}x{case.batch}-{case.L}.{case.K}-t{case.t}"


@pytest.mark.parametrize("case", C.parity_cases(), ids=_id)
def test_parity(case, torch_cuda):
    """Both operations, both classes, both scales: grid and pairs (batch 3 and 33), the limb
    counts, K + 1 over the fold cadence, every degree."""
    q, p = C.moduli_of(case)
    x = C.seeded_input(case)
    with nttmul.NttExactConv(case.n, q, p, case.t) as xc:
        assert (xc.q_limbs, xc.p_limbs, xc.word_bits) == (case.L, case.K, case.bits)
        assert (xc.info.n, 1 << xc.info.logn, xc.info.ndev, xc.info.scratch_mb) == \
            (case.n, case.n, 1, C.DEFAULT_SCRATCH_MB)
        assert (xc.info.scale, xc.info.band_log2) == (case.t, C.BAND_LOG2)
        got = _call(torch_cuda, xc, case.op, x)
    _check(case.op, case.n, q, p, case.t, x, got)


# ---- the edge polynomial: the test of the correction itself -------------------------------------

def _edge_values(P, eps):
    """[t X]_P of the edge coefficients: the ends, the middle, just outside the band on both sides
    (d = ceil(eps P) + 1), and three values that lie inside the band wherever it holds an
    integer."""
    d = -(-(eps * P).numerator // (eps * P).denominator) + 1
    e = max(0, int(eps * P) - 1)
    h = (P - 1) // 2
    return [0, 1, P - 1, h, h + 1, h - d, h + 1 + d, h - e, h + 1 + e, h - e // 2]


def _inside(T, P, eps):
    return abs(Fraction(T, P) - Fraction(1, 2)) <= eps


@pytest.mark.parametrize("t", C.SCALES)
@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("K", C.EDGE_K)
@pytest.mark.parametrize("n", C.EDGE_N)
def test_edge_polynomial(n, K, bits, t, torch_cuda):
    """The P part is the library's forward transform of coefficients chosen so that [t X]_P sits at
    0, 1, P - 1, (P -+ 1) / 2, just outside the guard band on both sides and inside it; the rest of
    the polynomial is seeded and the Q part random.  Outside the band both operations are exact;
    inside, the result is one of the two candidates, the same one in every limb."""
    torch = torch_cuda
    L = C.EDGE_L
    case = C.Case("moddown", bits, n, 1, L, K, t)
    q, p = C.moduli_of(case)
    P = prod(p)
    Ctx = _ctx(n)
    with nttmul.NttExactConv(n, q, p, t) as xc, Ctx(n, p) as cp, Ctx(n, q) as cq:
        assert xc.band_log2 >= C.MIN_BAND_LOG2
        eps = xc.eps
        assert eps == Fraction(K, 1 << xc.info.band_log2) <= Fraction(K, 1 << 40)
        values = _edge_values(P, eps)
        rng = np.random.default_rng(n + 10 * K + bits + t)
        coef_p = C.seeded_input(case._replace(op="extend"), seed=n + K + bits)   # [1, K, n]
        tinv = pow(t, -1, P)
        where = [3 + 17 * i for i in range(len(values))]
        for k, T in zip(where, values):
            for j, m in enumerate(p):
                coef_p[0, j, k] = (T * tinv % P) % m
        x_hat_q = np.stack([rng.integers(0, m, size=(1, n), dtype=np.uint64).astype(_dt(bits))
                            for m in q], axis=1)
        p_hat = cp.forward(coef_p)
        coef_q = cq.inverse(x_hat_q)
        x_hat = np.concatenate([x_hat_q, p_hat], axis=1)
        down = cq.inverse(_call(torch, xc, "moddown", x_hat))
        up = cq.inverse(_call(torch, xc, "extend", p_hat))
    # the seeded rest of the polynomial is outside the band, the edge coefficients as constructed
    rest = [k for k in range(n) if k not in where]
    assert ref.count_in_band(coef_p[:, :, rest], p, t, eps) == 0
    want_down = ref.moddown_coeff(np.concatenate([coef_q, coef_p], axis=1), q, p, t)
    want_up = ref.extend_coeff(coef_p, q, p, t)
    assert np.array_equal(down[:, :, rest], want_down[:, :, rest])
    assert np.array_equal(up[:, :, rest], want_up[:, :, rest])
    inside = 0
    for k, T in zip(where, values):
        c = T - P * (T > P // 2)
        assert [int(v) for v in want_up[0, :, k]] == [c % m for m in q]
        if not _inside(T, P, eps):
            assert np.array_equal(down[0, :, k], want_down[0, :, k]), (k, T)
            assert np.array_equal(up[0, :, k], want_up[0, :, k]), (k, T)
            continue
        inside += 1
        # c, or c -+ P on the side of the rounding boundary: the same candidate in every limb
        other = c - P if c > 0 else c + P
        ups = [[cc % m for m in q] for cc in (c, other)]
        assert [int(v) for v in up[0, :, k]] in ups, (k, T)
        downs = [[(int(coef_q[0, l, k]) * t - cc) * pow(P, -1, m) % m for l, m in enumerate(q)]
                 for cc in (c, other)]
        assert downs[0] == [int(v) for v in want_down[0, :, k]]
        assert [int(v) for v in down[0, :, k]] in downs, (k, T)
    # the band holds integers once eps P >= 2: then three of the values lie inside it
    assert inside >= (3 if eps * P >= 2 else 0)
    assert not _inside(values[5], P, eps) and not _inside(values[6], P, eps)


# ---- consistency with the floor form ---------------------------------------------------------------

@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("L,K", ((3, 2), (4, 1), (2, 5)))
def test_consistency_with_the_floor_moddown(L, K, bits, torch_cuda):
    """Outside the band, moddown at t = 1 is mdntt_moddown's output plus [frac(phi) >= 1/2] plus
    alpha in the coefficient domain, alpha = floor(phi) being what the unreduced conversion leaves
    uncorrected.  In Python integers at n = 256."""
    torch = torch_cuda
    n, batch = C.N, 3
    case = C.Case("moddown", bits, n, batch, L, K)
    q, p = C.moduli_of(case)
    x = C.seeded_input(case, seed=L + K + bits)
    with nttmul.NttExactConv(n, q, p) as xc, nttmul.NttModDown(n, q, p) as md, \
            _ctx(n)(n, q) as low, _ctx(n)(n, p) as cp:
        exact = low.inverse(_call(torch, xc, "moddown", x)).astype(object)
        floor = low.inverse(md.moddown(x)).astype(object)
        coef_p = cp.inverse(x[:, L:])
        assert ref.count_in_band(coef_p, p, 1, xc.eps) == 0
    y = ref.y_of(coef_p, p)
    for b in range(batch):
        for k in range(n):
            phi = ref.phi(y[b, :, k], p)
            alpha = phi.numerator // phi.denominator
            up = int(phi - alpha >= Fraction(1, 2))
            for l, m in enumerate(q):
                assert exact[b, l, k] == (floor[b, l, k] + up + alpha) % m, (b, l, k)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,L", C.RESCALE)
def test_rescale_is_the_exact_rounding(n, L, bits, torch_cuda):
    """K = 1, t = 1: the inverse transform of out is round(X / p) mod q_l for random big integers X
    in [0, Q p), the ends of the range among them; and out itself is the CPU reference's, word for
    word."""
    torch = torch_cuda
    batch = C.RESCALE_BATCH
    case = C.rescale_case(bits, n, L)
    q, p = C.moduli_of(case)
    ext = q + p
    X, x = C.rescale_input(case)
    assert ref.count_in_band(x[:, L:], p, 1, Fraction(1, 1 << C.BAND_LOG2)) == 0
    Ctx = _ctx(n)
    with Ctx(n, ext) as big, Ctx(n, q) as low, nttmul.NttExactConv(n, q, p) as xc:
        x_hat = big.forward(x)
        got = _call(torch, xc, "moddown", x_hat)
        back = low.inverse(got)
    assert np.array_equal(x_hat, H.forward(x, ext))
    F.assert_equal(got, F.reference("xconv", "moddown", x_hat, q, p, 1), (n, L, bits))
    for b in range(batch):
        assert np.array_equal(back[b].astype(object), ref.moddown_values(X[b], q, p)), b


# ---- the key switch chain --------------------------------------------------------------------------

@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n", C.CHAIN_N)
def test_the_rounded_key_switch_halves_the_noise(n, bits, torch_cuda):
    """ksntt_modup -> ksntt_mac -> xconv.moddown on hoist_ref.chain's keys: every coefficient of
    c_0 + c_1 s - sigma_k(x) sigma_k(s_2) lies strictly below (1 + h) / 2, which the floor ModDown
    exceeds on the same data (tests/test_xconv_ref.py)."""
    import hoist_cases
    ch = H.chain(n, bits)
    q, p, alpha, ks = ch["q"], ch["p"], ch["alpha"], ch["ks"]
    batch, rots, L = ch["x"].shape[0], len(ks), len(q)
    with _ctx(n)(n, q) as low, nttmul.NttKeySwitch(n, q, p, alpha) as kn, \
            nttmul.NttExactConv(n, q, p) as xc:
        up_hat = kn.modup(low.forward(ch["x"]))
        mid_hat = kn.mac(up_hat, ch["key_hat"], ks)
        flat = np.ascontiguousarray(mid_hat.reshape(batch * rots * 2, L + len(p), n))
        out_hat = _call(torch_cuda, xc, "moddown", flat)
        back = low.inverse(out_hat).reshape(batch, rots, 2, L, n)
    want = ref.moddown_coeff(ch["mid"].reshape(-1, L + len(p), n), q, p)
    F.assert_equal(out_hat, H.forward(want, q), (n, bits))
    assert np.array_equal(back, want.reshape(back.shape))
    errs = H.chain_errors(ch, back)
    assert 2 * max(errs) < 1 + hoist_cases.CHAIN_H, errs


# ---- sub-batches, the host forms, the flag, the device path's rules --------------------------------

@pytest.mark.parametrize("case", C.subbatch_cases(), ids=_id)
def test_sub_batches(case, torch_cuda):
    """scratch_mb = 1: three sub-batches with a partial last one at n = 4096, one polynomial each
    at n = 65536."""
    want = [w for *_, w in C.SUBBATCH if sum(w) == case.batch][0]
    assert C.chunks(case) == list(want) and len(want) == 3
    q, p = C.moduli_of(case)
    x = C.seeded_input(case)
    with nttmul.NttExactConv(case.n, q, p, case.t, scratch_mb=1) as xc:
        assert xc.info.scratch_mb == 1
        one = _call(torch_cuda, xc, case.op, x[:1])   # the scratch grows after this call
        got = _call(torch_cuda, xc, case.op, x)
    assert np.array_equal(one[0], got[0])
    _check(case.op, case.n, q, p, case.t, x, got)


@pytest.mark.parametrize("op", C.OPS)
@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,batch", C.HOST)
def test_host_form_equals_the_device_form(n, batch, bits, op, torch_cuda):
    L, K = C.HOST_SHAPE
    case = C.Case(op, bits, n, batch, L, K)
    q, p = C.moduli_of(case)
    x = C.seeded_input(case)
    with nttmul.NttExactConv(n, q, p) as xc:
        assert xc.io_dtype == _dt(bits)
        dev = _call(torch_cuda, xc, op, x)
        host = getattr(xc, op)(x)
        assert host.dtype == _dt(bits) and np.array_equal(host, dev)
        assert getattr(xc, op)(x[:0]).shape == (0, L, n)
        with pytest.raises(ValueError):
            getattr(xc, op)(np.zeros((1, L + K + 1, n), dtype=_dt(bits)))
    _check(op, n, q, p, 1, x, dev)


@pytest.mark.parametrize("op", C.OPS)
@pytest.mark.parametrize("bits", (32, 64))
def test_validate_flag_leaves_the_output_untouched(bits, op, torch_cuda):
    """A word equal to its own limb's modulus (in range for the limb before it: the primes
    descend) is NTTMUL_ERANGE and out is untouched; a clean input succeeds; without the flag there
    is no check."""
    torch = torch_cuda
    n, batch, (L, K) = C.VALIDATE
    case = C.Case(op, bits, n, batch, L, K, 1, True)
    q, p = C.moduli_of(case)
    mods = p if op == "extend" else q + p
    assert all(a > b for a, b in zip(mods, mods[1:]))
    good = C.seeded_input(case)
    with nttmul.NttExactConv(n, q, p, validate=True) as strict, \
            nttmul.NttExactConv(n, q, p) as lax:
        got = _call(torch, strict, op, good)
        assert np.array_equal(got, _call(torch, lax, op, good))
        _check(op, n, q, p, 1, good, got)
        for limb in (1, len(mods) - 1):
            bad = good.copy()
            bad[batch - 1, limb, n - 1] = mods[limb]
            out = torch.full((batch * L * n,), -1,
                             dtype=torch.int32 if bits == 32 else torch.int64, device="cuda")
            with pytest.raises(nttmul.NttmulError) as ei:
                getattr(strict, f"{op}_device")(out, _to_dev(torch, bad, bits), batch)
            assert ei.value.status == nttmul.NTTMUL_ERANGE, limb
            torch.cuda.synchronize()
            assert bool((out == -1).all())
            _call(torch, lax, op, bad)


def test_device_path_rules(torch_cuda):
    """A non-default stream; the empty batch; bad arguments on a live context."""
    torch = torch_cuda
    case = C.Case("moddown", 32, C.N, 3, 3, 2, 65537)
    q, p = C.moduli_of(case)
    with nttmul.NttExactConv(C.N, q, p, case.t) as xc:
        side = torch.cuda.Stream()
        x = C.seeded_input(case)
        got = _call(torch, xc, "moddown", x, stream=side.cuda_stream)
        F.assert_equal(got, F.reference("xconv", "moddown", x, q, p, case.t))
        out = torch.full((C.N,), 7, dtype=torch.int32, device="cuda")
        for op in C.OPS:
            fn = getattr(xc._lib, f"nttmul_xconv_{op}_device")
            getattr(xc, f"{op}_device")(out, out, 0)                     # batch = 0: a no-op
            torch.cuda.synchronize()
            assert bool((out == 7).all())
            assert fn(xc._h, None, out.data_ptr(), 1, 0, None) == nttmul.NTTMUL_EINVAL
            assert fn(xc._h, out.data_ptr(), None, 1, 0, None) == nttmul.NTTMUL_EINVAL
            assert fn(xc._h, None, None, 0, 0, None) == nttmul.NTTMUL_OK
            assert fn(xc._h, out.data_ptr(), out.data_ptr(), 1, 99, None) == nttmul.NTTMUL_ENODEV
            host = getattr(xc._lib, f"nttmul_xconv_{op}")
            assert host(xc._h, None, None, 0) == nttmul.NTTMUL_OK
            assert host(xc._h, None, out.data_ptr(), 1) == nttmul.NTTMUL_EINVAL
            with pytest.raises(ValueError):                              # too small a tensor
                getattr(xc, f"{op}_device")(out, out, 2)
        name = xc._lib.nttmul_xconv_kernel_name
        assert name(xc._h, 1, None, 1) == nttmul.NTTMUL_EINVAL
        assert name(xc._h, 2, None, 0) == nttmul.NTTMUL_EINVAL
        assert name(xc._h, 1, None, 0) == len(C.kernel_name("moddown", C.N, 32))


def test_mirror_agrees_with_the_library_dispatch(torch_cuda):
    """tests/xconv_cases.py kernel_name against nttmul_xconv_kernel_name at every degree, and the
    names are kernels the library holds."""
    held = nttmul.kernel_hashes(nttmul.XCONV_LIB_PATH)
    for bits in (32, 64):
        for n in C.ALL_N:
            q, p = C.moduli_of(C.Case("extend", bits, n, 1, 2, 1))
            with nttmul.NttExactConv(n, q, p) as xc:
                for op in C.OPS:
                    name = xc.kernel_name(op)
                    assert name == C.kernel_name(op, n, bits)
                    for part in name.split(" + "):
                        assert nttmul.dispatch_key(part) in held
