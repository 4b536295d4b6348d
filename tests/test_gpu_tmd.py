"""GPU parity of BGV's plaintext-preserving ModDown (include/nttmul_tmd.h, lib/libnttmul_tmd.so,
csrc/tmd_dev.hpp k_tmd_*): two launches per sub-batch up to n = 4096, four above.

At every degree every word of the NTT-domain output is compared bit for bit with the CPU reference
(tests/full_ref.py over tests/tmd_ref.py and the oracle's transforms), which shares no code with
the device; beside it the output is held to the identity out = nttmul_mdntt_moddown(x_hat) -
forward(u mod q_l) (tests/tmd_gpu.py), which says which side is wrong.  Every output is preset to the sentinel in a guarded arena
(tests/guarded.py).  Everything is integer arithmetic: no comparison is conditional on the data."""
from math import prod

import numpy as np
import pytest

import full_ref as F
import hoist_cases
import hoist_ref as H
import ks_ref
import nttmul
import tmd_cases as C
import tmd_ref as ref
from tmd_gpu import call as _call, check as _check, ctx as _ctx, dt as _dt, to_dev as _to_dev
from xconv_ref import _crt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _id(case):
    return f"u{case.bits}-n{case.n}x{case.batch}-{case.L}.{case.K}-t{case.t}"


@pytest.mark.parametrize("case", C.parity_cases(), ids=_id)
def test_parity(case, torch_cuda):
    """Bit for bit tmd_ref: both classes, the three plaintext moduli, K + 1 on both sides of both
    fold cadences, batch 3 (a workgroup ends partial)."""
    q, p = C.moduli_of(case)
    x = C.seeded_input(case)
    with nttmul.NttPlainModDown(case.n, q, p, case.t) as tm:
        assert (tm.q_limbs, tm.p_limbs, tm.word_bits) == (case.L, case.K, case.bits)
        assert (tm.info.n, 1 << tm.info.logn, tm.info.ndev, tm.info.scratch_mb) == \
            (case.n, case.n, 1, C.DEFAULT_SCRATCH_MB)
        assert (tm.info.t, tm.msg_factor) == (case.t, pow(prod(p), -1, case.t))
        got = _call(torch_cuda, tm, x)
    F.assert_equal(got, F.reference("tmd", "moddown", x, q, p, case.t), _id(case))


@pytest.mark.parametrize("case", C.identity_cases() + C.degree_cases(), ids=_id)
def test_the_identity_at_every_kernel_size(case, torch_cuda):
    """Every word is the CPU reference's; and out == mdntt_moddown(x_hat) - forward(u mod q_l), u
    from the library's own inverse of the P limbs and Python integers."""
    q, p = C.moduli_of(case)
    x = C.seeded_input(case)
    with nttmul.NttPlainModDown(case.n, q, p, case.t) as tm:
        got = _call(torch_cuda, tm, x)
    _check(case.n, q, p, case.t, x, got)


@pytest.mark.parametrize("case", C.subbatch_cases(), ids=_id)
def test_sub_batches(case, torch_cuda):
    """scratch_mb = 1 at n = 8192: three sub-batches with a partial last one."""
    want = [w for *_, w in C.SUBBATCH if sum(w) == case.batch][0]
    assert C.chunks(case) == list(want) and len(want) == 3
    q, p = C.moduli_of(case)
    x = C.seeded_input(case)
    with nttmul.NttPlainModDown(case.n, q, p, case.t, scratch_mb=1) as tm:
        assert tm.info.scratch_mb == 1
        one = _call(torch_cuda, tm, x[:1])            # the scratch grows after this call
        got = _call(torch_cuda, tm, x)
    assert np.array_equal(one[0], got[0])
    _check(case.n, q, p, case.t, x, got)


# ---- the edge polynomial: the test of the correction itself -------------------------------------

def _edge_y(p, t, v, alpha, rng):
    """y with sum_j y_j g_j = v (mod t) and floor(sum_j y_j / p_j) = alpha, or None where none
    was found (K = 1 and t > p_0: y_0 is fixed by v and may not be a residue)."""
    K = len(p)
    g = [-pow(m, -1, t) % t for m in p]
    ginv = pow(g[0], -1, t)
    for _ in range(400):
        if alpha == 0:                                # every y_j / p_j below 1 / K
            lo = [0] * K
            hi = [m // K for m in p]
        else:                                         # every y_j / p_j at or above (K - 1) / K
            lo = [-(-m * (K - 1) // K) for m in p]
            hi = list(p)
        y = [lo[j] + int.from_bytes(rng.bytes(8), "little") % (hi[j] - lo[j]) for j in range(K)]
        r = (v - sum(a * b for a, b in zip(y[1:], g[1:]))) * ginv % t
        # y_0 = r (mod t) inside [lo_0, hi_0)
        y0 = lo[0] + (r - lo[0]) % t
        if y0 >= hi[0]:
            continue
        steps = (hi[0] - 1 - y0) // t
        y[0] = y0 + t * (int.from_bytes(rng.bytes(8), "little") % (steps + 1))
        if sum(a * b for a, b in zip(y, g)) % t == v and \
                sum(a * (prod(p) // m) for a, m in zip(y, p)) // prod(p) == alpha:
            return y
    return None


@pytest.mark.parametrize("which", range(3))
@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("K", C.EDGE_K)
@pytest.mark.parametrize("n", C.EDGE_N)
def test_edge_polynomial(n, K, bits, which, torch_cuda):
    """Entry 0: the P part is the library's forward transform of coefficients built so that
    v = 0, 1, (t - 1) / 2, (t + 1) / 2 and t - 1, each with alpha = 0 and alpha = K - 1, the rest
    seeded, and x_hat's Q limbs are all q_l - 1.  Entry 1: every y_j = p_j - 1, the worst-case
    fill of both accumulators, and x_hat's Q limbs are all 0."""
    L = C.EDGE_L
    t = C.plain_moduli(bits)[which]
    case = C.Case(bits, n, 2, L, K, t)
    q, p = C.moduli_of(case)
    P = prod(p)
    rng = np.random.default_rng(n + 10 * K + bits + which)
    coef_p = C.seeded_input(case, seed=n + K + bits)[:, L:]                  # [2, K, n]
    targets = [(v, a) for v in (0, 1, (t - 1) // 2, (t + 1) // 2, t - 1) for a in {0, K - 1}]
    placed = []
    for i, (v, a) in enumerate(targets):
        y = _edge_y(p, t, v, a, rng)
        if y is None:
            continue
        k = 3 + 17 * i
        for j, m in enumerate(p):
            coef_p[0, j, k] = y[j] * (P // m) % m                            # y_j = x_j Ph_j^-1
        placed.append((k, v, a))
    # everything is reachable unless one y_0 has to hit one residue of a t above p_0
    assert len(placed) == len(targets) or (K == 1 and t > p[0])
    assert len(placed) >= (1 if K == 1 and t > p[0] else len(targets))
    for j, m in enumerate(p):
        coef_p[1, j, :] = -(P // m) % m                                      # y_j = p_j - 1
    y = ref.y_of(coef_p, p)
    assert all(int(y[1, j, k]) == m - 1 for j, m in enumerate(p) for k in (0, n - 1))
    u = ref.u_of(coef_p, p, t)
    for k, v, a in placed:
        assert int(u[0, k]) == (v if v <= (t - 1) // 2 else v - t)
        assert sum(int(y[0, j, k]) * (P // m) for j, m in enumerate(p)) // P == a
    x_q = np.stack([np.stack([np.full(n, m - 1), np.zeros(n, dtype=np.int64)]) for m in q],
                   axis=1).astype(_dt(bits))                                 # [2, L, n]
    with _ctx(n)(n, p) as cp, nttmul.NttPlainModDown(n, q, p, t) as tm:
        x_hat = np.concatenate([x_q, cp.forward(coef_p)], axis=1)
        got = _call(torch_cuda, tm, x_hat)
    _check(n, q, p, t, x_hat, got)


# ---- the flag, the device path's rules --------------------------------------------------------------

@pytest.mark.parametrize("bits", (32, 64))
def test_validate_flag_leaves_the_output_untouched(bits, torch_cuda):
    """A word equal to its own limb's modulus (in range for the limb before it: the primes
    descend) is NTTMUL_ERANGE and out is untouched; a clean input succeeds; without the flag there
    is no check."""
    torch = torch_cuda
    n, batch, (L, K) = C.VALIDATE
    t = 65537
    case = C.Case(bits, n, batch, L, K, t, True)
    q, p = C.moduli_of(case)
    mods = q + p
    assert all(a > b for a, b in zip(mods, mods[1:]))
    good = C.seeded_input(case)
    with nttmul.NttPlainModDown(n, q, p, t, validate=True) as strict, \
            nttmul.NttPlainModDown(n, q, p, t) as lax:
        got = _call(torch, strict, good)
        assert np.array_equal(got, _call(torch, lax, good))
        _check(n, q, p, t, good, got)
        for limb in (1, len(mods) - 1):
            bad = good.copy()
            bad[batch - 1, limb, n - 1] = mods[limb]
            out = torch.full((batch * L * n,), -1,
                             dtype=torch.int32 if bits == 32 else torch.int64, device="cuda")
            with pytest.raises(nttmul.NttmulError) as ei:
                strict.moddown_device(out, _to_dev(torch, bad, bits), batch)
            assert ei.value.status == nttmul.NTTMUL_ERANGE, limb
            torch.cuda.synchronize()
            assert bool((out == -1).all())
            _call(torch, lax, bad)


def test_device_path_rules(torch_cuda):
    """A non-default stream; the host form; the empty batch; bad arguments on a live context."""
    torch = torch_cuda
    n, t = 256, 65537
    case = C.Case(32, n, 3, 3, 2, t)
    q, p = C.moduli_of(case)
    with nttmul.NttPlainModDown(n, q, p, t) as tm:
        side = torch.cuda.Stream()
        x = C.seeded_input(case)
        got = _call(torch, tm, x, stream=side.cuda_stream)
        assert np.array_equal(got, ref.moddown(x, q, p, t))
        host = tm.moddown(x)
        assert host.dtype == np.uint32 and np.array_equal(host, got)
        assert tm.moddown(x[:0]).shape == (0, 3, n)
        with pytest.raises(ValueError):
            tm.moddown(np.zeros((1, 6, n), dtype=np.uint32))
        out = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        fn = tm._lib.nttmul_tmd_moddown_device
        tm.moddown_device(out, out, 0)                                       # batch = 0: a no-op
        torch.cuda.synchronize()
        assert bool((out == 7).all())
        assert fn(tm._h, None, out.data_ptr(), 1, 0, None) == nttmul.NTTMUL_EINVAL
        assert fn(tm._h, out.data_ptr(), None, 1, 0, None) == nttmul.NTTMUL_EINVAL
        assert fn(tm._h, None, None, 0, 0, None) == nttmul.NTTMUL_OK
        assert fn(tm._h, out.data_ptr(), out.data_ptr(), 1, 99, None) == nttmul.NTTMUL_ENODEV
        hostfn = tm._lib.nttmul_tmd_moddown
        assert hostfn(tm._h, None, None, 0) == nttmul.NTTMUL_OK
        assert hostfn(tm._h, None, out.data_ptr(), 1) == nttmul.NTTMUL_EINVAL
        with pytest.raises(ValueError):                                      # too small a tensor
            tm.moddown_device(out, out, 2)
        name = tm._lib.nttmul_tmd_kernel_name
        assert name(tm._h, None, 1) == nttmul.NTTMUL_EINVAL
        assert name(tm._h, None, 0) == len(C.kernel_name(n, 32))


def test_mirror_agrees_with_the_library_dispatch(torch_cuda):
    """tests/tmd_cases.py kernel_name against nttmul_tmd_kernel_name at every degree, and the
    names are kernels the library holds."""
    held = nttmul.kernel_hashes(nttmul.TMD_LIB_PATH)
    for bits in (32, 64):
        for n in C.ALL_N:
            q, p = C.moduli_of(C.Case(bits, n, 1, 2, 1, 3))
            with nttmul.NttPlainModDown(n, q, p, 3) as tm:
                name = tm.kernel_name()
                assert name == C.kernel_name(n, bits)
                for part in name.split(" + "):
                    assert nttmul.dispatch_key(part) in held


# ---- the key switch chain: the BGV invariant --------------------------------------------------------

@pytest.mark.parametrize("t", C.CHAIN_T)
@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n", C.CHAIN_N)
def test_the_key_switch_keeps_the_error_a_multiple_of_t(n, bits, t, torch_cuda):
    """ksntt_modup -> ksntt_mac -> tmd_moddown on hoist_ref.chain's zero-noise keys:
    e = c_0' + c_1' s - sigma_k(x) sigma_k(s2), centred mod Q, has every coefficient = 0 (mod t)
    and |e| <= (K + (t + 1) / 2)(1 + h) (tests/test_tmd_ref.py derives it: d_0 + d_1 s is a
    multiple of P and of t).  The control: nttmul_mdntt_moddown's output of the same data has a
    coefficient that is not, so the check can fail."""
    ch = H.chain(n, bits)
    q, p, alpha, ks = ch["q"], ch["p"], ch["alpha"], ch["ks"]
    batch, rots, L, K = ch["x"].shape[0], len(ks), len(q), len(p)
    with _ctx(n)(n, q) as low, nttmul.NttKeySwitch(n, q, p, alpha) as kn, \
            nttmul.NttPlainModDown(n, q, p, t) as tm, nttmul.NttModDown(n, q, p) as md:
        up_hat = kn.modup(low.forward(ch["x"]))
        mid_hat = kn.mac(up_hat, ch["key_hat"], ks)
        flat = np.ascontiguousarray(mid_hat.reshape(batch * rots * 2, L + K, n))
        out_hat = _call(torch_cuda, tm, flat)
        back = low.inverse(out_hat).reshape(batch, rots, 2, L, n)
        floor = low.inverse(md.moddown(flat)).reshape(batch, rots, 2, L, n)
    want = ref.moddown_coeff(ch["mid"].reshape(-1, L + K, n), q, p, t)
    F.assert_equal(out_hat, H.forward(want, q), (n, bits, t))
    assert np.array_equal(back, want.reshape(back.shape))
    es = C.chain_error_polys(ch, back)
    assert len(es) == batch * rots
    assert all(v % t == 0 for e in es for v in e)
    worst = max(abs(v) for e in es for v in e)
    print("tmd chain error", n, bits, t, worst, "bound", ref.bound(K, t) * (1 + hoist_cases.CHAIN_H))
    assert worst <= ref.bound(K, t) * (1 + hoist_cases.CHAIN_H)
    assert any(v % t for e in C.chain_error_polys(ch, floor) for v in e)


# ---- rescale and product end to end -----------------------------------------------------------------

def _encrypt(rng, n, q, s, m, t):
    """(c_0, c_1) [2, L, n] residues with c_0 + c_1 s = m + t e, |e| <= 1, c_1 uniform."""
    Q = prod(q)
    e = [int(v) for v in rng.integers(-1, 2, size=n)]
    c1 = [int.from_bytes(rng.bytes(32), "little") % Q for _ in range(n)]
    c0 = (np.array([a + t * b for a, b in zip(m, e)], dtype=object)
          - ks_ref.negacyclic(s, c1, Q)) % Q
    return np.array([[[int(v) % ql for v in c] for ql in q] for c in (c0, c1)], dtype=object)


def _decrypt(c, q, s):
    """The centred c_0 + c_1 s mod Q of coefficient-order residues c [2, L, n]: n signed integers."""
    Q = prod(q)
    c0, c1 = (_crt(np.asarray(c[i])[None], q)[0] for i in (0, 1))
    v = (c0 + ks_ref.negacyclic(s, c1, Q)) % Q
    return [int(a) - Q if int(a) > Q // 2 else int(a) for a in v]


@pytest.mark.parametrize("bits", (32, 64))
def test_the_rescale_decrypts_to_the_scaled_message(bits, torch_cuda):
    """K = 1, P = {q_last}: a ciphertext over L + 1 limbs with a seeded message in Z_t and noise
    |e| <= 1 decrypts, after the rescale, to [q_last^-1 m]_t exactly.  Margin: the phase after the
    rescale is below (t + 2 t) / q_last + (1 + (t + 1) / 2)(1 + h) < 2^20 against Q / 2 > 2^60."""
    n, t, L = C.E2E_N, C.E2E_T, 2
    q, p = ks_ref.bases(bits, L, 1)
    rng = np.random.default_rng(bits + 1)
    s = ks_ref.ternary(rng, n, hoist_cases.CHAIN_H)
    m = [int(v) for v in rng.integers(0, t, size=n)]
    ct = _encrypt(rng, n, q + p, s, m, t).astype(_dt(bits))                  # [2, L + 1, n]
    with _ctx(n)(n, q + p) as big, _ctx(n)(n, q) as low, nttmul.NttPlainModDown(n, q, p, t) as tm:
        out = low.inverse(_call(torch_cuda, tm, big.forward(ct)))
        mf = tm.msg_factor
    assert mf == pow(p[0], -1, t)
    phase = _decrypt(out, q, s)
    assert max(abs(v) for v in phase) < 1 << 20 and prod(q) > 1 << 61
    assert [v % t for v in phase] == [mf * a % t for a in m]


@pytest.mark.parametrize("bits", (32, 64))
def test_the_product_decrypts_to_the_scaled_product(bits, torch_cuda):
    """ctmul_high -> ksntt_modup -> ctmul_relin -> tmd_moddown on the merged context
    (q[:L-1], (q_{L-1},) + p), with the zero-noise s^2 -> s key: the result decrypts to
    [msg_factor P m_1 m_2]_t = [q_{L-1}^-1 m_1 m_2]_t, the negacyclic product in
    Z_t[x] / (x^n + 1), exactly.
    Margin: the product's phase is below n (2 t)^2 < 2^43 in absolute value (|m + t e| < 2 t per
    coefficient), against Q / 2 > 2^122 (32-bit words, L = 4) before and Q' / 2 > 2^91 after the
    division, so no reduction modulo Q wraps; after the division by P q_{L-1} the phase is below
    2^43 / 2^31 + (K + 1 + (t + 1) / 2)(1 + h) < 2^20."""
    from ctmul_ref import signed_square
    n, t = C.E2E_N, C.E2E_T
    L, K, alpha = hoist_cases.CHAIN_SHAPE
    q, p = ks_ref.bases(bits, L, K)
    assert L >= 3 and n * (2 * t) ** 2 < 1 << 43 and prod(q[:-1]) > 1 << 92
    rng = np.random.default_rng(bits + 2)
    s = ks_ref.ternary(rng, n, hoist_cases.CHAIN_H)
    key = np.stack([c.astype(_dt(bits))
                    for c in ks_ref.keygen(rng, n, q, p, alpha, s, signed_square(s))])
    m1, m2 = ([int(v) for v in rng.integers(0, t, size=n)] for _ in range(2))
    x = _encrypt(rng, n, q, s, m1, t).astype(_dt(bits))[None, None]          # [1, 1, 2, L, n]
    y = _encrypt(rng, n, q, s, m2, t).astype(_dt(bits))[None, None]
    lo, hi = q[:-1], (q[-1],) + p
    M = L + K
    Ctx = _ctx(n)
    with Ctx(n, q) as cq, Ctx(n, q + p) as big, Ctx(n, lo) as low, \
            nttmul.NttCtMul(n, q, p) as ct, nttmul.NttKeySwitch(n, q, p, alpha) as kn, \
            nttmul.NttPlainModDown(n, lo, hi, t) as tm:
        x_hat = cq.forward(x.reshape(2, L, n)).reshape(x.shape)
        y_hat = cq.forward(y.reshape(2, L, n)).reshape(y.shape)
        key_hat = big.forward(key.reshape(-1, M, n)).reshape(key.shape)
        up_hat = kn.modup(ct.high(x_hat, y_hat))
        mid = ct.relin(up_hat, key_hat, x_hat, y_hat)                        # [1, 2, M, n]
        out = low.inverse(_call(torch_cuda, tm, np.ascontiguousarray(mid.reshape(2, M, n))))
        mf = tm.msg_factor
    assert mf == pow(prod(hi), -1, t)
    phase = _decrypt(out, lo, s)
    assert max(abs(v) for v in phase) < 1 << 20
    want = ks_ref.negacyclic(m1, m2, t)
    # relin's c_hat is P (d_0 + d_1 s + d_2 s^2): the key's gadget and the P (d_0, d_1) term carry
    # the factor P, which the division takes out again, so of msg_factor = (P q_{L-1})^-1 the
    # message sees msg_factor P = q_{L-1}^-1 (a key switch alone sees msg_factor P = 1)
    factor = mf * prod(p) % t
    assert factor == pow(q[-1], -1, t)
    assert [v % t for v in phase] == [factor * int(a) % t for a in want]
