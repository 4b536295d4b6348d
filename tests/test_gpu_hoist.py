"""GPU tests of the hoisted rotations (include/nttmul_hoist.h, lib/libnttmul_hoist.so,
csrc/hoist_dev.hpp k_rns_hoist / k_rnsmp_hoist).

The header's promise is bit-for-bit equality with the library's own kernels: result (r, i) of
hoist_ntt(forward(a), b_hat, k) is mac_ntt(galois_coeff(a, k_r), b_hat[r][i]).  That is the main
comparison, at every degree and in both word classes; it is anchored to Python integers
(tests/hoist_ref.py) at four degrees, to a closed form on the worst-case input, and to the
key-switch identity end to end.  Every output is preset to the sentinel in a guarded arena
(tests/guarded.py).  In every test the rotations' and components' b_hat are independent draws, so a
swapped rotation or component fails.  The shapes are tests/hoist_cases.py's: the smallest at which
the kernels can go wrong."""
import numpy as np
import pytest

import bconv_ref as B
import guarded as G
import hoist_cases as C
import hoist_ref as H
import nttmul
import rnsmp_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _ctx(n, moduli, **kw):
    cls = nttmul.RnsHoistContext if C.family(n) == "rns" else nttmul.RnsMpHoistContext
    return cls(n, moduli, **kw)


def _to_dev(torch, x, bits):
    x = np.ascontiguousarray(x, dtype=_dt(bits))
    return torch.from_numpy(x.view(np.int32 if bits == 32 else np.int64).reshape(-1)).cuda()


def _from_dev(t, bits, shape):
    return t.cpu().numpy().view(_dt(bits)).reshape(shape)


def _hoist(torch, ctx, a_hat, bh, ks):
    """One hoist_ntt_device call out of a guarded arena: a_hat [batch, terms, L, n], bh
    [rots, comps, terms, L, n]; returns c [batch, rots, comps, L, n].  After the call no guard word
    and no input has changed and every word of c is written."""
    batch, terms = a_hat.shape[:2]
    rots, comps = bh.shape[:2]
    assert rots == len(ks)
    shape = (batch, rots, comps, ctx.limbs, ctx.n)
    guard = G.guard_words(a_hat.size // batch, int(np.prod(shape[1:])))
    arena = G.DeviceArena(torch, ctx.word_bits, guard, c=int(np.prod(shape)), a=a_hat, b=bh)
    ctx.hoist_ntt_device(arena["c"], arena["a"], arena["b"], ks, batch, terms, comps)
    torch.cuda.synchronize()
    arena.check()
    return arena.get("c", shape)


def _operands(case, seed):
    """a (coefficients) and b_hat of a case: seeded canonical words per limb; any canonical vector
    is a valid b_hat.  The rotations and components are independent draws."""
    bits, L = C.word_bits(case.moduli), len(case.moduli)
    rots = len(case.ks)
    rng = np.random.default_rng(seed)
    a = B.random_words(rng, case.moduli, case.batch * case.terms, case.n, _dt(bits))
    bh = B.random_words(rng, case.moduli, rots * case.comps * case.terms, case.n, _dt(bits))
    return (a.reshape(case.batch, case.terms, L, case.n),
            bh.reshape(rots, case.comps, case.terms, L, case.n))


def _differ(got, want):
    bad = np.argwhere((got != want).any(axis=-1))
    return f"{len(bad)} rows differ, first {bad[0] if len(bad) else None}"


def _all_differ(got):
    """No two (rotation, component) results of a call are equal."""
    flat = got.reshape(got.shape[0], -1, *got.shape[3:])
    return all(not np.array_equal(flat[:, i], flat[:, j])
               for i in range(flat.shape[1]) for j in range(i))


# ---------------------------------------------------------------------------------------------
# 1. equality with the library's own kernels
# ---------------------------------------------------------------------------------------------

def _groups():
    out = {}
    for case in C.equality_cases():
        out.setdefault((case.n, case.moduli), []).append(case)
    return out


GROUPS = _groups()


@pytest.mark.parametrize("n,moduli", sorted(GROUPS),
                         ids=lambda v: str(v) if isinstance(v, int) else
                         f"u{C.word_bits(v)}x{len(v)}")
def test_each_result_equals_mac_ntt_of_the_rotated_polynomial(n, moduli, torch_cuda):
    """Every term count of one basis at one degree, comps 1 and 2 with one and three rotations:
    hoist_ntt(forward(a), b_hat, k)[:, r, i] == mac_ntt(galois_coeff(a, k_r), b_hat[r][i]) bit for
    bit, all on the library's own kernels."""
    cases = GROUPS[n, moduli]
    assert {(c.comps, len(c.ks)) for c in cases} == {(1, 1), (1, 3), (2, 1), (2, 3)}
    L = len(moduli)
    with _ctx(n, moduli) as ctx, nttmul.GaloisContext(n, moduli) as gal:
        done = {}
        for case in cases:
            key = case.terms
            if key not in done:                      # one a and its transform per term count
                a, _ = _operands(case, 7 * n + 100 * L + case.terms)
                done[key] = (a, ctx.forward(a.reshape(-1, L, n)).reshape(a.shape), {})
            a, a_hat, rotated = done[key]
            _, bh = _operands(case, 11 * n + 100 * L + case.terms + case.comps)
            got = _hoist(torch_cuda, ctx, a_hat, bh, case.ks)
            for r, k in enumerate(case.ks):
                if k not in rotated:
                    rotated[k] = gal.coeff(a.reshape(-1, L, n), k).reshape(a.shape)
                for i in range(case.comps):
                    want = ctx.mac_ntt(rotated[k], np.ascontiguousarray(bh[r, i]), shared=True)
                    assert np.array_equal(got[:, r, i], want), \
                        (case, r, i, _differ(got[:, r, i], want))
            assert _all_differ(got), case


# ---------------------------------------------------------------------------------------------
# 2. against Python integers
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n", C.ORACLE_N)
def test_against_python_integers(n, bits, torch_cuda):
    """tests/hoist_ref.py hoist: the NTT-order table of tests/galois_ref.py, exact products and
    sums, the oracle's inverse transform; the rotation list holds k = 2n - 1."""
    T = C.cases_of(n)
    moduli = (T.BASIS32 if bits == 32 else T.BASIS64)[:C.ORACLE_LIMBS]
    case = C.Case(n, moduli, C.ORACLE_BATCH, C.ORACLE_TERMS, 2, (5, 2 * n - 1))
    assert case in C.all_cases()
    a_hat, bh = _operands(case, n + bits)            # any canonical vectors
    with _ctx(n, moduli) as ctx:
        got = _hoist(torch_cuda, ctx, a_hat, bh, case.ks)
    want = H.hoist(a_hat, bh, case.ks, moduli)
    assert np.array_equal(got, want), _differ(got, want)
    assert _all_differ(got)


# ---------------------------------------------------------------------------------------------
# 3. worst-case words
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n", C.RANGE_N)
def test_worst_case_words(n, bits, torch_cuda):
    """Every word of a_hat and of b_hat is q_l - 1, seven terms: the largest values the
    accumulators can hold.  A permutation of a constant vector is that vector, so every slot's sum
    of products is 7 (q_l - 1)^2 mod q_l = 7, and every result is, bit for bit, the library's own
    inverse of that constant vector."""
    T = C.cases_of(n)
    moduli = T.BASIS32 if bits == 32 else T.BASIS64
    batch, terms, L = T.RANGE_BATCH, C.RANGE_TERMS, len(moduli)
    ks = (2 * n - 1, 5)
    assert C.Case(n, moduli, batch, terms, 2, ks) in C.all_cases()
    top = np.array([q - 1 for q in moduli], dtype=_dt(bits))
    a_hat = np.ascontiguousarray(np.broadcast_to(top[None, None, :, None], (batch, terms, L, n)))
    bh = np.ascontiguousarray(np.broadcast_to(top[None, None, None, :, None],
                                              (2, 2, terms, L, n)))
    const = np.empty((1, L, n), dtype=_dt(bits))
    for l, q in enumerate(moduli):
        const[0, l] = terms * (q - 1) ** 2 % q
        assert const[0, l, 0] == terms
    with _ctx(n, moduli) as ctx:
        got = _hoist(torch_cuda, ctx, a_hat, bh, ks)
        want = ctx.inverse(const)[0]
        one = _hoist(torch_cuda, ctx, a_hat, np.ascontiguousarray(bh[:1, :1]), ks[:1])
    for p in range(batch):
        for r in range(2):
            for i in range(2):
                assert np.array_equal(got[p, r, i], want), (p, r, i)
    assert np.array_equal(one[:, 0, 0], got[:, 0, 0])


# ---------------------------------------------------------------------------------------------
# 4. NTTMUL_FLAG_VALIDATE, host forms, sub-batches, device path rules
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,moduli,limb,above", C.VALIDATE)
def test_validate_flag_checks_a_hat_and_all_of_b_hat(n, moduli, limb, above, torch_cuda):
    """One word equal to its own limb's modulus (in range for the limb `above`) in a_hat, then in
    the last rotation's last component of b_hat: NTTMUL_ERANGE and c keeps the sentinel; a clean
    call succeeds; without the flag there is no check."""
    torch = torch_cuda
    assert moduli[limb] < moduli[above]
    batch, terms, bits = C.VALIDATE_BATCH, C.VALIDATE_TERMS, C.word_bits(moduli)
    case = C.Case(n, moduli, batch, terms, 2, C.draw(n, 2, 3), True)
    assert case in C.all_cases()
    a, bh = _operands(case, 5)
    with _ctx(n, moduli, validate=True) as strict, _ctx(n, moduli) as lax:
        good = _hoist(torch, strict, a, bh, case.ks)
        assert np.array_equal(good, _hoist(torch, lax, a, bh, case.ks))
        bad_a, bad_b = a.copy(), bh.copy()
        bad_a[batch - 1, terms - 1, limb, n - 1] = moduli[limb]
        bad_b[1, 1, terms - 1, limb, n - 1] = moduli[limb]
        for xa, xb in ((bad_a, bh), (a, bad_b)):
            shape = (batch, 2, 2, len(moduli), n)
            arena = G.DeviceArena(torch, bits, G.guard_words(xa.size // batch, xb.size),
                                  c=int(np.prod(shape)), a=xa, b=xb)
            with pytest.raises(nttmul.NttmulError) as ei:
                strict.hoist_ntt_device(arena["c"], arena["a"], arena["b"], case.ks, batch, terms,
                                        2)
            assert ei.value.status == nttmul.NTTMUL_ERANGE
            torch.cuda.synchronize()
            assert (arena.get("c") == G.sentinel(bits)).all()           # c untouched
            _hoist(torch, lax, xa, xb, case.ks)                         # no flag, no check
        ok_a = a.copy()
        ok_a[0, 0, above, 0] = moduli[limb]                             # in range for that limb
        _hoist(torch, strict, ok_a, bh, case.ks)


@pytest.mark.parametrize("n,moduli", C.HOST)
def test_host_forms_equal_the_device_forms(n, moduli, torch_cuda):
    batch, terms, bits = C.HOST_BATCH, C.HOST_TERMS, C.word_bits(moduli)
    ks = C.draw(n, 3, 1)
    with _ctx(n, moduli) as ctx:
        for comps in (1, 2):
            case = C.Case(n, moduli, batch, terms, comps, ks)
            assert case in C.all_cases()
            a, bh = _operands(case, 77 + comps)
            dev = _hoist(torch_cuda, ctx, a, bh, ks)
            host = ctx.hoist_ntt(a, bh, ks)
            assert host.dtype == _dt(bits) and host.shape == dev.shape
            assert np.array_equal(host, dev)
            assert ctx.hoist_ntt(a[:0], bh, ks).shape == (0, 3, comps, len(moduli), n)
        with pytest.raises(ValueError):
            ctx.hoist_ntt(a, bh[0], ks)                                 # no rotation axis
        with pytest.raises(ValueError):
            ctx.hoist_ntt(a, bh, ks[:2])                                # one rotation short


@pytest.mark.parametrize("n,moduli,batch,terms,comps,rots,want_chunks", C.SUBBATCH)
def test_sub_batches_with_one_mib_of_scratch(n, moduli, batch, terms, comps, rots, want_chunks,
                                             torch_cuda):
    """scratch_mb = 1: the call runs in the sub-batches of output units the mirror computes (the
    mirror's rule is csrc/subbatch.hpp mp_unit_chunk), at least three, their borders inside a batch
    entry or one unit above the limit, and writes what a context with the default scratch writes
    in one pass, which equals the Python integers."""
    case = C.Case(n, moduli, batch, terms, comps, C.draw(n, rots, 2), False, 1)
    assert case in C.subbatch_cases()
    assert C.chunks(case) == list(want_chunks) and len(want_chunks) >= 3
    assert len(C.chunks(case._replace(scratch_mb=0))) == 1
    a, bh = _operands(case, 11 + terms)
    with _ctx(n, moduli, scratch_mb=1) as small, _ctx(n, moduli) as whole:
        assert (small.info.scratch_mb, whole.info.scratch_mb) == (1, M.DEFAULT_SCRATCH_MB)
        got = _hoist(torch_cuda, small, a, bh, case.ks)
        ref = _hoist(torch_cuda, whole, a, bh, case.ks)
    assert np.array_equal(got, ref), _differ(got, ref)
    want = H.hoist(a[-1:], bh, case.ks, moduli)                         # the last sub-batches
    assert np.array_equal(got[-1:], want)
    assert _all_differ(got)


@pytest.mark.parametrize("n", (256, 8192))
def test_device_path_rules(n, torch_cuda):
    """The refusals on a live context, all before any device access and in the header's order:
    terms = 0, comps = 0 and 3, rots = 0 and 17, a NULL k, an even k, k = 0, k >= 2n, a NULL
    operand with batch > 0, a device the context does not have; batch = 0 is a no-op."""
    import ctypes
    torch = torch_cuda
    moduli = C.cases_of(n).BASIS32
    EINVAL, OK = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_OK
    karr = lambda *ks: (ctypes.c_uint32 * len(ks))(*ks)                  # noqa: E731
    with _ctx(n, moduli) as ctx:
        out = torch.full((2 * len(moduli) * n,), 7, dtype=torch.int32, device="cuda")
        p = out.data_ptr()
        dev, host = ctx._c.hoist_ntt_device, ctx._c.hoist_ntt
        good = karr(5)
        assert dev(ctx._h, p, p, p, good, 1, 1, 0, 2, 0, None) == EINVAL     # terms = 0
        assert dev(ctx._h, p, p, p, good, 1, 1, 1, 0, 0, None) == EINVAL     # comps = 0
        assert dev(ctx._h, p, p, p, good, 1, 1, 1, 3, 0, None) == EINVAL     # comps > the maximum
        assert dev(ctx._h, p, p, p, good, 0, 1, 1, 2, 0, None) == EINVAL     # rots = 0
        assert dev(ctx._h, p, p, p, karr(*[1] * 17), 17, 1, 1, 2, 0, None) == EINVAL
        assert dev(ctx._h, p, p, p, None, 1, 1, 1, 2, 0, None) == EINVAL     # a NULL k
        for bad in (0, 4, 2 * n, 2 * n + 1):
            assert dev(ctx._h, p, p, p, karr(5, bad), 2, 1, 1, 1, 0, None) == EINVAL
            assert dev(ctx._h, None, None, None, karr(bad), 1, 0, 1, 1, 0, None) == EINVAL
            assert host(ctx._h, p, p, p, karr(bad), 1, 1, 1, 1) == EINVAL
        for args in ((None, p, p), (p, None, p), (p, p, None)):
            assert dev(ctx._h, *args, good, 1, 1, 1, 2, 0, None) == EINVAL
            assert host(ctx._h, *args, good, 1, 1, 1, 2) == EINVAL
        assert dev(ctx._h, None, None, None, good, 1, 0, 1, 2, 0, None) == OK
        assert host(ctx._h, None, None, None, good, 1, 0, 1, 2) == OK
        assert dev(ctx._h, p, p, p, good, 1, 1, 1, 2, 99, None) == nttmul.NTTMUL_ENODEV
        assert dev(ctx._h, p, p, p, karr(4), 1, 1, 1, 2, 99, None) == EINVAL   # k before the device
        ctx.hoist_ntt_device(out, out, out, (5,), 0, 1, 2)                   # batch = 0: a no-op
        torch.cuda.synchronize()
        assert bool((out == 7).all())
        with pytest.raises(ValueError):                                      # too small a tensor
            ctx.hoist_ntt_device(out, out, out, (5,), 2, 1, 2)
        assert ctx._c.hoist_kernel_name(ctx._h, 0, None, 0) == EINVAL
        assert ctx._c.hoist_kernel_name(ctx._h, 3, None, 0) == EINVAL
        assert ctx._c.hoist_kernel_name(ctx._h, 2, None, 0) == len(C.kernel_name(n, moduli, 2))


# ---------------------------------------------------------------------------------------------
# 5. the hoisted key switch, end to end
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,kind", C.CHAIN)
def test_hoisted_key_switch(n, kind, bits, torch_cuda):
    """modup, forward over batch * dnum, one hoist_ntt (comps = 2, three rotations) and one moddown
    over batch * rots * 2 on device-resident data: every stage equals tests/hoist_ref.py's chain in
    Python integers bit for bit, and the result satisfies c_0 + c_1 s - sigma_k(x) sigma_k(s2)
    within +-(K + 1)(1 + h) for zero-noise keys that switch sigma_k(s2) to s."""
    torch = torch_cuda
    L, K, alpha = C.CHAIN_SHAPE
    batch, rots = C.CHAIN_BATCH, C.CHAIN_ROTS
    assert C.family(n) == kind
    ch = H.chain(n, bits)
    q, p, ks = ch["q"], ch["p"], ch["ks"]
    ext, Mx, dn = q + p, L + K, -(-L // alpha)
    tdt = torch.int32 if bits == 32 else torch.int64
    sentinel = int(G.sentinel(bits)) - (1 << bits)
    full = lambda words: torch.full((words,), sentinel, dtype=tdt, device="cuda")   # noqa: E731
    with nttmul.KeySwitchBasis(n, q, p, alpha) as ksb, _ctx(n, ext) as ctx:
        assert ksb.digits == dn
        assert C.Case(n, ext, batch, dn, 2, ks) in C.all_cases()
        st = torch.cuda.current_stream().cuda_stream
        dx, dkey = _to_dev(torch, ch["x"], bits), _to_dev(torch, ch["key"], bits)
        key_hat = full(rots * 2 * dn * Mx * n)
        ctx.forward_device(key_hat, dkey, rots * 2 * dn, stream=st)      # the keys, once
        up, up_hat = full(batch * dn * Mx * n), full(batch * dn * Mx * n)
        mid, out = full(batch * rots * 2 * Mx * n), full(batch * rots * 2 * L * n)
        ksb.modup_device(up, dx, batch, stream=st)
        ctx.forward_device(up_hat, up, batch * dn, stream=st)
        ctx.hoist_ntt_device(mid, up_hat, key_hat, ks, batch, dn, 2, stream=st)
        ksb.moddown_device(out, mid, batch * rots * 2, stream=st)
        torch.cuda.synchronize()
        got = {"up": _from_dev(up, bits, ch["up"].shape),
               "up_hat": _from_dev(up_hat, bits, ch["up_hat"].shape),
               "key_hat": _from_dev(key_hat, bits, ch["key_hat"].shape),
               "mid": _from_dev(mid, bits, ch["mid"].shape),
               "out": _from_dev(out, bits, ch["out"].shape)}
    for stage in ("up", "up_hat", "key_hat", "mid", "out"):
        assert np.array_equal(got[stage], ch[stage]), (stage, _differ(got[stage], ch[stage]))
    assert not (got["out"] == G.sentinel(bits)).any()
    errs = H.chain_errors(ch, got["out"])
    assert max(errs) <= H.chain_bound(), errs


# ---------------------------------------------------------------------------------------------
# 6. dispatch anchor
# ---------------------------------------------------------------------------------------------

def test_mirror_names_the_kernels_the_library_names(torch_cuda):
    """nttmul_*_hoist_kernel_name (the dry run of the launching statements) equals the mirror for
    every (n, class) and comps, and names kernels of the loaded code object."""
    table = nttmul.kernel_hashes(nttmul.HOIST_LIB_PATH)
    for n in C.ALL_N:
        T = C.cases_of(n)
        for moduli in (T.BASIS32, T.BASIS64):
            with _ctx(n, moduli) as ctx:
                for comps in (1, 2):
                    name = ctx.hoist_kernel_name(comps)
                    assert name == C.kernel_name(n, moduli, comps), (n, comps)
                    assert all(k in table for k in name.split(" + ")), name
                assert ctx.macn_kernel_name(1) == ctx.kernel_name("mac")
    launched = {k for case in C.all_cases() for k in C.kernels_of(case)}
    assert launched <= set(table)
