"""GPU tests of the mac against two NTT-domain operands (include/nttmul_macn.h,
lib/libnttmul_macn.so, csrc/macn_dev.hpp k_rns_macn / k_rnsmp_macn).

The header's promise is bit-for-bit equality, per component, with the same context's mac_ntt: that
is the main comparison, at every degree and in both word classes, and it is anchored to the CPU
oracle (sums of products in Python integers) at four degrees and to a closed form on the
worst-case input.  Every output is preset to the sentinel in a guarded arena (tests/guarded.py).
In every test the components' b_hat differ, so a swapped or duplicated component fails.  The
shapes are tests/macn_cases.py's: the smallest at which the kernels can go wrong."""
import numpy as np
import pytest

import bconv_ref as B
import guarded as G
import ks_ref
import macn_cases as C
import nttmul
import rnsmp_cases as M
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


def _ctx(n, moduli, **kw):
    cls = nttmul.RnsMacnContext if C.family(n) == "rns" else nttmul.RnsMpMacnContext
    return cls(n, moduli, **kw)


def _to_dev(torch, x, bits):
    x = np.ascontiguousarray(x, dtype=_dt(bits))
    return torch.from_numpy(x.view(np.int32 if bits == 32 else np.int64).reshape(-1)).cuda()


def _from_dev(t, bits, shape):
    return t.cpu().numpy().view(_dt(bits)).reshape(shape)


def _macn(torch, ctx, a, bh, shared, stream=0):
    """One macn_ntt_device call out of a guarded arena: a [batch, terms, L, n], bh
    [comps, terms, L, n] or [batch, comps, terms, L, n]; returns c [batch, comps, L, n].  After the
    call no guard word and no input has changed and every word of c is written."""
    batch, terms = a.shape[:2]
    comps = bh.shape[-4]
    shape = (batch, comps, ctx.limbs, ctx.n)
    guard = G.guard_words(a.size // batch, bh.size // (1 if shared else batch))
    arena = G.DeviceArena(torch, ctx.word_bits, guard, c=int(np.prod(shape)), a=a, b=bh)
    ctx.macn_ntt_device(arena["c"], arena["a"], arena["b"], batch, terms, comps, shared=shared,
                        stream=stream)
    torch.cuda.synchronize()
    arena.check()
    return arena.get("c", shape)


def _mac(torch, ctx, a, bh, shared):
    """The context's own mac_ntt_device, likewise: bh [terms, L, n] or [batch, terms, L, n]."""
    batch, terms = a.shape[:2]
    shape = (batch, ctx.limbs, ctx.n)
    guard = G.guard_words(a.size // batch, bh.size // (1 if shared else batch))
    arena = G.DeviceArena(torch, ctx.word_bits, guard, c=int(np.prod(shape)), a=a, b=bh)
    ctx.mac_ntt_device(arena["c"], arena["a"], arena["b"], batch, terms, shared=shared)
    torch.cuda.synchronize()
    arena.check()
    return arena.get("c", shape)


def _component(bh, i, shared):
    return np.ascontiguousarray(bh[i] if shared else bh[:, i])


def _operands(case, seed):
    """a and b_hat of a case: seeded canonical words per limb; any canonical vector is a valid
    b_hat.  The components are independent draws."""
    bits, L = C.word_bits(case.moduli), len(case.moduli)
    rng = np.random.default_rng(seed)
    a = B.random_words(rng, case.moduli, case.batch * case.terms, case.n, _dt(bits))
    k = (1 if case.shared else case.batch) * case.comps * case.terms
    bh = B.random_words(rng, case.moduli, k, case.n, _dt(bits))
    a = a.reshape(case.batch, case.terms, L, case.n)
    bh = bh.reshape(((case.comps,) if case.shared else (case.batch, case.comps))
                    + (case.terms, L, case.n))
    if case.comps > 1:
        assert not np.array_equal(_component(bh, 0, case.shared), _component(bh, 1, case.shared))
    return a, bh


def _differ(got, want):
    bad = np.argwhere((got != want).any(axis=-1))
    return f"{len(bad)} rows differ, first {bad[0] if len(bad) else None}"


# ---------------------------------------------------------------------------------------------
# 1. equality with the library's own mac_ntt
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
def test_each_component_equals_mac_ntt(n, moduli, torch_cuda):
    """Every term count and b_hat form of one basis at one degree: component i of macn_ntt
    (comps = 2) equals mac_ntt against b_hat[..][i] bit for bit, and comps = 1 equals mac_ntt."""
    cases = GROUPS[n, moduli]
    assert {c.comps for c in cases} == {1, 2} and {c.shared for c in cases} == {True, False}
    with _ctx(n, moduli) as ctx:
        for case in cases:
            a, bh = _operands(case, 7 * n + 100 * len(moduli) + case.terms)
            got = _macn(torch_cuda, ctx, a, bh, case.shared)
            for i in range(case.comps):
                want = _mac(torch_cuda, ctx, a, _component(bh, i, case.shared), case.shared)
                assert np.array_equal(got[:, i], want), (case, i, _differ(got[:, i], want))
            if case.comps == 2:
                assert not np.array_equal(got[:, 0], got[:, 1])


# ---------------------------------------------------------------------------------------------
# 2. parity with the oracle
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n", C.ORACLE_N)
def test_parity_with_the_oracle(n, bits, torch_cuda):
    """c[p][i][l] = sum over t of the oracle's product a[p][t][l] * b[p or shared][i][t][l] mod
    q_l, summed in Python integers, with b_hat = the context's own forward(b)."""
    T = C.cases_of(n)
    moduli = (T.BASIS32 if bits == 32 else T.BASIS64)[:C.ORACLE_LIMBS]
    batch, terms, L = C.ORACLE_BATCH, C.ORACLE_TERMS, len(moduli)
    plans = [O.Plan(n, q) for q in moduli]
    with _ctx(n, moduli) as ctx:
        for shared in (True, False):
            a, b = _operands(C.Case(n, moduli, batch, terms, 2, shared), n + bits + shared)
            bh = ctx.forward(b.reshape(-1, L, n)).reshape(b.shape)
            got = _macn(torch_cuda, ctx, a, bh, shared)
            for p in range(batch):
                for i in range(2):
                    for l, q in enumerate(moduli):
                        bi = b[i] if shared else b[p, i]
                        acc = sum(plans[l].product_merged(a[p, t, l], bi[t, l]).astype(object)
                                  for t in range(terms))
                        assert np.array_equal(got[p, i, l], (acc % q).astype(_dt(bits))), \
                            (shared, p, i, l)


# ---------------------------------------------------------------------------------------------
# 3. worst-case ranges
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n", C.RANGE_N)
def test_worst_case_ranges(n, bits, torch_cuda):
    """Every word of a is q_l - 1, component 0 of b_hat all q_l - 1, component 1 all q_l - 2, seven
    terms: the largest values both accumulators can hold.  Closed form: a constant vector v in the
    NTT domain is the transform of the constant polynomial v, so component 0 is
    7 (-1)(-(1 + x + .. + x^(n-1))), every coefficient 7, and component 1 every coefficient 14."""
    T = C.cases_of(n)
    moduli = T.BASIS32 if bits == 32 else T.BASIS64
    batch, terms, L = T.RANGE_BATCH, C.RANGE_TERMS, len(moduli)
    top = np.array([q - 1 for q in moduli], dtype=_dt(bits))
    a = np.ascontiguousarray(np.broadcast_to(top[None, None, :, None], (batch, terms, L, n)))
    with _ctx(n, moduli) as ctx:
        for shared in (True, False):
            lead = (2,) if shared else (batch, 2)
            bh = np.ascontiguousarray(np.broadcast_to(top[None, :, None], lead + (terms, L, n)))
            (bh[1] if shared else bh[:, 1])[...] -= 1
            got = _macn(torch_cuda, ctx, a, bh, shared)
            for i in range(2):
                want = _mac(torch_cuda, ctx, a, _component(bh, i, shared), shared)
                assert np.array_equal(got[:, i], want), (shared, i, _differ(got[:, i], want))
                for l, q in enumerate(moduli):
                    assert (got[:, i, l] == (i + 1) * terms % q).all(), (shared, i, l)
        one = _macn(torch_cuda, ctx, a, np.ascontiguousarray(bh[:, :1]), False)   # comps = 1
        assert np.array_equal(one[:, 0], got[:, 0])


# ---------------------------------------------------------------------------------------------
# 4. sub-batches
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,moduli,terms,batch,want_chunks", C.SUBBATCH)
def test_sub_batches_with_one_mib_of_scratch(n, moduli, terms, batch, want_chunks, torch_cuda):
    """scratch_mb = 1: the call runs in the sub-batches the mirror computes (the mirror's rule is
    rnsmp.cpp run's, csrc/subbatch.hpp), at least three, and writes what a context with the
    default scratch writes in one pass; the borders' polynomials also equal mac_ntt."""
    small, whole = _ctx(n, moduli, scratch_mb=1), _ctx(n, moduli)
    assert (small.info.scratch_mb, whole.info.scratch_mb) == (1, M.DEFAULT_SCRATCH_MB)
    for shared in (True, False):
        case = C.Case(n, moduli, batch, terms, 2, shared, False, 1)
        assert C.chunks(case) == list(want_chunks) and len(want_chunks) >= 3
        assert len(C.chunks(case._replace(scratch_mb=0))) == 1
        a, bh = _operands(case, 11 + terms)
        got = _macn(torch_cuda, small, a, bh, shared)
        ref = _macn(torch_cuda, whole, a, bh, shared)
        assert np.array_equal(got, ref), (shared, _differ(got, ref))
        for i in range(2):
            want = _mac(torch_cuda, whole, a, _component(bh, i, shared), shared)
            assert np.array_equal(got[:, i], want), (shared, i)
    small.close()
    whole.close()


# ---------------------------------------------------------------------------------------------
# 5. NTTMUL_FLAG_VALIDATE
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,moduli,limb,above", C.VALIDATE)
def test_validate_flag_checks_a_and_every_component(n, moduli, limb, above, torch_cuda):
    """One word equal to its own limb's modulus (in range for the limb `above`) in a, then in
    component 1 of b_hat: NTTMUL_ERANGE and c keeps the sentinel; a clean call succeeds; without
    the flag there is no check."""
    torch = torch_cuda
    assert moduli[limb] < moduli[above]
    batch, terms, bits = C.VALIDATE_BATCH, C.VALIDATE_TERMS, C.word_bits(moduli)
    case = C.Case(n, moduli, batch, terms, 2, True, True)
    a, bh = _operands(case, 5)
    with _ctx(n, moduli, validate=True) as strict, _ctx(n, moduli) as lax:
        good = _macn(torch, strict, a, bh, True)
        assert np.array_equal(good, _macn(torch, lax, a, bh, True))
        bad_a, bad_b = a.copy(), bh.copy()
        bad_a[batch - 1, terms - 1, limb, n - 1] = moduli[limb]
        bad_b[1, terms - 1, limb, n - 1] = moduli[limb]
        for xa, xb in ((bad_a, bh), (a, bad_b)):
            shape = (batch, 2, len(moduli), n)
            arena = G.DeviceArena(torch, bits, G.guard_words(xa.size // batch, xb.size),
                                  c=int(np.prod(shape)), a=xa, b=xb)
            with pytest.raises(nttmul.NttmulError) as ei:
                strict.macn_ntt_device(arena["c"], arena["a"], arena["b"], batch, terms, 2)
            assert ei.value.status == nttmul.NTTMUL_ERANGE
            torch.cuda.synchronize()
            assert (arena.get("c") == G.sentinel(bits)).all()           # c untouched
            _macn(torch, lax, xa, xb, True)                             # no flag, no check
        ok_a = a.copy()
        ok_a[0, 0, above, 0] = moduli[limb]                             # in range for that limb
        _macn(torch, strict, ok_a, bh, True)


# ---------------------------------------------------------------------------------------------
# 6. host forms
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,moduli", C.HOST)
def test_host_forms_equal_the_device_forms(n, moduli, torch_cuda):
    batch, terms, bits = C.HOST_BATCH, C.HOST_TERMS, C.word_bits(moduli)
    with _ctx(n, moduli) as ctx:
        for shared in (True, False):
            a, bh = _operands(C.Case(n, moduli, batch, terms, 2, shared), 77)
            dev = _macn(torch_cuda, ctx, a, bh, shared)
            host = ctx.macn_ntt(a, bh, shared=shared)
            assert host.dtype == _dt(bits) and host.shape == dev.shape
            assert np.array_equal(host, dev)
            one = ctx.macn_ntt(a, bh[:1] if shared else bh[:, :1], shared=shared)   # comps = 1
            assert np.array_equal(one[:, 0],
                                  ctx.mac_ntt(a, _component(bh, 0, shared), shared=shared))
            assert np.array_equal(one[:, 0], dev[:, 0])
            assert ctx.macn_ntt(a[:0], bh if shared else bh[:0], shared=shared).shape == \
                (0, 2, len(moduli), n)
        with pytest.raises(ValueError):
            ctx.macn_ntt(a, bh[0, 0], shared=True)                      # no component axis
        with pytest.raises(ValueError):
            ctx.macn_ntt(a, bh[:batch - 1], shared=False)               # one batch entry short


# ---------------------------------------------------------------------------------------------
# 7. device path rules
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (256, 8192))
def test_device_path_rules(n, torch_cuda):
    """The refusals on a live context, all before any device access: terms = 0, comps = 0 and 3, a
    NULL operand with batch > 0, a device the context does not have; batch = 0 is a no-op."""
    torch = torch_cuda
    moduli = C.cases_of(n).BASIS32
    EINVAL = nttmul.NTTMUL_EINVAL
    with _ctx(n, moduli) as ctx:
        out = torch.full((2 * len(moduli) * n,), 7, dtype=torch.int32, device="cuda")
        p = out.data_ptr()
        dev, host = ctx._c.macn_ntt_device, ctx._c.macn_ntt
        assert dev(ctx._h, p, p, p, 1, 0, 2, 1, 0, None) == EINVAL       # terms = 0
        assert dev(ctx._h, p, p, p, 1, 1, 0, 1, 0, None) == EINVAL       # comps = 0
        assert dev(ctx._h, p, p, p, 1, 1, 3, 1, 0, None) == EINVAL       # comps > the maximum
        assert dev(ctx._h, p, p, p, 0, 1, 3, 1, 0, None) == EINVAL       # also with batch = 0
        for args in ((None, p, p), (p, None, p), (p, p, None)):
            assert dev(ctx._h, *args, 1, 1, 2, 1, 0, None) == EINVAL
            assert host(ctx._h, *args, 1, 1, 2, 1) == EINVAL
        assert dev(ctx._h, None, None, None, 0, 1, 2, 1, 0, None) == nttmul.NTTMUL_OK
        assert host(ctx._h, None, None, None, 0, 1, 2, 1) == nttmul.NTTMUL_OK
        assert dev(ctx._h, p, p, p, 1, 1, 2, 1, 99, None) == nttmul.NTTMUL_ENODEV
        assert dev(ctx._h, p, p, p, 1, 1, 1, 1, 99, None) == nttmul.NTTMUL_ENODEV
        ctx.macn_ntt_device(out, out, out, 0, 1, 2)                      # batch = 0: a no-op
        torch.cuda.synchronize()
        assert bool((out == 7).all())
        with pytest.raises(ValueError):                                  # too small a tensor
            ctx.macn_ntt_device(out, out, out, 2, 1, 2)
        assert ctx._c.macn_kernel_name(ctx._h, 0, None, 0) == EINVAL
        assert ctx._c.macn_kernel_name(ctx._h, 3, None, 0) == EINVAL
        assert ctx._c.macn_kernel_name(ctx._h, 2, None, 0) == len(C.kernel_name(n, moduli, 2))


# ---------------------------------------------------------------------------------------------
# 8. two streams and a growing scratch
# ---------------------------------------------------------------------------------------------

def test_one_context_serves_two_streams_and_a_growing_scratch(torch_cuda):
    """macn_ntt and mac_ntt in turn on one multi-pass context, alternating between two streams
    with no synchronisation between the calls, every step on inputs of its own and into an output
    preset to the sentinel; the batch is raised in the middle, so the scratch grows after its
    first use.  Every output is compared at the end with what a second context computed call by
    call: the scratch is handed from stream to stream by the context's event."""
    torch = torch_cuda
    n, moduli = C.STREAMS
    bits, L, terms = C.word_bits(moduli), len(moduli), C.STREAMS_TERMS
    ctx, other = _ctx(n, moduli), _ctx(n, moduli)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    sent = G.sentinel(bits)
    steps, k = [], 0
    for rnd, batch in enumerate(C.STREAMS_BATCHES * 2):                  # 2, 5, 2, 5
        a, bh = _operands(C.Case(n, moduli, batch, terms, 2, True), 300 + rnd)
        want2 = _macn(torch, other, a, bh, True)
        for op in ("macn", "mac", "macn"):
            comps = 2 if op == "macn" else 1
            dins = [_to_dev(torch, a, bits), _to_dev(torch, bh if comps == 2 else bh[1], bits)]
            out = torch.full((batch * comps * L * n,), int(sent) - (1 << bits),
                             dtype=dins[0].dtype, device="cuda")
            want = want2 if comps == 2 else want2[:, 1:2]
            steps.append((op, batch, comps, dins, out, want, streams[k % 2]))
            k += 1
    torch.cuda.synchronize()
    for op, batch, comps, dins, out, _, s in steps:                      # no synchronisation here
        if op == "macn":
            ctx.macn_ntt_device(out, dins[0], dins[1], batch, terms, 2, stream=s.cuda_stream)
        else:
            ctx.mac_ntt_device(out, dins[0], dins[1], batch, terms, shared=True,
                               stream=s.cuda_stream)
    torch.cuda.synchronize()
    for i, (op, batch, comps, _, out, want, _) in enumerate(steps):
        got = _from_dev(out, bits, (batch, comps, L, n))
        assert not (got == sent).any(), (i, op)
        assert np.array_equal(got, want), (i, op, batch, _differ(got, want))
    ctx.close()
    other.close()


# ---------------------------------------------------------------------------------------------
# 9. the three-launch key switch
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n,kind", C.CHAIN)
def test_three_launch_key_switch(n, kind, bits, torch_cuda):
    """modup, one macn_ntt (comps = 2, shared) and one moddown over batch * 2, against the chain of
    tests/test_gpu_ks.py (one mac_ntt and one moddown per key component) on the same inputs: bit
    for bit the same (c0, c1), and the same +-(K + 1)(1 + h) key-switch identity."""
    torch = torch_cuda
    L, K, alpha = C.CHAIN_SHAPE
    batch, h = C.CHAIN_BATCH, C.CHAIN_H
    q, p = ks_ref.bases(bits, L, K)
    ext, Mx, dn = q + p, L + K, -(-L // alpha)
    assert C.family(n) == kind
    rng = np.random.default_rng(n + bits)
    s, s2 = ks_ref.ternary(rng, n, h), ks_ref.ternary(rng, n, h)
    key = np.stack([k.astype(_dt(bits)) for k in ks_ref.keygen(rng, n, q, p, alpha, s, s2)])
    assert not np.array_equal(key[0], key[1])                    # (b, a): [2][dnum][L + K][n]
    x = B.random_words(rng, q, batch, n, _dt(bits))
    tdt = torch.int32 if bits == 32 else torch.int64
    sentinel = int(G.sentinel(bits)) - (1 << bits)
    full = lambda words: torch.full((words,), sentinel, dtype=tdt, device="cuda")   # noqa: E731
    with nttmul.KeySwitchBasis(n, q, p, alpha) as ks, _ctx(n, ext) as mac:
        assert ks.digits == dn
        st = torch.cuda.current_stream().cuda_stream
        dx, dkey = _to_dev(torch, x, bits), _to_dev(torch, key, bits)
        dhat = full(2 * dn * Mx * n)
        mac.forward_device(dhat, dkey, 2 * dn, stream=st)                # key_hat, once
        up = full(batch * dn * Mx * n)
        # three launches (five above n = 4096)
        mid, out = full(batch * 2 * Mx * n), full(batch * 2 * L * n)
        ks.modup_device(up, dx, batch, stream=st)
        mac.macn_ntt_device(mid, up, dhat, batch, dn, 2, shared=True, stream=st)
        ks.moddown_device(out, mid, batch * 2, stream=st)
        # the existing chain: five launches (nine)
        mid1 = [full(batch * Mx * n) for _ in range(2)]
        out1 = [full(batch * L * n) for _ in range(2)]
        hat = dhat.view(2, dn * Mx * n)
        for i in range(2):
            mac.mac_ntt_device(mid1[i], up, hat[i], batch, dn, shared=True, stream=st)
            ks.moddown_device(out1[i], mid1[i], batch, stream=st)
        torch.cuda.synchronize()
        got_mid = _from_dev(mid, bits, (batch, 2, Mx, n))
        got = _from_dev(out, bits, (batch, 2, L, n))
        for i in range(2):
            assert np.array_equal(got_mid[:, i], _from_dev(mid1[i], bits, (batch, Mx, n))), i
            assert np.array_equal(got[:, i], _from_dev(out1[i], bits, (batch, L, n))), i
        assert not (got == G.sentinel(bits)).any()
    bound = (K + 1) * (1 + h)
    for b in range(batch):
        err = ks_ref.key_switch_error(x[b], got[b, 0], got[b, 1], q, s, s2)
        assert err <= bound, (b, err, bound)


# ---------------------------------------------------------------------------------------------
# 10. dispatch anchor
# ---------------------------------------------------------------------------------------------

def test_mirror_names_the_kernels_the_library_names(torch_cuda):
    """nttmul_*_macn_kernel_name (the dry run of the launching statements) equals the mirror for
    every (n, class) and comps, and names kernels of the loaded code object."""
    table = nttmul.kernel_hashes(nttmul.MACN_LIB_PATH)
    for n in C.ALL_N:
        T = C.cases_of(n)
        for moduli in (T.BASIS32, T.BASIS64):
            with _ctx(n, moduli) as ctx:
                for comps in (1, 2):
                    name = ctx.macn_kernel_name(comps)
                    assert name == C.kernel_name(n, moduli, comps), (n, comps)
                    assert all(k in table for k in name.split(" + ")), name
                assert ctx.macn_kernel_name(1) == ctx.kernel_name("mac")
    launched = {k for case in C.all_cases() for k in C.kernels_of(case)}
    assert launched <= set(table)
