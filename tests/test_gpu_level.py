"""The view calls of include/nttmul_level.h on the GPU, in both word classes, at n = 256 (one
256-slot slice per polynomial), 512 and 8192, on a chain of L_top = 5, K = 2, alpha = 2 from
tests/basis_cases.py (mixed, unsorted limb sizes) and the levels 5 (the identity view), 4, 3 (a
partial last digit) and 1 (tests/level_cases.py).

Every view call is compared bit for bit with the dense call of the same context on
tests/level_ref.gather of the top-level operand, made on the device; and, on every output word
at every n, with the CPU reference of the dense call (tests/full_ref.py), which shares no code with
the device.  A second test sets every word outside the
view to all ones, out of range for every modulus: the output must not change and
NTTMUL_FLAG_VALIDATE must pass, and one word inside the view out of range must be NTTMUL_ERANGE
with the output untouched.  A third runs the chain end to end on zero-noise keys made once for the
five-limb chain and used at level 3."""
import ctypes

import numpy as np
import pytest

import bconv_ref as B
import full_ref as F
import galois_ref
import hoist_ref as H
import ks_ref
import level_cases as C
import level_gpu as G
import level_ref as LR
import nttmul

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _reference(case, ops, key, w):
    """The CPU reference of the dense call on host copies (tests/full_ref.py)."""
    bits = case.bits
    q, p = C.level_bases(bits, case.L)
    a, key = G.host(ops["a"], bits), G.host(key, bits)
    if case.op == "mac":
        return F.reference("level", "mac", a, key, ops["ks"], q + p)
    if case.op == "lintrans":
        return F.reference("level", "lintrans", a, key, ops["ks"], q, p,
                           None if w is None else G.host(w, bits),
                           None if ops["c0"] is None else G.host(ops["c0"], bits))
    return F.reference("level", "relin", a, key, G.host(ops["x"], bits), G.host(ops["y"], bits),
                       q, p)


def _groups():
    """The parity cases by (op, bits, n, L): one context per test."""
    groups = {}
    for c in C.parity_cases():
        groups.setdefault((c.op, c.bits, c.n, c.L), []).append(c)
    return [pytest.param(v, id=f"{k[0]}-u{k[1]}-n{k[2]}-L{k[3]}") for k, v in groups.items()]


@pytest.mark.parametrize("cases", _groups())
def test_view_equals_the_dense_call_on_the_gathered_operand(cases, torch_cuda):
    torch = torch_cuda
    first = cases[0]
    logn = first.n.bit_length() - 1
    with G.context(first) as ctx:
        assert ctx._lib is nttmul.load_level_library()
        assert (ctx.q_limbs, ctx.p_limbs) == (first.L, C.K)
        for case in cases:
            # the mirror's name is the library's own dry run
            assert C.kernel_name(case) == nttmul.level_kernel_name(
                case.op, logn, case.bits, case.comps, case.weighted)
            ops = G.operands(torch, case)
            key, w = G.gathered(case, ops)
            kept = ops["key"].clone(), None if ops.get("w") is None else ops["w"].clone()
            got = G.call(torch, ctx, case, ops, C.VIEW)
            want = G.call(torch, ctx, case, ops, None, key=key, w=w)
            assert torch.equal(got, want), G.case_id(case)
            assert not bool((got == -1).any()), G.case_id(case)
            assert torch.equal(ops["key"], kept[0])
            assert kept[1] is None or torch.equal(ops["w"], kept[1])
            if case.L == C.L_TOP:
                # the identity view: the gathered operand is the operand
                assert torch.equal(key, ops["key"])
            F.assert_equal(G.host(got, case.bits), _reference(case, ops, key, w),
                           G.case_id(case))


@pytest.mark.parametrize("case", C.validate_cases(), ids=G.case_id)
def test_words_outside_the_view_are_neither_read_nor_checked(case, torch_cuda):
    torch = torch_cuda
    ops = G.operands(torch, case, seed=7)
    terms = ops["terms"]
    with G.context(case, validate=True) as ctx:
        clean = G.call(torch, ctx, case, ops, C.VIEW)
        F.assert_equal(G.host(clean, case.bits), _reference(case, ops, *G.gathered(case, ops)),
                       G.case_id(case))
        # every word outside the view all ones
        poisoned = dict(ops)
        sel = torch.from_numpy(LR.selected(tuple(ops["key"].shape), C.VIEW, case.L, terms)).cuda()
        assert 0 < int(sel.sum()) < sel.numel()
        poisoned["key"] = torch.where(sel, ops["key"], torch.full_like(ops["key"], -1))
        if ops.get("w") is not None:
            wsel = torch.from_numpy(LR.selected(tuple(ops["w"].shape), C.VIEW, case.L, None)).cuda()
            assert 0 < int(wsel.sum()) < wsel.numel()
            poisoned["w"] = torch.where(wsel, ops["w"], torch.full_like(ops["w"], -1))
        got = G.call(torch, ctx, case, poisoned, C.VIEW)            # NTTMUL_FLAG_VALIDATE passes
        assert torch.equal(got, clean), G.case_id(case)
        # the dense call on the gathered poisoned operand sees no poison either
        key, w = G.gathered(case, poisoned)
        assert torch.equal(G.call(torch, ctx, case, poisoned, None, key=key, w=w), clean)
        # one word inside the view out of range: the last selected word, then the first
        targets = [("key", sel)] + ([("w", wsel)] if ops.get("w") is not None else [])
        for name, mask in targets:
            flat = torch.nonzero(mask.reshape(-1)).reshape(-1)
            for at in (int(flat[-1]), int(flat[0])):
                bad = dict(poisoned)
                bad[name] = poisoned[name].clone()
                bad[name].view(-1)[at] = -1
                out = torch.full(G.out_shape(case), -1, dtype=G.tdt(torch, case.bits),
                                 device="cuda")
                with pytest.raises(nttmul.NttmulError) as ei:
                    G.call(torch, ctx, case, bad, C.VIEW, out=out)
                assert ei.value.status == nttmul.NTTMUL_ERANGE
                torch.cuda.synchronize()
                assert bool((out == -1).all()), "NTTMUL_ERANGE must leave the output untouched"


@pytest.mark.parametrize("bits", (32, 64))
def test_view_statuses_on_a_context_come_before_any_device_access(bits, torch_cuda):
    """The dense call's statuses, then the view's, then batch = 0 and the device: every refusal
    of the view is NTTMUL_EINVAL also where the device is not the context's or batch is 0."""
    torch = torch_cuda
    lib = nttmul.load_level_library()
    EINVAL, ENODEV, OK = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_ENODEV, nttmul.NTTMUL_OK
    L, n = 4, 256
    case = C.Case("mac", bits, n, 1, L, 1, 1)
    ops = G.operands(torch, case)
    out = torch.full(G.out_shape(case), -1, dtype=G.tdt(torch, bits), device="cuda")
    k = (ctypes.c_uint32 * 1)(*ops["ks"])
    V = nttmul.LevelView
    bad_views = (None, V(L - 1, 3), V(nttmul.RNS_MAX_LIMBS - C.K + 1, 3), V(5, 1))
    q, p = C.level_bases(bits, L)
    with nttmul.NttLevelKeySwitch(n, q, p, 2) as kn, nttmul.NttLevelLinTrans(n, q, p) as lt, \
            nttmul.NttLevelCtMul(n, q, p) as ct:
        a, key, c = ops["a"].data_ptr(), ops["key"].data_ptr(), out.data_ptr()

        def calls(view, batch, dev):
            v = None if view is None else ctypes.byref(view)
            return (lib.nttmul_ksntt_mac_view_device(kn._h, c, a, key, k, 1, batch, 2, 1, v, dev,
                                                     None),
                    lib.nttmul_lintrans_apply_view_device(lt._h, c, a, key, None, None, k, 1,
                                                          batch, 2, 1, v, dev, None),
                    lib.nttmul_ctmul_relin_view_device(ct._h, c, a, key, a, a, batch, 1, 2, v,
                                                       dev, None))
        for view in bad_views:
            for batch in (1, 0):
                for dev in (0, 99):
                    assert calls(view, batch, dev) == (EINVAL,) * 3
        good = V(*C.VIEW)
        assert calls(good, 0, 0) == (OK,) * 3
        assert calls(good, 1, 99) == (ENODEV,) * 3
        assert calls(V(nttmul.RNS_MAX_LIMBS - C.K, 3), 0, 0) == (OK,) * 3    # the widest operand
        assert calls(V(L, 2), 0, 0) == (OK,) * 3                             # the identity
        torch.cuda.synchronize()
        assert bool((out == -1).all())


def _addmod(torch, x, y, m):
    s = x.to(torch.int64) + y.to(torch.int64)
    return torch.where(s >= m, s - m, s).to(x.dtype)


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("n", C.CHAIN_N)
def test_chain_at_level_3_on_keys_made_once_for_the_five_limb_chain(n, bits, torch_cuda):
    """Zero-noise keys for three rotations, made once over the five-limb chain (ks_ref.keygen on
    hoist_ref.rotate_signed secrets, as hoist_ref.chain makes them).  At level 3: ksntt_modup ->
    mac_view -> mdntt_moddown returns, per rotation, c_0 + c_1 s - sigma_k(x) sigma_k(s') within
    +-(K + 1)(1 + h), ModDown's rounding alone; apply_view at R = 3 is the sum of the rotations bit
    for bit in Q u P and decrypts to the sum within the same bound."""
    torch = torch_cuda
    dt = np.uint32 if bits == 32 else np.uint64
    L, h, batch = C.CHAIN_LEVEL, C.CHAIN_H, 1
    q_top, p = C.chain_bases(bits)
    q, ext_top = q_top[:L], q_top + p
    ks = C.ks_of(n, 3)
    rng = np.random.default_rng(n + bits)
    s, s2 = ks_ref.ternary(rng, n, h), ks_ref.ternary(rng, n, h)
    key = np.stack([np.stack([c.astype(dt) for c in
                              ks_ref.keygen(rng, n, q_top, p, C.ALPHA, s, H.rotate_signed(s2, k))])
                    for k in ks])
    assert key.shape == (3, 2, C.TOP_TERMS, C.L_TOP + C.K, n)
    x = B.random_words(rng, q, batch, n, dt)
    low_cls = nttmul.RnsHoistContext if n <= 4096 else nttmul.RnsMpHoistContext
    with low_cls(n, ext_top) as top:                                # the keys' transforms, once
        key_hat = top.forward(key.reshape(-1, len(ext_top), n)).reshape(key.shape)
    M, terms = L + C.K, C.terms_of(L)
    tdt = G.tdt(torch, bits)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(
        np.int32 if bits == 32 else np.int64)).cuda()
    with low_cls(n, q) as low, nttmul.NttLevelKeySwitch(n, q, p, C.alpha_of(L)) as kn, \
            nttmul.NttLevelLinTrans(n, q, p) as lt, nttmul.NttModDown(n, q, p) as md:
        assert kn.digits == terms
        d_key = dev(key_hat)
        up = torch.full((batch, terms, M, n), -1, dtype=tdt, device="cuda")
        kn.modup_device(up, dev(low.forward(x)), batch)
        mid = torch.full((batch, 3, 2, M, n), -1, dtype=tdt, device="cuda")
        kn.mac_device(mid, up, d_key, ks, batch, terms, 2, view=C.VIEW)
        lin = torch.full((batch, 2, M, n), -1, dtype=tdt, device="cuda")
        lt.apply_device(lin, up, d_key, ks, batch, terms, 2, view=C.VIEW)
        out = torch.full((batch * 3 * 2, L, n), -1, dtype=tdt, device="cuda")
        md.moddown_device(out, mid, batch * 3 * 2)
        out_lin = torch.full((batch * 2, L, n), -1, dtype=tdt, device="cuda")
        md.moddown_device(out_lin, lin, batch * 2)
        torch.cuda.synchronize()
        # apply_view without weights is the modular sum of mac_view's rotations, bit for bit
        total = mid[:, 0]
        for r in (1, 2):
            nxt = torch.empty_like(total)
            for l, m in enumerate(q + p):
                nxt[..., l, :] = _addmod(torch, total[..., l, :], mid[:, r][..., l, :], m)
            total = nxt
        assert torch.equal(lin, total)
        back = low.inverse(G.host(out, bits)).reshape(batch, 3, 2, L, n)
        back_lin = low.inverse(G.host(out_lin, bits)).reshape(batch, 2, L, n)
    bound = (C.K + 1) * (1 + h)
    errs, want_sum = [], [np.zeros(n, dtype=object) for _ in q]
    for r, k in enumerate(ks):
        xr = galois_ref.coeff(x, k, q)[0]
        s2r = H.rotate_signed(s2, k)
        errs.append(ks_ref.key_switch_error(xr, back[0, r, 0], back[0, r, 1], q, s, s2r))
        for i, m in enumerate(q):
            want_sum[i] = (want_sum[i] + ks_ref.negacyclic(s2r, xr[i], m)) % m
    worst = 0
    for i, m in enumerate(q):
        e = (np.asarray(back_lin[0, 0, i]).astype(object)
             + ks_ref.negacyclic(s, back_lin[0, 1, i], m) - want_sum[i]) % m
        worst = max(worst, max(int(min(v, m - v)) for v in e))
    print("level chain errors", n, bits, errs, "sum", worst, "bound", bound)
    assert max(errs) <= bound
    assert worst <= bound
