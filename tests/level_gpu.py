"""What the GPU tests of include/nttmul_level.h share (test_gpu_level.py, test_gpu_level_footprint.py,
test_gpu_level_scale.py): operands made on the device for a case of tests/level_cases.py, the view
call and the dense call of the same context.  Imported only by tests that have a GPU."""
import numpy as np

import level_cases as C
import level_ref as LR
import nttmul


def tdt(torch, bits):
    return torch.int32 if bits == 32 else torch.int64


def host(t, bits):
    return t.cpu().numpy().view(np.uint32 if bits == 32 else np.uint64)


def random_device(torch, moduli, lead, n, bits, seed):
    """Canonical words [*lead, len(moduli), n] made on the device, limb l below moduli[l]."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    x = torch.empty((*lead, len(moduli), n), dtype=tdt(torch, bits), device="cuda")
    for l, m in enumerate(moduli):
        x[..., l, :] = torch.randint(0, m, (*lead, n), dtype=torch.int64, device="cuda",
                                     generator=gen).to(x.dtype)
    return x


def context(case, validate=False):
    """The case's context at its level, created through lib/libnttmul_level.so."""
    q, p = C.level_bases(case.bits, case.L)
    if case.op == "mac":
        return nttmul.NttLevelKeySwitch(case.n, q, p, C.alpha_of(case.L), validate=validate)
    if case.op == "lintrans":
        return nttmul.NttLevelLinTrans(case.n, q, p, validate=validate)
    return nttmul.NttLevelCtMul(case.n, q, p, validate=validate)


def operands(torch, case, seed=0):
    """dict of the case's operands on the device: the dense ones at the case's level, `key` (and
    `w` when weighted) made for the whole chain, and ks."""
    bits, n, b, L = case.bits, case.n, case.batch, case.L
    q_top, p = C.chain_bases(bits)
    q = q_top[:L]
    ext, ext_top = q + p, q_top + p
    terms = C.terms_of(L)
    seed += 1000 * L + n + bits
    ops = dict(terms=terms, ks=C.ks_of(n, case.rots),
               a=random_device(torch, ext, (b, terms), n, bits, seed))
    if case.op == "relin":
        ops["key"] = random_device(torch, ext_top, (2, C.TOP_TERMS), n, bits, seed + 1)
        ops["x"] = random_device(torch, q, (b, case.pairs, 2), n, bits, seed + 2)
        ops["y"] = random_device(torch, q, (b, case.pairs, 2), n, bits, seed + 3)
        return ops
    ops["key"] = random_device(torch, ext_top, (case.rots, case.comps, C.TOP_TERMS), n, bits,
                               seed + 1)
    ops["w"] = random_device(torch, ext_top, (case.rots,), n, bits, seed + 2) \
        if case.weighted else None
    ops["c0"] = random_device(torch, q, (b,), n, bits, seed + 3) if case.c0 else None
    return ops


def out_shape(case):
    M = case.L + C.K
    if case.op == "mac":
        return (case.batch, case.rots, case.comps, M, case.n)
    return (case.batch, 2 if case.op == "relin" else case.comps, M, case.n)


def call(torch, ctx, case, ops, view, out=None, key=None, w=None):
    """The case's call on ctx with `view` (None: the dense call) into out (made here, preset to
    all ones, when None).  key, w: operands in place of ops's (the gathered ones)."""
    key = ops["key"] if key is None else key
    w = ops.get("w") if w is None else w
    if out is None:
        out = torch.full(out_shape(case), -1, dtype=tdt(torch, case.bits), device="cuda")
    b, terms = case.batch, ops["terms"]
    if case.op == "mac":
        ctx.mac_device(out, ops["a"], key, ops["ks"], b, terms, case.comps, view=view)
    elif case.op == "lintrans":
        ctx.apply_device(out, ops["a"], key, ops["ks"], b, terms, case.comps, w_hat=w,
                         c0_hat=ops.get("c0"), view=view)
    else:
        ctx.relin_device(out, ops["a"], key, ops["x"], ops["y"], b, case.pairs, terms, view=view)
    torch.cuda.synchronize()
    return out


def gathered(case, ops):
    """(key, w) dense at the case's level: level_ref.gather of the top-level operands."""
    key = LR.gather(ops["key"], C.VIEW, case.L, ops["terms"])
    w = None if ops.get("w") is None else LR.gather(ops["w"], C.VIEW, case.L, None)
    return key, w


def case_id(c):
    tail = {"mac": f"c{c.comps}r{c.rots}",
            "lintrans": f"c{c.comps}r{c.rots}w{int(c.weighted)}z{int(c.c0)}",
            "relin": f"p{c.pairs}"}[c.op]
    return f"{c.op}-u{c.bits}-n{c.n}x{c.batch}-L{c.L}-{tail}"
