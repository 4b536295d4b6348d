"""The caller's memory around the view calls (include/nttmul_level.h "Caller memory"), in the style
of tests/test_gpu_ctmul_footprint.py and on tests/guarded.py as it stands: the `_device` entry
points and the host forms run between sentinel guards at addresses aligned to the word and to
nothing larger; afterwards no guard word has changed, every input, the viewed top-level operands
among them, is bit-identical to the copy taken before the call, exactly the output's words are
written (the arena's output is that long, every word after it is a guard, and no word of it keeps
the sentinel), and the result is the dense call's on the gathered operand bit for bit.

The rows are tests/level_cases.py footprint_cases(): n = 256 with batch 5 and n = 8192 with batch
3 (partial last workgroups), level 3 of the five-limb chain, two components, three rotations with
weights and c_0, three pairs, both word classes.  The no-GPU half holds the rows to the header:
every exported function has a row or a reason in EXEMPT."""
import numpy as np
import pytest

import guarded
import level_cases as C
import nttmul

EXEMPT = {"nttmul_level_kernel_name": "writes at most cap bytes of a name"}


def groups():
    out = {}
    for f in C.footprint_cases():
        out.setdefault((f.case.op, f.case.bits, f.case.n), []).append(f)
    return out


GROUPS = groups()


def test_every_exported_function_has_a_row_or_a_reason():
    named = {f.entry for f in C.footprint_cases()}
    exported = set(nttmul.level_exported_symbols())
    assert named <= exported and set(EXEMPT) <= exported
    assert not named & set(EXEMPT)
    assert sorted(exported - named - set(EXEMPT)) == []
    assert all(EXEMPT.values())
    for entry in named:
        for host in ("", "host"):
            assert any(f.entry == entry and f.host == host for f in C.footprint_cases()) == \
                (entry.endswith("_device") != bool(host))


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _ptr(view, host):
    return view.ctypes.data if host else view.data_ptr()


@pytest.mark.gpu
@pytest.mark.parametrize("param", sorted(GROUPS), ids=lambda p: f"{p[0]}-u{p[1]}-n{p[2]}")
def test_calls(param, torch_cuda):
    import ctypes

    import level_gpu as G
    torch = torch_cuda
    op, bits, n = param
    rows = GROUPS[param]
    case = rows[0].case
    assert all(f.case == case for f in rows) and len(rows) == 2
    ops = G.operands(torch, case, seed=11)
    terms, ks = ops["terms"], ops["ks"]
    shape = G.out_shape(case)
    view = nttmul.LevelView(*C.VIEW)
    karr = (ctypes.c_uint32 * len(ks))(*ks)
    # one batch entry of the widest operand: a rotation of the top-level key
    guard = guarded.guard_words(2 * C.TOP_TERMS * C.top_limbs() * n)
    with G.context(case) as ctx:
        key, w = G.gathered(case, ops)
        want = G.host(G.call(torch, ctx, case, ops, None, key=key, w=w), bits)
        names = ("a", "key", "w", "c0", "x", "y")
        inputs = {k: G.host(ops[k], bits) for k in names if ops.get(k) is not None}
        for f in rows:
            host = bool(f.host)
            operands = dict(out=int(np.prod(shape)), **inputs)
            arena = guarded.HostArena(bits, guard, **operands) if host else \
                guarded.DeviceArena(torch, bits, guard, **operands)
            at = lambda k: _ptr(arena[k], host)
            fn = getattr(ctx._lib, f.entry)
            tail = () if host else (0, torch.cuda.current_stream().cuda_stream or None)
            if op == "mac":
                st = fn(ctx._h, at("out"), at("a"), at("key"), karr, len(ks), case.batch, terms,
                        case.comps, ctypes.byref(view), *tail)
            elif op == "lintrans":
                st = fn(ctx._h, at("out"), at("a"), at("key"), at("w"), at("c0"), karr, len(ks),
                        case.batch, terms, case.comps, ctypes.byref(view), *tail)
            else:
                st = fn(ctx._h, at("out"), at("a"), at("key"), at("x"), at("y"), case.batch,
                        case.pairs, terms, ctypes.byref(view), *tail)
            ctx._check(st)
            if not host:
                torch.cuda.synchronize()
            arena.check()
            assert np.array_equal(arena.get("out", shape), want), f
