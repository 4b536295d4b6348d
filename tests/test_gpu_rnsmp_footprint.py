"""The caller's memory around lib/libnttmul_rnsmp.so's calls (include/nttmul_rnsmp.h "Caller
memory"), in the style of tests/test_gpu_footprint.py and on tests/guarded.py as it stands: every
`_device` entry point and every host form runs between sentinel guards at addresses aligned to
the word and to nothing larger; afterwards no guard word and no input has changed, every output
word is written, and the result is right bit for bit.

The rows are tests/rnsmp_cases.py footprint_cases(): n = 8192 and 65536, both word classes,
L = 3, batch 1 and 5 (the column and row kernels index caller memory by (p L + l) and a row or a
column: 5 and 3 are multiples of nothing the addressing shifts by), the transforms also in place.
The ledger below, without a GPU, requires a row or an exemption for every function the header
adds."""
import re

import numpy as np
import pytest

import guarded as G
import nttmul
import rnsmp_cases as R
from oracle import oracle as O

# Functions of include/nttmul_rnsmp.h without a footprint row: (regular expression, reason)
EXEMPT = (
    (r"nttmul_rnsmp_(create|destroy)", "create and release a context; write one handle"),
    (r"nttmul_rnsmp_(last_error|get_info|limb_info|kernel_name)",
     "diagnostics and queries: one small struct or a string of at most cap bytes, no launch"),
)


def _exempt_reason(name):
    for pattern, reason in EXEMPT:
        if re.fullmatch(pattern, name):
            return reason
    return None


def groups():
    out = {}
    for f in R.footprint_cases():
        out.setdefault((f.case.n, R.word_bits(f.case.moduli)), []).append(f)
    return out


GROUPS = groups()


# ---------------------------------------------------------------------------------------------
# the ledger (no GPU)
# ---------------------------------------------------------------------------------------------

def test_every_exported_entry_point_has_a_row_or_an_exemption():
    exported = nttmul.rnsmp_exported_symbols()
    assert len(exported) == len(set(exported)) == 14
    named = {f.entry for f in R.footprint_cases()}
    assert sorted(named - set(exported)) == [], "rows name functions the header does not export"
    missing = sorted(s for s in exported if s not in named and not _exempt_reason(s))
    assert not missing, f"exported without a footprint row or an exemption: {missing}"
    both = sorted(s for s in named if _exempt_reason(s))
    assert not both, f"exempt but covered by a row: {both}"
    for pattern, reason in EXEMPT:
        assert any(re.fullmatch(pattern, s) for s in exported), f"rule matches nothing: {pattern}"
        assert reason.strip() and "\n" not in reason
    # everything that takes a batch of caller buffers is covered by rows, not by exemptions
    batchy = [s for s in exported if re.fullmatch(
        r"nttmul_rnsmp_(multiply|forward|inverse|mac_ntt)(_device)?", s)]
    assert len(batchy) == 8 and set(batchy) == named


def test_the_rows_hold_what_the_plan_asks_for():
    rows = R.footprint_cases()
    dev = [f for f in rows if not f.host]
    assert {(f.case.n, R.word_bits(f.case.moduli)) for f in rows} == \
        {(n, w) for n in (8192, 65536) for w in (32, 64)} == set(GROUPS)
    assert {len(f.case.moduli) for f in rows} == {3}
    assert {f.case.batch for f in dev} == {1, 5} and {f.case.batch for f in rows if f.host} == {3}
    assert {(f.case.op, f.alias) for f in dev if f.alias} == {("forward", "out=in"), ("inverse", "out=in")}
    assert {(f.case.op, f.case.shared) for f in dev} >= {("mac", False), ("mac", True)}
    assert sum(len(v) for v in GROUPS.values()) == len(rows)
    # a batch that is no multiple of anything: odd, and coprime to the limb count
    assert all(b % 2 == 1 and b % 3 for b in (5,))
    for f in rows:
        guard = R.fp_guard_words(f.case)
        assert guard >= G.GUARD_MIN and guard >= f.case.terms * len(f.case.moduli) * f.case.n
        keys = R.units_per_block(f.case)
        assert set(keys) == set(R.kernels_of(f.case))
        assert all(guard >= upb * words for upb, _, words in keys.values())


# ---------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _sum_mod(rows, q):
    acc = rows[0].astype(object)
    for r in rows[1:]:
        acc = acc + r.astype(object)
    return (acc % q).astype(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("param", sorted(GROUPS), ids=lambda p: f"{p[0]}-u{p[1]}")
def test_rnsmp(param, torch_cuda):
    """Product, both transforms (also in place) and the mac over [batch][3][n] operands, batch 1
    and 5, and the host forms with batch 3: products against the oracle per limb, transforms
    against plain contexts of the same library per limb."""
    torch = torch_cuda
    n, bits = param
    rows = GROUPS[param]
    moduli = rows[0].case.moduli
    L, T = len(moduli), R.FP_TERMS
    B_ = max(f.case.batch for f in rows)
    dt = G.dtype_of(bits)
    per = [O.fill_inputs(n, q, 40, B_ * T) for q in moduli]
    a = np.ascontiguousarray(np.stack([p[0].reshape(B_, T, n) for p in per], axis=2))
    b = np.ascontiguousarray(np.stack([p[1].reshape(B_, T, n) for p in per], axis=2))
    plans = [O.Plan(n, q) for q in moduli]

    def products(shared):
        """[B_, T, L, n]: the oracle's a[p][t][l] * b[shared ? 0 : p][t][l]."""
        return np.stack([np.stack([np.stack([
            plans[l].product_merged(a[p, t, l], b[0 if shared else p, t, l])
            for l in range(L)]) for t in range(T)]) for p in range(B_)])

    prod = {s: products(s) for s in (False, True)}
    mac = {s: np.stack([_sum_mod([prod[s][:, t, l] for t in range(T)], q)
                        for l, q in enumerate(moduli)], axis=1) for s in (False, True)}
    plain = [nttmul.Context(n, q, _lib=nttmul.load_rnsmp_library()) for q in moduli]

    def per_limb(op, x):
        flat = x.reshape(-1, L, n)
        out = np.stack([getattr(plain[l], op)(np.ascontiguousarray(flat[:, l]), dtype=dt)
                        for l in range(L)], axis=1)
        return out.reshape(x.shape).astype(np.uint64)

    fwd, inv, b_hat = per_limb("forward", a[:, 0]), per_limb("inverse", a[:, 0]), per_limb("forward", b)
    with nttmul.RnsMpContext(n, moduli) as ctx:
        assert ctx.word_bits == bits
        for f in rows:
            c = f.case
            assert c.moduli == moduli and f.entry == R.ENTRY[c.op] + ("" if f.host else "_device")
            batch, words = c.batch, c.batch * L * n
            guard = R.fp_guard_words(c)
            if c.op == "mac":
                assert c.terms == T
                operands = dict(c=words, a=a[:batch], b=b_hat[0] if c.shared else b_hat[:batch])
                want, out = mac[c.shared][:batch], "c"
            elif c.op == "multiply":
                operands = dict(c=words, a=a[:batch, 0], b=b[:batch, 0])
                want, out = prod[False][:batch, 0], "c"
            else:
                operands = dict(out=words, x=a[:batch, 0])
                want, out = (fwd if c.op == "forward" else inv)[:batch], "out"
            inplace = ()
            if f.alias:
                assert f.alias == "out=in" and c.op in ("forward", "inverse") and not f.host
                del operands["out"]
                inplace, out = ("x",), "x"
            if f.host:
                arena = G.HostArena(bits, guard, **operands)
                ptr = lambda k: arena[k].ctypes.data                           # noqa: E731
                fn = getattr(ctx._lib, f.entry)
                if c.op == "mac":
                    ctx._check(fn(ctx._h, ptr("c"), ptr("a"), ptr("b"), batch, T, int(c.shared)))
                elif c.op == "multiply":
                    ctx._check(fn(ctx._h, ptr("c"), ptr("a"), ptr("b"), batch))
                else:
                    ctx._check(fn(ctx._h, ptr("out"), ptr("x"), batch))
            else:
                arena = G.DeviceArena(torch, bits, guard, inplace=inplace, **operands)
                ptr = lambda k: arena[k]                                       # noqa: E731
                s = torch.cuda.current_stream().cuda_stream
                if c.op == "mac":
                    ctx.mac_ntt_device(ptr("c"), ptr("a"), ptr("b"), batch, T, shared=c.shared,
                                       stream=s)
                elif c.op == "multiply":
                    ctx.multiply_device(ptr("c"), ptr("a"), ptr("b"), batch, stream=s)
                else:
                    getattr(ctx, f"{c.op}_device")(ptr(out), ptr("x"), batch, stream=s)
                torch.cuda.synchronize()
            arena.check()
            got = arena.get(out, (batch, L, n)).astype(np.uint64)
            assert got.dtype == np.uint64 and np.array_equal(got, want), f
    for p in plain:
        p.close()
