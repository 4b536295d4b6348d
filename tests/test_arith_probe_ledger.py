"""The ledger of the device primitives, in the style of the kernel ledgers: no primitive without
a contract row and a probe op.

Runs without a GPU.  Names come from the header text: every __device__ member function of the
five arithmetic structs of csrc/modarith.hpp and every mac_add overload of csrc/mac_dev.hpp has a
row in tests/arith_contracts.py or a reason in its EXEMPT list; every row names an op that
lib/libnttmul_probe.so exports, and the reverse.  The host side of the probe (the plan's tables
and constants it hands the tests) is checked here too."""
import os
import re

import numpy as np
import pytest

import arith_contracts as C
import nttmul
import probe_lib

CSRC = os.path.join(nttmul.PKG_DIR, "csrc")
STRUCTS = ("Arith32", "Arith32P", "Arith32P3", "Arith32W", "Arith64")
MODULI = C.MODULI
ALL_Q = sorted({q for qs in MODULI.values() for q in qs})


def header_functions():
    """{(struct, function)} of the __device__ members of modarith.hpp's arithmetic structs, and
    (class, "mac_add") per overload of mac_dev.hpp."""
    text = open(os.path.join(CSRC, "modarith.hpp")).read()
    out = set()
    for m in re.finditer(r"^struct (\w+)[^{;]*\{\n(.*?)^\};", text, re.S | re.M):
        if m.group(1) in STRUCTS:
            out |= {(m.group(1), f) for f in re.findall(r"__device__[^;{(]*?\b(\w+)\s*\(", m.group(2))}
    mac = open(os.path.join(CSRC, "mac_dev.hpp")).read()
    out |= {(cls, "mac_add") for cls in
            re.findall(r"__device__[^;{(]*\bmac_add\(const (\w+) &", mac)}
    return out


def test_the_header_scan_finds_the_primitives():
    fns = header_functions()
    assert {s for s, _ in fns} == set(STRUCTS)
    for known in (("Arith32", "mont"), ("Arith32P", "ct"), ("Arith32P", "basemul4_lane"),
                  ("Arith32P3", "basemul"), ("Arith32P3", "outputs"), ("Arith32W", "redc"),
                  ("Arith64", "mulhi64"), ("Arith64", "canon_inv"), ("Arith32P", "mac_add"),
                  ("Arith32W", "mac_add"), ("Arith64", "mac_add")):
        assert known in fns, known
    assert len(fns) >= 45


def test_every_primitive_has_a_row_or_a_reason():
    fns = header_functions()
    rows = {C.op_function(r.op) for r in C.ROWS}
    missing = sorted(f for f in fns if f not in rows and f not in C.EXEMPT)
    assert not missing, f"primitives with neither a contract row nor an exemption: {missing}"
    assert sorted(f for f in C.EXEMPT if f in rows) == [], "exempt and tested"
    assert sorted(f for f in C.EXEMPT if f not in fns) == [], "stale exemptions"
    assert sorted(f for f in rows if f not in fns) == [], "rows for functions the headers lack"
    for reason in C.EXEMPT.values():
        assert reason.strip() and "\n" not in reason


def test_rows_and_probe_ops_are_the_same_set():
    ops = probe_lib.ops()
    assert len(ops) == len(set(ops))
    assert sorted(C.BY_OP) == sorted(ops)
    assert len(C.ROWS) == len(C.BY_OP)
    for row in C.ROWS:
        nin, nout, bits = probe_lib.shape(row.op)
        assert bits == C.word_bits(C.op_class(row.op)), row.op
        assert nout == len(row.outs), row.op
        words = sum(2 if d in C.TW_DOMS or d == "csub" else 1 for _, d in row.operands)
        if row.base:
            words = 2 * row.base + 2
        assert nin == words, row.op


def test_the_instantiations_the_kernels_use_have_rows():
    """The template arguments named in the ops are the ones kernels_dev.hpp / mac_dev.hpp spell."""
    for op in ["Arith32P.ct<%s>" % c for c in ("T,F,F", "T,F,T", "F,F,F", "F,F,T", "F,T,F", "F,T,T")] + \
            ["Arith32P.basemul<4,%s,%s>" % (n, z) for n in "FT" for z in "FT"] + \
            ["Arith32P3.basemul<8,%s,%s>" % (n, z) for n in "FT" for z in "FT"] + \
            ["Arith32P.basemul4_lane<F>", "Arith32P.basemul4_lane<T>", "Arith64.mulhi64<F>",
             "Arith64.mulhi64<T>", "Arith64.shoup<T>", "Arith64.shoup<F>", "Arith64.ct<F>",
             "Arith64.ct<T>", "Arith64.basemul<4,F>", "Arith64.basemul<4,T>"]:
        assert op in C.BY_OP, op


def test_moduli_are_the_issue_s():
    assert MODULI["Arith32P"][:5] == (7681, 12289, C.D.Q31LO, C.D.Q31, C.D.Q31HI)
    assert MODULI["Arith32P3"] == MODULI["Arith32P"]      # p3_fold_ok holds below 2^31
    assert MODULI["Arith32P"][5] == nttmul.find_prime(256, 31)
    w0, w1 = MODULI["Arith32W"]
    assert (1 << 31) <= w0 < w1 < (1 << 32) and w1 == nttmul.find_prime(256, 32)
    assert not any(nttmul.is_prime(q) for q in range((1 << 31) + 1, w0, 512))
    l0 = MODULI["Arith64"][0]
    assert l0 >= (1 << 32) and not any(nttmul.is_prime(q) for q in range((1 << 32) + 1, l0, 512))
    assert MODULI["Arith64"][1:] == (C.D.Q33, C.D.Q62, nttmul.find_prime(256, 62))
    assert all(nttmul.is_prime(q) and q % 512 == 1 for q in ALL_Q)


@pytest.mark.parametrize("q", ALL_Q)
def test_documented_pair_formats_match_the_planner(q):
    """The pairs Python forms for the edge twiddles follow the documented formats: formed for the
    tables' own values they reproduce every pair of the planner's two tables, typing included."""
    fw, iw, sg, fwp, iwp = probe_lib.tables(q)
    fforms, iforms = C.table_forms(q, sg)
    if q < (1 << 31):
        assert sg.any() and not sg.all(), "the forward table carries both forms"
    else:
        assert not sg.any()
    for forms, pairs, plain in ((fforms, fw, fwp), (iforms, iw, iwp)):
        for i in range(1, 256):
            assert 0 < int(plain[i]) < q
            assert C.pair_of(forms[i], int(plain[i]), q) == (int(pairs[i][0]), int(pairs[i][1])), (q, i)
    tw = C.twiddle_lists(q, fw, iw, sg, fwp, iwp)
    assert sum(len(v) for v in tw.values()) == 2 * 255 + len(tw) * len(C.edge_twiddles(q))


@pytest.mark.parametrize("q", ALL_Q)
def test_probe_constants_are_make_params(q):
    k = probe_lib.consts(q)
    bits = 32 if q < (1 << 32) else 64
    assert k["qinv_neg"] == (-pow(q, -1, 1 << bits)) % (1 << bits)
    if q < (1 << 31):
        assert (k["c32"], k["as"]) == ((1 << 32) % q, (3 * q + 1) // 2)
    if bits == 64:
        assert k["q2"] == 2 * q
    iw1 = int(probe_lib.tables(q)[4][1])
    f = pow(256, -1, q) * (1 << bits) % q
    uform, sform = ("tw_u", "tw_s") if q < (1 << 31) else ("tw_m",) * 2 if bits == 32 else ("tw_h",) * 2
    for mul, name in ((1, ""), (4, "4"), (8, "8")):
        assert C.pair_of(uform, f * mul % q, q) == (k["f" + name], k["f" + name + "s"])
        assert C.pair_of(sform, iw1 * f * mul % q, q) == (k["wf" + name], k["wf" + name + "s"])


def test_probe_refuses_a_modulus_outside_the_class():
    x = [np.zeros(4, np.uint64)] * 2
    for op, cls in (("Arith32P.mont", "Arith64"), ("Arith64.mont", "Arith32P"),
                    ("Arith32W.mont", "Arith32P"), ("Arith32.mont", "Arith32W")):
        with pytest.raises(RuntimeError):
            probe_lib.run(op, MODULI[cls][0], x)
    with pytest.raises(RuntimeError):
        probe_lib.shape("Arith32P.nothing")


@pytest.mark.parametrize("cls", STRUCTS)
def test_tuples_stay_inside_their_domains(cls):
    """The generator itself: every operand of every tuple lies in the domain its row declares,
    both ends of each domain are present, and the reference runs on them (largest modulus)."""
    q = MODULI[cls][-1]
    tw = C.python_twiddle_lists(q)
    for row in C.ROWS:
        head = row.op.split(".")[0]
        if (C.op_class(row.op) if head == "mac_add" else head) != cls:
            continue
        bits = C.word_bits(C.op_class(row.op))
        words, values = C.tuples(row, q, tw)
        assert len({len(w) for w in words}) == 1 and len(words[0]) >= 2048, row.op
        assert all(int(w.max()) < (1 << bits) for w in words), row.op
        want = row.ref(q, *values)
        assert len(want) == len(row.outs)
        if row.operands[0][1] == "csub":
            x, m = values
            assert ((x >= 0) & (x < 2 * m) & (x < (1 << bits))).all() and set(m) == {q, 2 * q}
            continue
        doms = ([row.operands[0][1]] * (2 * row.base) + [row.operands[1][1]] if row.base
                else [d for _, d in row.operands])
        for dom, v in zip(doms, values):
            if dom in C.TW_DOMS:
                assert ((v > 0) & (v < q)).all(), (row.op, dom)
            else:
                lo, hi = C.domain_bounds(dom, q, bits)
                assert ((v >= lo) & (v < hi)).all(), (row.op, dom)
                assert lo in set(v) and hi - 1 in set(v), (row.op, dom)
