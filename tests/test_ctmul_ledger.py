"""The kernel ledger of lib/libnttmul_ctmul.so, in the style of tests/test_lintrans_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_ctmul.so = libnttmul_lintrans.so's kernels, bit for bit, plus k_ctmul_high
and k_ctmul_relin in both word classes (4 kernels), and every one is launched by a case of
tests/ctmul_cases.py (whose mirror test_gpu_ctmul.py anchors to the library's kernel_name entry
point on the GPU)."""
import os
import re
import subprocess

import pytest

import ctmul_cases as C
import nttmul

OLDER = ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
         "GALOIS_LIB_PATH", "KS_LIB_PATH", "MACN_LIB_PATH", "HOIST_LIB_PATH", "MDNTT_LIB_PATH",
         "KSNTT_LIB_PATH", "LINTRANS_LIB_PATH"]
CLASSES = (("Arith32P", "u32"), ("Arith64", "u64"))


@pytest.fixture(scope="module")
def lintrans():
    return nttmul.kernel_hashes(nttmul.LINTRANS_LIB_PATH)


@pytest.fixture(scope="module")
def ctmul():
    return nttmul.kernel_hashes(nttmul.CTMUL_LIB_PATH)


def _launched():
    out = {}
    for case in C.all_cases():
        for key in C.kernels_of(case):
            out.setdefault(key, case)
    return out


def expected_extra():
    return {f"k_ctmul_{op}<{cls},{io}>" for cls, io in CLASSES for op in C.OPS}


def test_common_kernels_are_the_lintrans_librarys_bit_for_bit(lintrans, ctmul):
    assert len([k for k in lintrans if k.startswith("k_lintrans")]) == 8
    assert sorted(set(lintrans) - set(ctmul)) == []
    assert {k: ctmul[k] for k in lintrans} == lintrans


def test_the_additional_kernels_are_exactly_what_the_cases_launch(lintrans, ctmul):
    extra = set(ctmul) - set(lintrans)
    launched = _launched()
    ours = {k for k in launched if k.startswith("k_ctmul")}
    # the range check: a kernel of the older libraries
    assert {k.split("<")[0] for k in set(launched) - ours} == {"k_rns_check_range"}
    assert all(k in lintrans for k in set(launched) - ours)
    assert sorted(extra - set(launched)) == [], "kernels no case launches"
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    assert C.UNREACHABLE == ()
    assert extra == expected_extra() and len(extra) == 4
    # every instantiation is hit at n = 256, with y_hat distinct and equal
    small = {(C.kernel_name(c.op, c.bits), c.square) for c in C.parity_cases() if c.n == 256}
    assert small == {(k, z) for k in expected_extra() for z in (False, True)}


def test_every_instantiation_in_the_source_has_a_case_and_the_reverse():
    """csrc/ctmul.hip: high<A, IO> and relin<A, IO> per word class, each in the launch and in the
    dry run."""
    src = open(os.path.join(nttmul.PKG_DIR, "csrc", "ctmul.hip")).read()
    for op in C.OPS:
        assert src.count(f"{op}<Arith32P, uint32_t>(") == src.count(f"{op}<Arith64, uint64_t>(") == 2
    assert set(re.findall(r"k_ctmul_(\w+)<A, IO>", src)) == set(C.OPS)
    named = {C.kernel_name(op, bits) for op in C.OPS for bits in (32, 64)}
    assert named == expected_extra() == {k for k in _launched() if k.startswith("k_ctmul")}


@pytest.mark.parametrize("path", OLDER)
def test_the_older_libraries_do_not_grow(path):
    """The twelve older libraries keep their ABI and kernels: the new entry points and k_ctmul_*
    are in the thirteenth library only."""
    out = subprocess.run(["nm", "-D", "--defined-only", getattr(nttmul, path)],
                         capture_output=True, text=True, check=True).stdout
    assert not re.search(r"ctmul", out)
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "ctmul" in k]


def test_mirror_restates_the_selection_and_the_grids():
    for bits, (cls, io) in zip((32, 64), CLASSES):
        for op in C.OPS:
            assert C.kernel_name(op, bits) == f"k_ctmul_{op}<{cls},{io}>"
    with pytest.raises(AssertionError):
        C.kernel_name("low", 32)
    with pytest.raises(AssertionError):
        C.relin_grid(1, 131072)
    with pytest.raises(AssertionError):
        C.high_grid(1, 128, 32)
    assert C.V == 4
    # relin: units, ceil(units / V), the partial last workgroup
    assert C.relin_grid(0, 256) == dict(units=0, groups=0, wgx=0, tail=0)
    assert C.relin_grid(1, 256) == dict(units=1, groups=1, wgx=1, tail=1)
    assert C.relin_grid(C.V - 1, 256) == dict(units=3, groups=1, wgx=1, tail=3)
    assert C.relin_grid(C.V, 256) == dict(units=4, groups=1, wgx=1, tail=0)
    assert C.relin_grid(C.V + 1, 256) == dict(units=5, groups=2, wgx=2, tail=1)
    assert C.relin_grid(2 * C.V - 1, 4096) == dict(units=7, groups=2, wgx=32, tail=3)
    assert C.relin_grid(5, 65536) == dict(units=5, groups=2, wgx=512, tail=1)
    # high: 256 vectors of 16 bytes per workgroup
    assert C.high_grid(0, 256, 32) == dict(vectors=0, wgx=0, vec=4, per=4, tail=0)
    assert C.high_grid(1, 256, 32) == dict(vectors=64, wgx=1, vec=4, per=4, tail=64)
    assert C.high_grid(4, 256, 32) == dict(vectors=256, wgx=1, vec=4, per=4, tail=0)
    assert C.high_grid(5, 256, 32) == dict(vectors=320, wgx=2, vec=4, per=4, tail=64)
    assert C.high_grid(1, 256, 64) == dict(vectors=128, wgx=1, vec=2, per=2, tail=128)
    assert C.high_grid(7, 512, 32) == dict(vectors=896, wgx=4, vec=4, per=2, tail=128)
    assert C.high_grid(7, 512, 64) == dict(vectors=1792, wgx=7, vec=2, per=1, tail=0)
    assert C.high_grid(5, 65536, 64) == dict(vectors=5 * 32768, wgx=640, vec=2, per=1, tail=0)
    case = C.Case("relin", 64, 8192, 5, 3, 2, 2, 2, False, True)
    assert C.kernels_of(case) == ["k_rns_check_range<u64>"] * 4 + ["k_ctmul_relin<Arith64,u64>"]
    assert C.kernels_of(case._replace(square=True)) == \
        ["k_rns_check_range<u64>"] * 3 + ["k_ctmul_relin<Arith64,u64>"]
    case = C.Case("high", 32, 8192, 5, 3, 2, 2, 2, True, True)
    assert C.kernels_of(case) == ["k_rns_check_range<u32>"] + ["k_ctmul_high<Arith32P,u32>"]
    assert C.units_per_block(case) == {"k_ctmul_high<Arith32P,u32>": (1, 5, 1024)}
    assert C.grid_rows(case) == {"k_ctmul_high<Arith32P,u32>": 3}
    assert C.launch_waves(case) == {"k_ctmul_high<Arith32P,u32>": 5 * 8 * 3 * 4}
    case = C.Case("relin", 32, 8192, 5, 3, 2, 2, 1, False)
    assert C.units_per_block(case) == {"k_ctmul_relin<Arith32P,u32>": (4, 5, 256)}
    assert C.grid_rows(case) == {"k_ctmul_relin<Arith32P,u32>": 5}
    assert C.launch_waves(case) == {"k_ctmul_relin<Arith32P,u32>": 2 * 32 * 5 * 4}
    small = C.Case("high", 32, 256, 5, 3, 2, 2, 1, False)
    assert C.units_per_block(small) == {"k_ctmul_high<Arith32P,u32>": (4, 5, 256)}


def test_the_cases_cover_what_the_issue_names():
    rows = C.parity_cases()
    for op in C.OPS:
        for bits in (32, 64):
            mine = [c for c in rows if c.bits == bits and c.op == op]
            assert {c.n for c in mine} == {256, 512, 4096, 8192, 65536}
            for n in (256, 512, 4096, 8192):
                here = [c for c in mine if c.n == n]
                assert {c.batch for c in here} == {1, C.V + 1, 2 * C.V - 1}
                assert {(c.L, c.K) for c in here} == {(1, 1), (4, 2), (12, 4)}
                assert {c.terms for c in here} == {1, 3} and {c.pairs for c in here} == {1, 3}
                assert {c.square for c in here} == {False, True}
            big = [c for c in mine if c.n == 65536]
            assert {(c.L, c.K) for c in big} == {(2, 1)}
            assert {c.batch for c in big} == {1, C.V + 1, 2 * C.V - 1}
            assert {c.pairs for c in big} == {1, 3} and {c.square for c in big} == {False, True}
            assert {(c.n, c.pairs, c.terms) for c in C.worst_cases()
                    if c.bits == bits and c.op == op} == {(n, 16, 16) for n in (256, 4096)}
    assert (C.V + 1) % C.V and (2 * C.V - 1) % C.V and C.V + 1 > C.V  # a partial and a full workgroup
    assert C.CHAIN_N == (256, 8192) and set(C.parity_cases()) <= set(C.referenced_cases())
    big = C.large_case()
    per = big.terms * (big.L + big.K) * big.n * (big.bits // 8)
    assert big.op == "relin" and big.batch * per > 1 << 32 >= (big.batch - 1) * per
    # the figures the header and the documents state
    assert [C.launches(n) for n in (4096, 8192)] == [6, 10]
    assert C.relin_byte_units(4, 2, 1, 2) == 4 * 6 + 16 and C.high_byte_units(4, 1) == 12


def test_every_kernel_that_takes_several_units_has_a_partial_workgroup_case():
    """k_ctmul_relin takes V entries at every n; k_ctmul_high takes several polynomials where 256
    vectors hold more than one.  Each such (kernel, units per workgroup) has a parity case whose
    last workgroup is partial, and one whose launch has a whole workgroup before it."""
    seen = {}
    for c in C.parity_cases():
        for key, (per, units, _) in C.units_per_block(c).items():
            if per > 1:
                seen.setdefault((key, per), []).append(units)
    assert {k for k, _ in seen} == expected_extra()
    assert {per for (k, per) in seen if "high<Arith32P" in k} == {4, 2}       # n = 256, 512
    assert {per for (k, per) in seen if "high<Arith64" in k} == {2}           # n = 256
    for (key, per), units in seen.items():
        assert any(u % per for u in units), (key, per)
        assert any(u % per and u > per for u in units), (key, per)
        assert any(u < per for u in units) or per == 2, (key, per)


def test_the_scale_cases_meet_the_rule_of_scale_cases():
    import scale_cases as S
    assert (C.MIN_WAVES, C.WAVE) == (S.MIN_WAVES, S.WAVE)
    rows = C.scale_cases()
    assert {(c.op, c.bits, c.n) for c in rows} == {(op, b, C.SCALE_N) for op in C.OPS
                                                   for b in (32, 64)}
    for case in rows:
        (key, waves), = C.launch_waves(case).items()
        assert key == C.kernel_name(case.op, case.bits)
        assert waves >= S.MIN_WAVES, (case, waves)
        per, units, _ = C.units_per_block(case)[key]
        assert per == (C.V if case.op == "relin" else 1)
        assert per == 1 or units % per, case                          # a partial last workgroup
        l = S.Launch(key, per, units, C.grid_rows(case)[key], 256, C.bpu(case), 1, 0)
        assert S.waves(l) == waves and S.wants_partial(l) == (per > 1)
        # the smallest such batch: every smaller one is short of the rule or ends whole
        for b in range(1, case.batch):
            less = case._replace(batch=b)
            assert min(C.launch_waves(less).values()) < S.MIN_WAVES or not C.ends_partial(less)


def test_every_exported_function_has_a_footprint_row_or_a_reason():
    EXEMPT = {"nttmul_ctmul_" + s for s in ("create", "destroy", "last_error", "get_info",
                                            "kernel_name")}      # no caller operand is written
    rows = C.footprint_cases()
    named = {f.entry for f in rows}
    exported = set(nttmul.ctmul_exported_symbols())
    writers = {s for s in exported if re.fullmatch(r"nttmul_ctmul_(high|relin)(_device)?", s)}
    assert len(writers) == 4 and named == writers
    assert EXEMPT == exported - writers
    for entry in writers:
        got = {(f.case.bits, f.case.n, f.case.batch, f.case.square) for f in rows
               if f.entry == entry}
        assert got == {(b, n, batch, sq) for b in (32, 64) for n, batch in C.FP_SIZES
                       for sq in (False, True)}
    assert all(batch % C.V for _, batch in C.FP_SIZES)              # a partial last workgroup
    assert all((f.host == "host") == (not f.entry.endswith("_device")) for f in rows)
    import guarded as G
    for f in rows:
        for per, units, words in C.units_per_block(f.case).values():
            assert C.fp_guard_words(f.case) >= max(per * words, G.guard_words(1))


def test_every_additional_kernel_is_launched_by_a_case_held_to_the_cpu_reference(lintrans, ctmul):
    """The mirror reports the cases whose every output word a GPU test compares with the CPU
    reference (referenced_cases(): at every n, tests/full_ref.py); the cases full_ref.SUBSET holds
    on a part of their batch only do not count, and are at most one in ten.  Every kernel this
    library adds over its predecessor is launched by one of the rest."""
    import full_ref
    cases = C.referenced_cases()
    assert cases and all(c in C.all_cases() for c in cases[:8] + cases[-8:])
    whole = [c for c in cases if not full_ref.on_subset("ctmul", c)]
    assert 10 * (len(cases) - len(whole)) <= len(cases)
    held = {k for c in whole for k in C.kernels_of(c)}
    excused = {k for k in ctmul if any(re.fullmatch(pat, k) for pat, _ in
                                        getattr(C, "UNREACHABLE", ()))}
    extra = set(ctmul) - set(lintrans)
    assert extra and sorted(extra - held - excused) == []
