"""The kernel ledger of lib/libnttmul_lintrans.so, in the style of tests/test_ksntt_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_lintrans.so = libnttmul_ksntt.so's kernels, bit for bit, plus k_lintrans
with one and two components, weighted and not, in both word classes (8 kernels), and every one is
launched by a case of tests/lintrans_cases.py (whose mirror test_gpu_lintrans.py anchors to the
library's kernel_name entry point on the GPU)."""
import re
import subprocess

import pytest

import lintrans_cases as C
import nttmul

OLDER = ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
         "GALOIS_LIB_PATH", "KS_LIB_PATH", "MACN_LIB_PATH", "HOIST_LIB_PATH", "MDNTT_LIB_PATH",
         "KSNTT_LIB_PATH"]
CLASSES = (("Arith32P", "u32"), ("Arith64", "u64"))


@pytest.fixture(scope="module")
def ksntt():
    return nttmul.kernel_hashes(nttmul.KSNTT_LIB_PATH)


@pytest.fixture(scope="module")
def lintrans():
    return nttmul.kernel_hashes(nttmul.LINTRANS_LIB_PATH)


def _launched():
    out = {}
    for case in C.all_cases():
        for key in C.kernels_of(case):
            out.setdefault(key, case)
    return out


def expected_extra():
    return {f"k_lintrans<{cls},{io},{comps},{w}>" for cls, io in CLASSES for comps in (1, 2)
            for w in (0, 1)}


def test_common_kernels_are_the_ksntt_librarys_bit_for_bit(ksntt, lintrans):
    assert len([k for k in ksntt if k.startswith("k_ksntt_")]) == 30
    assert sorted(set(ksntt) - set(lintrans)) == []
    assert {k: lintrans[k] for k in ksntt} == ksntt


def test_the_additional_kernels_are_exactly_what_the_cases_launch(ksntt, lintrans):
    extra = set(lintrans) - set(ksntt)
    launched = _launched()
    ours = {k for k in launched if k.startswith("k_lintrans")}
    # the range check: a kernel of the older libraries
    assert {k.split("<")[0] for k in set(launched) - ours} == {"k_rns_check_range"}
    assert all(k in ksntt for k in set(launched) - ours)
    assert sorted(extra - set(launched)) == [], "kernels no case launches"
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    assert C.UNREACHABLE == ()
    assert extra == expected_extra() and len(extra) == 8
    # every instantiation is hit at n = 256, with and without c0
    small = {(C.kernel_name(c.bits, c.comps, c.weighted), c.c0) for c in C.parity_cases()
             if c.n == 256}
    assert small == {(k, z) for k in expected_extra() for z in (False, True)}


def test_every_instantiation_in_the_source_has_a_case_and_the_reverse():
    """csrc/lintrans.hip apply_comps: the four apply<A, IO, COMPS, WEIGHTED> per word class."""
    import os
    src = open(os.path.join(nttmul.PKG_DIR, "csrc", "lintrans.hip")).read()
    inst = set(re.findall(r"apply<A, IO, (\d), ([01])>", src))
    assert inst == {(str(c), w) for c in (1, 2) for w in ("0", "1")}
    assert src.count("apply_comps<Arith32P, uint32_t>") == \
        src.count("apply_comps<Arith64, uint64_t>") == 2
    named = {C.kernel_name(bits, int(c), w == "1") for bits in (32, 64) for c, w in inst}
    assert named == expected_extra() == {k for k in _launched() if k.startswith("k_lintrans")}


@pytest.mark.parametrize("path", OLDER)
def test_the_older_libraries_do_not_grow(path):
    """The eleven older libraries keep their ABI and kernels: the new entry points and k_lintrans
    are in the twelfth library only."""
    out = subprocess.run(["nm", "-D", "--defined-only", getattr(nttmul, path)],
                         capture_output=True, text=True, check=True).stdout
    assert not re.search(r"lintrans", out)
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "lintrans" in k]


def test_mirror_restates_the_selection_and_the_grid():
    for bits, (cls, io) in zip((32, 64), CLASSES):
        for comps in (1, 2):
            for w in (False, True):
                assert C.kernel_name(bits, comps, w) == f"k_lintrans<{cls},{io},{comps},{int(w)}>"
    with pytest.raises(AssertionError):
        C.kernel_name(32, 3, True)
    with pytest.raises(AssertionError):
        C.grid(1, 131072)
    assert C.V == 4
    # units, ceil(units / V), the partial last workgroup
    assert C.grid(0, 256) == dict(units=0, groups=0, wgx=0, tail=0)
    assert C.grid(1, 256) == dict(units=1, groups=1, wgx=1, tail=1)
    assert C.grid(C.V - 1, 256) == dict(units=3, groups=1, wgx=1, tail=3)
    assert C.grid(C.V, 256) == dict(units=4, groups=1, wgx=1, tail=0)
    assert C.grid(C.V + 1, 256) == dict(units=5, groups=2, wgx=2, tail=1)
    assert C.grid(2 * C.V - 1, 4096) == dict(units=7, groups=2, wgx=32, tail=3)
    assert C.grid(5, 65536) == dict(units=5, groups=2, wgx=512, tail=1)
    case = C.Case(64, 8192, 5, 3, 2, 2, 2, (5,), True, True, True)
    assert C.kernels_of(case) == ["k_rns_check_range<u64>"] * 4 + ["k_lintrans<Arith64,u64,2,1>"]
    case = C.Case(32, 8192, 5, 3, 2, 2, 1, (5,), False, False, True)
    assert C.kernels_of(case) == ["k_rns_check_range<u32>"] * 2 + ["k_lintrans<Arith32P,u32,1,0>"]
    assert C.units_per_block(case) == {"k_lintrans<Arith32P,u32,1,0>": (4, 5, 256)}
    assert C.grid_rows(case) == {"k_lintrans<Arith32P,u32,1,0>": 5}
    assert C.launch_waves(case) == {"k_lintrans<Arith32P,u32,1,0>": 2 * 32 * 5 * 4}


def test_the_cases_cover_what_the_issue_names():
    rows = C.parity_cases()
    for bits in (32, 64):
        mine = [c for c in rows if c.bits == bits]
        assert {c.n for c in mine} == {256, 512, 4096, 8192, 65536}
        for n in (256, 512, 4096, 8192):
            here = [c for c in mine if c.n == n]
            assert {c.batch for c in here} == {1, C.V + 1, 2 * C.V - 1}
            assert {(c.L, c.K) for c in here} == {(1, 1), (4, 2), (12, 4)}
            assert {c.terms for c in here} == {1, 3} and {c.comps for c in here} == {1, 2}
            assert {len(c.ks) for c in here} == {1, 2, 16}
            assert {k for c in here for k in c.ks} == {1, 5, 25, 2 * n - 1}
            assert any(len(set(c.ks)) < len(c.ks) for c in here)      # a repeated element
            assert {(c.comps, c.weighted, c.c0) for c in here} == \
                {(i, w, z) for i in (1, 2) for w in (False, True) for z in (False, True)}
        big = [c for c in mine if c.n == 65536]
        assert {(c.L, c.K) for c in big} == {(2, 1)} and max(len(c.ks) for c in big) == 3
        assert {c.batch for c in big} == {1, C.V + 1, 2 * C.V - 1}
        assert {(c.weighted, c.c0) for c in big} == {(w, z) for w in (0, 1) for z in (0, 1)}
        assert {(c.n, len(c.ks), c.terms, c.comps, c.weighted, c.c0) for c in C.worst_cases()
                if c.bits == bits} == {(n, 16, 16, 2, True, True) for n in (256, 4096)}
    assert (C.V + 1) % C.V and (2 * C.V - 1) % C.V and C.V + 1 > C.V  # a partial and a full workgroup
    assert C.CHAIN_N == (256, 8192) and set(C.parity_cases()) <= set(C.referenced_cases())
    big = C.large_case()
    per = big.terms * (big.L + big.K) * big.n * (big.bits // 8)
    assert big.batch * per > 1 << 32 >= (big.batch - 1) * per
    # the figures the header and the documents state
    assert [C.launches(n) for n in (4096, 8192)] == [5, 9]
    assert (C.byte_units(2, 8, 2, False), C.byte_units(2, 8, 2)) == (18, 4)
    assert (C.moddown_polys(3, 8, False), C.moddown_polys(3, 8)) == (48, 6)


def test_the_scale_cases_meet_the_rule_of_scale_cases():
    import scale_cases as S
    assert (C.MIN_WAVES, C.WAVE) == (S.MIN_WAVES, S.WAVE)
    rows = C.scale_cases()
    assert {(c.bits, c.n) for c in rows} == {(b, C.SCALE_N) for b in (32, 64)}
    for case in rows:
        (key, waves), = C.launch_waves(case).items()
        assert key == C.kernel_name(case.bits, case.comps, case.weighted)
        assert waves >= S.MIN_WAVES, (case, waves)
        per, units, _ = C.units_per_block(case)[key]
        assert per == C.V and units % per, case                     # a partial last workgroup
        l = S.Launch(key, per, units, C.grid_rows(case)[key], 256, C.bpu(case), 1, 0)
        assert S.waves(l) == waves and S.wants_partial(l)
        # the smallest such batch: every smaller one is short of the rule or ends whole
        for b in range(1, case.batch):
            less = case._replace(batch=b)
            assert min(C.launch_waves(less).values()) < S.MIN_WAVES or b % C.V == 0


def test_every_exported_function_has_a_footprint_row_or_a_reason():
    EXEMPT = {"nttmul_lintrans_" + s for s in ("create", "destroy", "last_error", "get_info",
                                               "kernel_name")}   # no caller operand is written
    rows = C.footprint_cases()
    named = {f.entry for f in rows}
    exported = set(nttmul.lintrans_exported_symbols())
    writers = {s for s in exported if re.fullmatch(r"nttmul_lintrans_apply(_device)?", s)}
    assert len(writers) == 2 and named == writers
    assert EXEMPT == exported - writers
    for entry in writers:
        got = {(f.case.bits, f.case.n, f.case.batch, f.case.weighted, f.case.c0) for f in rows
               if f.entry == entry}
        assert got == {(b, n, batch, w, z) for b in (32, 64) for n, batch in C.FP_SIZES
                       for w, z in C.FP_OPTIONAL}
    assert all(batch % C.V for _, batch in C.FP_SIZES)              # a partial last workgroup
    assert all((f.host == "host") == (not f.entry.endswith("_device")) for f in rows)
    import guarded as G
    for f in rows:
        for per, units, words in C.units_per_block(f.case).values():
            assert C.fp_guard_words(f.case) >= max(per * words, G.guard_words(1))


def test_every_additional_kernel_is_launched_by_a_case_held_to_the_cpu_reference(ksntt, lintrans):
    """The mirror reports the cases whose every output word a GPU test compares with the CPU
    reference (referenced_cases(): at every n, tests/full_ref.py); the cases full_ref.SUBSET holds
    on a part of their batch only do not count, and are at most one in ten.  Every kernel this
    library adds over its predecessor is launched by one of the rest."""
    import full_ref
    cases = C.referenced_cases()
    assert cases and all(c in C.all_cases() for c in cases[:8] + cases[-8:])
    whole = [c for c in cases if not full_ref.on_subset("lintrans", c)]
    assert 10 * (len(cases) - len(whole)) <= len(cases)
    held = {k for c in whole for k in C.kernels_of(c)}
    excused = {k for k in lintrans if any(re.fullmatch(pat, k) for pat, _ in
                                        getattr(C, "UNREACHABLE", ()))}
    extra = set(lintrans) - set(ksntt)
    assert extra and sorted(extra - held - excused) == []
