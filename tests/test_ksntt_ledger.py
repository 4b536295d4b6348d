"""The kernel ledger of lib/libnttmul_ksntt.so, in the style of tests/test_mdntt_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_ksntt.so = libnttmul_mdntt.so's kernels, bit for bit, plus k_ksntt_fwd at
the five degrees up to 4096, k_ksntt_cols_fwd and k_ksntt_rows at the four splits above and
k_ksntt_mac with one and two components, in both word classes (30 kernels), and every one is
launched by a case of tests/ksntt_cases.py (whose mirror test_gpu_ksntt.py anchors to the
library's kernel_name entry point on the GPU).  modup's inverse half adds no kernel: it launches
libnttmul_mdntt.so's k_mdntt_inv / k_mdntt_inv_rows and libnttmul_rnsmp.so's k_rnsmp_cols_inv."""
import re
import subprocess

import pytest

import ksntt_cases as C
import nttmul

OLDER = ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
         "GALOIS_LIB_PATH", "KS_LIB_PATH", "MACN_LIB_PATH", "HOIST_LIB_PATH", "MDNTT_LIB_PATH"]
CLASSES = (("Arith32P", "u32"), ("Arith64", "u64"))


@pytest.fixture(scope="module")
def mdntt():
    return nttmul.kernel_hashes(nttmul.MDNTT_LIB_PATH)


@pytest.fixture(scope="module")
def ksntt():
    return nttmul.kernel_hashes(nttmul.KSNTT_LIB_PATH)


def _launched():
    out = {}
    for case in C.all_cases():
        for key in C.kernels_of(case):
            out.setdefault(key, case)
    return out


def _unreachable_reason(key):
    for pattern, reason in C.UNREACHABLE:
        if re.fullmatch(pattern, key):
            return reason
    return None


def expected_extra():
    want = {f"k_ksntt_fwd<{cls},{io},{logn}>" for cls, io in CLASSES for logn in range(8, 13)}
    want |= {f"{k}<{cls},{io},{l1}>" for cls, io in CLASSES for l1 in range(1, 5)
             for k in ("k_ksntt_cols_fwd", "k_ksntt_rows")}
    want |= {f"k_ksntt_mac<{cls},{io},{comps}>" for cls, io in CLASSES for comps in (1, 2)}
    return want


def test_common_kernels_are_the_mdntt_librarys_bit_for_bit(mdntt, ksntt):
    assert len(mdntt) > 269 + 56 + 9 + 2 + 18 + 36 + 44
    assert sorted(set(mdntt) - set(ksntt)) == []
    assert {k: ksntt[k] for k in mdntt} == mdntt


def test_the_additional_kernels_are_exactly_what_the_cases_launch(mdntt, ksntt):
    extra = set(ksntt) - set(mdntt)
    launched = _launched()
    ours = {k for k in launched if k.startswith("k_ksntt_")}
    # the range check and the inverse half: kernels of the older libraries
    assert all(k in mdntt for k in set(launched) - ours)
    assert {k.split("<")[0] for k in set(launched) - ours} == {
        "k_rns_check_range", "k_mdntt_inv", "k_mdntt_inv_rows", "k_rnsmp_cols_inv"}
    missing = sorted(k for k in extra if k not in launched and not _unreachable_reason(k))
    assert not missing, f"kernels no case launches and no rule excuses: {missing}"
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    assert not [k for k in launched if _unreachable_reason(k)]
    assert C.UNREACHABLE == ()
    assert extra == expected_extra() and len(extra) == 30
    # the inverse half is reused at every degree and in both classes, never copied
    for cls, io in CLASSES:
        assert {f"k_mdntt_inv<{cls},{io},{logn}>" for logn in range(8, 13)} <= set(launched)
        assert {f"{k}<{cls},{io},{l1}>" for l1 in range(1, 5)
                for k in ("k_mdntt_inv_rows", "k_rnsmp_cols_inv")} <= set(launched)


@pytest.mark.parametrize("path", OLDER)
def test_the_older_libraries_do_not_grow(path):
    """The ten older libraries keep their ABI and kernels: the new entry points and the k_ksntt_*
    kernels are in the eleventh library only."""
    out = subprocess.run(["nm", "-D", "--defined-only", getattr(nttmul, path)],
                         capture_output=True, text=True, check=True).stdout
    assert not re.search(r"ksntt", out)
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "ksntt" in k]


def test_mirror_restates_the_selection_rules():
    for n in C.ALL_N:
        for bits, (cls, io) in zip((32, 64), CLASSES):
            if n <= 4096:
                logn = n.bit_length() - 1
                assert C.kernel_name("modup", n, bits) == \
                    f"k_mdntt_inv<{cls},{io},{logn}> + k_ksntt_fwd<{cls},{io},{logn}>"
            else:
                l1 = n.bit_length() - 13
                assert C.kernel_name("modup", n, bits) == (
                    f"k_mdntt_inv_rows<{cls},{io},{l1}> + k_rnsmp_cols_inv<{cls},{io},{l1}> + "
                    f"k_ksntt_cols_fwd<{cls},{io},{l1}> + k_ksntt_rows<{cls},{io},{l1}>")
            for comps in (1, 2):                                    # one kernel at every n
                assert C.kernel_name("mac", n, bits, comps) == f"k_ksntt_mac<{cls},{io},{comps}>"
            assert len(C.sequence("modup", n, bits)) + 1 + (2 if n <= 4096 else 4) == \
                C.launches(n)                                       # with mdntt_moddown's
    with pytest.raises(AssertionError):
        C.kernel_name("modup", 131072, 32)
    with pytest.raises(AssertionError):
        C.kernel_name("mac", 256, 32, 3)
    case = C.Up(64, 8192, 3, 3, 2, 2, True)
    assert C.kernels_of(case) == ["k_rns_check_range<u64>"] + C.sequence("modup", 8192, 64)
    case = C.Mac(32, 8192, 3, 3, 2, 2, 2, (5,), True)
    assert C.kernels_of(case) == ["k_rns_check_range<u32>"] * 2 + ["k_ksntt_mac<Arith32P,u32,2>"]
    # n = 256: 16 thread groups per workgroup, two polynomials each in the 32-bit inverse
    assert C.units_per_block(C.Up(32, 256, 33, 3, 2, 2)) == {
        "k_mdntt_inv<Arith32P,u32,8>": (32, 33, 256), "k_ksntt_fwd<Arith32P,u32,8>": (16, 33, 256)}
    assert C.units_per_block(C.Up(64, 65536, 3, 2, 2, 1)) == {
        "k_mdntt_inv_rows<Arith64,u64,4>": (1, 48, 4096),
        "k_rnsmp_cols_inv<Arith64,u64,4>": (1, 3, 65536),
        "k_ksntt_cols_fwd<Arith64,u64,4>": (1, 3, 65536),
        "k_ksntt_rows<Arith64,u64,4>": (1, 48, 4096)}
    # the inverse covers the L limbs of Q, the forward kernels the dnum (L + K) targets
    assert C.grid_rows(C.Up(32, 8192, 1, 5, 3, 2)) == {
        "k_mdntt_inv_rows<Arith32P,u32,1>": 5, "k_rnsmp_cols_inv<Arith32P,u32,1>": 5,
        "k_ksntt_cols_fwd<Arith32P,u32,1>": 24, "k_ksntt_rows<Arith32P,u32,1>": 24}
    mac = C.Mac(64, 256, 3, 2, 1, 3, 2, (1, 5, 25))
    assert C.units_per_block(mac) == {"k_ksntt_mac<Arith64,u64,2>": (4, 3, 256)}
    assert C.grid_rows(mac) == {"k_ksntt_mac<Arith64,u64,2>": 9}


def test_the_sub_batch_rule():
    """The chunk counts whole polynomials: the most whose y (L limbs) fits scratch_mb, never less
    than one; the column-passed sums go through up_hat and bound nothing; mac has no scratch."""
    for (bits, n, L, K, alpha, batch, want), case in zip(C.SUBBATCH, C.subbatch_cases()):
        got = C.chunks(case)
        assert got == list(want) and len(got) == 3 and sum(got) == batch and got[-1] < got[0]
        assert case.scratch_mb == 1
        assert len(C.chunks(case._replace(scratch_mb=0))) == 1      # the default scratch
        assert C.kernels_of(case) == C.sequence("modup", n, bits) * 3
    assert {n for _, n, *_ in C.SUBBATCH} == {4096, 65536}
    assert C.chunks(C.Up(32, 4096, 70, 60, 4, 15, False, 1)) == [1] * 70
    assert C.chunks(C.Up(32, 8192, 9, 8, 60, 8, False, 1)) == [4, 4, 1]
    assert C.chunks(C.Mac(32, 8192, 9, 8, 60, 1, 1, (5,))) == [9]


def test_the_cases_cover_what_the_issue_names():
    ups = C.modup_cases()
    for bits in (32, 64):
        mine = [c for c in ups if c.bits == bits]
        at = [c for c in mine if c.n == C.N]
        assert {(c.L, c.K, c.alpha) for c in at if c.batch in (3, 33)} == {
            (1, 1, 1), (4, 2, 2), (5, 2, 2), (5, 3, 5), (6, 1, 1), (3, 2, 2), (12, 4, 5)}
        assert {c.batch for c in at} == {1, 2, 3, 33}               # 2: the degree sweep's
        assert {(c.L, c.K, c.alpha) for c in at if c.batch == 1} == {(60, 4, 15)}
        cad = 2 if bits == 32 else 4
        assert C.CADENCE[bits] == cad and 5 % cad == 1 and 12 % 5 == 2   # a remainder, a short digit
        assert {c.n for c in mine if (c.L, c.K, c.alpha) == C.DEGREE_SHAPE and c.batch <= 2} == \
            set(C.ALL_N)
        assert all(c.batch == (1 if c.n == 65536 else 2) for c in mine
                   if (c.L, c.K, c.alpha) == C.DEGREE_SHAPE and c.n > 256)
        macs = [c for c in C.mac_cases() if c.bits == bits]
        assert {c.n for c in macs} == {256, 4096, 8192, 65536} and {c.batch for c in macs} == {3}
        for n in C.MAC_N:
            here = [c for c in macs if c.n == n]
            assert {c.ks for c in here} == {(1,), (5, 2 * n - 1, 25), C.rotations(n, 16)}
            assert {c.terms for c in here} == {1, 3} and {c.comps for c in here} == {1, 2}
            # both kernel instantiations see the identity and a real permutation
            assert {(c.comps, c.ks == (1,)) for c in here} == {(1, True), (1, False), (2, True),
                                                               (2, False)}
        assert {(c.n, c.terms) for c in C.mac_worst_cases() if c.bits == bits} == \
            {(n, 16) for n in C.MAC_N}
    assert 33 % 32 and 33 % 16 and 3 % 2                            # partial workgroups, a half pair
    assert C.RANGE_N == (256, 4096, 8192) and C.RANGE_FILLS == ("top", "worst", "zero")
    assert C.CHAIN_N == (256, 8192) and C.HOST == ((256, 5), (8192, 2))
    assert {(n, b) for n, b in C.FP_SIZES} == {(256, 1), (256, 33), (4096, 1), (8192, 1)}
    assert set(C.FP_SHAPES) == {(3, 2, 2), (5, 1, 5)}
    assert C.SCALE_N == (4096, 8192) and C.SCALE_SHAPE == (2, 1, 1) and C.SCALE_MAC_N == 4096
    for case in C.large_cases():
        per = C.out_polys(case) * case.n * (case.bits // 8)
        assert case.batch * per > 1 << 32 >= (case.batch - 1) * per
    assert {C.op_of(c) for c in C.large_cases()} == {"modup", "mac"}
    # the transform and launch counts the header and the documents state
    assert C.transforms(4, 2, 2, 3) == (2 * 6 + 6 * 6, 4 + 2 * 6 + 6 * 6 + 6 * 4)
    assert [C.launches(n, old) for n in (4096, 8192) for old in (False, True)] == [5, 6, 9, 10]


def test_the_scale_cases_meet_the_rule_of_scale_cases():
    import scale_cases as S
    assert (C.MIN_WAVES, C.WAVE) == (S.MIN_WAVES, S.WAVE)
    rows = C.scale_cases()
    assert {(C.op_of(c), c.bits, c.n) for c in rows} == \
        {("modup", b, n) for b in (32, 64) for n in C.SCALE_N} | \
        {("mac", b, C.SCALE_MAC_N) for b in (32, 64)}
    seen = set()
    for case in rows:
        assert len(C.chunks(case)) == 1
        waves = C.launch_waves(case)
        comps = getattr(case, "comps", 1)
        assert list(waves) == C.sequence(C.op_of(case), case.n, case.bits, comps)
        assert all(w >= S.MIN_WAVES for w in waves.values()), (case, waves)
        for key, (per, units, _) in C.units_per_block(case).items():
            # a partial last workgroup where one can exist: at n = 4096 a polynomial is four whole
            # workgroups of the mac
            assert per == 1 or units % per or key.startswith("k_ksntt_mac"), (case, key)
        less = case._replace(batch=case.batch - 1)
        assert (min(C.launch_waves(less).values()) < S.MIN_WAVES
                or any(per > 1 and units % per == 0
                       for per, units, _ in C.units_per_block(less).values()))
        seen |= set(waves)
    ours = {k for k in nttmul.kernel_hashes(nttmul.KSNTT_LIB_PATH) if k.startswith("k_ksntt_")}
    # one case per new kernel template and word class: the other degrees and the other component
    # count of a template lie between or beside the covered ones (scale_cases.SCALE_EXEMPT)
    assert {k.split(",")[0] for k in seen if k.startswith("k_ksntt_")} == \
        {k.split(",")[0] for k in ours}


def test_every_entry_point_that_writes_caller_memory_has_a_footprint_row():
    rows = C.footprint_cases()
    named = {f.entry for f in rows}
    writers = {s for s in nttmul.ksntt_exported_symbols()
               if re.fullmatch(r"nttmul_ksntt_(modup|mac)(_device)?", s)}
    assert len(writers) == 4 and named == writers
    assert set(nttmul.ksntt_exported_symbols()) - writers == {
        "nttmul_ksntt_create", "nttmul_ksntt_destroy", "nttmul_ksntt_last_error",
        "nttmul_ksntt_get_info", "nttmul_ksntt_kernel_name"}       # no caller operand is written
    for entry in writers:
        got = {(f.case.bits, f.case.n, f.case.batch, f.case.L, f.case.K) for f in rows
               if f.entry == entry}
        assert got == {(b, n, batch, L, K) for b in (32, 64) for n, batch in C.FP_SIZES
                       for L, K, _ in C.FP_SHAPES}
    assert all((f.host == "host") == (not f.entry.endswith("_device")) for f in rows)
    import guarded as G
    for f in rows:
        for per, units, words in C.units_per_block(f.case).values():
            assert C.fp_guard_words(f.case) >= max(per * words, G.guard_words(1))


def test_every_additional_kernel_is_launched_by_a_case_held_to_the_cpu_reference(mdntt, ksntt):
    """The mirror reports the cases whose every output word a GPU test compares with the CPU
    reference (referenced_cases(): at every n, tests/full_ref.py); the cases full_ref.SUBSET holds
    on a part of their batch only do not count, and are at most one in ten.  Every kernel this
    library adds over its predecessor is launched by one of the rest."""
    import full_ref
    cases = C.referenced_cases()
    assert cases and all(c in C.all_cases() for c in cases[:8] + cases[-8:])
    whole = [c for c in cases if not full_ref.on_subset("ksntt", c)]
    assert 10 * (len(cases) - len(whole)) <= len(cases)
    held = {k for c in whole for k in C.kernels_of(c)}
    excused = {k for k in ksntt if any(re.fullmatch(pat, k) for pat, _ in
                                        getattr(C, "UNREACHABLE", ()))}
    extra = set(ksntt) - set(mdntt)
    assert extra and sorted(extra - held - excused) == []
