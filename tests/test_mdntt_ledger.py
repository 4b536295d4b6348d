"""The kernel ledger of lib/libnttmul_mdntt.so, in the style of tests/test_hoist_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_mdntt.so = libnttmul_hoist.so's kernels, bit for bit, plus k_mdntt_inv and
k_mdntt_fwd at the five degrees up to 4096 and k_mdntt_inv_rows, k_mdntt_cols_fwd and k_mdntt_rows
at the four splits above, in both word classes (44 kernels), and every one is launched by a case
of tests/mdntt_cases.py (whose mirror test_gpu_mdntt.py anchors to the library's kernel_name entry
point on the GPU)."""
import re
import subprocess

import pytest

import mdntt_cases as C
import nttmul

OLDER = ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
         "GALOIS_LIB_PATH", "KS_LIB_PATH", "MACN_LIB_PATH", "HOIST_LIB_PATH"]


@pytest.fixture(scope="module")
def hoist():
    return nttmul.kernel_hashes(nttmul.HOIST_LIB_PATH)


@pytest.fixture(scope="module")
def mdntt():
    return nttmul.kernel_hashes(nttmul.MDNTT_LIB_PATH)


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


def test_common_kernels_are_the_hoist_librarys_bit_for_bit(hoist, mdntt):
    assert len(hoist) > 269 + 56 + 9 + 2 + 18 + 36
    assert sorted(set(hoist) - set(mdntt)) == []
    assert {k: mdntt[k] for k in hoist} == hoist


def test_the_additional_kernels_are_exactly_what_the_cases_launch(hoist, mdntt):
    extra = set(mdntt) - set(hoist)
    launched = _launched()
    ours = {k for k in launched if k.startswith("k_mdntt_")}
    # the range check and the inverse column pass
    assert all(k in hoist for k in set(launched) - ours)
    assert {k.split("<")[0] for k in set(launched) - ours} == {
        "k_rns_check_range", "k_rnsmp_cols_inv"}
    missing = sorted(k for k in extra if k not in launched and not _unreachable_reason(k))
    assert not missing, f"kernels no case launches and no rule excuses: {missing}"
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    assert not [k for k in launched if _unreachable_reason(k)]
    assert C.UNREACHABLE == ()
    classes = (("Arith32P", "u32"), ("Arith64", "u64"))
    want = {f"{k}<{cls},{io},{logn}>" for cls, io in classes for logn in range(8, 13)
            for k in ("k_mdntt_inv", "k_mdntt_fwd")}
    want |= {f"{k}<{cls},{io},{l1}>" for cls, io in classes for l1 in range(1, 5)
             for k in ("k_mdntt_inv_rows", "k_mdntt_cols_fwd", "k_mdntt_rows")}
    assert extra == want and len(extra) == 44


@pytest.mark.parametrize("path", OLDER)
def test_the_older_libraries_do_not_grow(path):
    """The nine older libraries keep their ABI and kernels: the new entry points and the k_mdntt_*
    kernels are in the tenth library only."""
    out = subprocess.run(["nm", "-D", "--defined-only", getattr(nttmul, path)],
                         capture_output=True, text=True, check=True).stdout
    assert not re.search(r"mdntt", out)
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "mdntt" in k]


def test_mirror_restates_the_selection_rules():
    for n in C.ALL_N:
        for bits, cls, io in ((32, "Arith32P", "u32"), (64, "Arith64", "u64")):
            if n <= 4096:
                logn = n.bit_length() - 1
                assert C.kernel_name(n, bits) == \
                    f"k_mdntt_inv<{cls},{io},{logn}> + k_mdntt_fwd<{cls},{io},{logn}>"
            else:
                l1 = n.bit_length() - 13
                assert C.kernel_name(n, bits) == (
                    f"k_mdntt_inv_rows<{cls},{io},{l1}> + k_rnsmp_cols_inv<{cls},{io},{l1}> + "
                    f"k_mdntt_cols_fwd<{cls},{io},{l1}> + k_mdntt_rows<{cls},{io},{l1}>")
    with pytest.raises(AssertionError):
        C.kernel_name(131072, 32)
    case = C.Case(64, 8192, 3, 2, 1, True)
    assert C.kernels_of(case) == ["k_rns_check_range<u64>"] + C.sequence(8192, 64)
    # n = 256: 16 thread groups per workgroup, two polynomials each in the 32-bit inverse
    assert C.units_per_block(C.Case(32, 256, 33, 3, 2)) == {
        "k_mdntt_inv<Arith32P,u32,8>": (32, 33, 256), "k_mdntt_fwd<Arith32P,u32,8>": (16, 33, 256)}
    assert C.units_per_block(C.Case(64, 256, 33, 3, 2)) == {
        "k_mdntt_inv<Arith64,u64,8>": (16, 33, 256), "k_mdntt_fwd<Arith64,u64,8>": (16, 33, 256)}
    assert C.units_per_block(C.Case(64, 65536, 3, 2, 2)) == {
        "k_mdntt_inv_rows<Arith64,u64,4>": (1, 48, 4096),
        "k_rnsmp_cols_inv<Arith64,u64,4>": (1, 3, 65536),
        "k_mdntt_cols_fwd<Arith64,u64,4>": (1, 3, 65536),
        "k_mdntt_rows<Arith64,u64,4>": (1, 48, 4096)}
    assert C.grid_rows(C.Case(32, 8192, 1, 5, 3)) == {
        "k_mdntt_inv_rows<Arith32P,u32,1>": 3, "k_rnsmp_cols_inv<Arith32P,u32,1>": 3,
        "k_mdntt_cols_fwd<Arith32P,u32,1>": 5, "k_mdntt_rows<Arith32P,u32,1>": 5}


def test_the_sub_batch_rule():
    """The chunk counts whole polynomials: the most whose y (K limbs) and, above n = 4096, t (L
    limbs) fit scratch_mb, never less than one."""
    for (bits, n, L, K, batch, want), case in zip(C.SUBBATCH, C.subbatch_cases()):
        got = C.chunks(case)
        assert got == list(want) and len(got) == 3 and sum(got) == batch
        assert case.scratch_mb == 1
        assert len(C.chunks(case._replace(scratch_mb=0))) == 1      # the default scratch
        assert C.kernels_of(case) == C.sequence(n, bits) * 3
    assert C.SUBBATCH[0][5][-1] < C.SUBBATCH[0][5][0]               # a partial last sub-batch
    bits, n, L, K = C.SUBBATCH[1][:4]
    assert max(L, K) * n * bits // 8 >= 1 << 20                     # one polynomial fills the limit
    # up to n = 4096 only y counts, above it the larger of y and t
    assert C.chunks(C.Case(32, 4096, 70, 60, 1, False, 1)) == [64, 6]
    assert C.chunks(C.Case(32, 8192, 9, 8, 1, False, 1)) == [4, 4, 1]


def test_the_cases_cover_what_the_issue_names():
    cases = C.parity_cases()
    for bits in (32, 64):
        mine = [c for c in cases if c.bits == bits and not c.moduli]
        at = [c for c in mine if c.n == C.N]
        assert {(c.L, c.K) for c in at if c.batch in (3, 33)} == {
            (1, 1), (4, 1), (4, 2), (3, 2), (5, 3), (12, 4)}
        assert {c.batch for c in at} == {1, 2, 3, 33}               # 2: the degree sweep's
        assert {(c.L, c.K) for c in at if c.batch == 1} >= {(60, 4), (1, 63)}
        assert {c.K for c in at if c.batch == 1 and c.L == 2} == set(C.CADENCE_K[bits])
        cad = 2 if bits == 32 else 4
        assert C.CADENCE[bits] == cad
        ks = C.CADENCE_K[bits]
        assert min(ks) < cad and cad in ks and cad + 1 in ks        # both sides of the cadence
        assert max(ks) >= (5 if bits == 32 else 17)                 # past the unfolded overflow
        assert {c.n for c in mine if (c.L, c.K) == C.DEGREE_SHAPE and c.batch <= 2} == set(C.ALL_N)
        assert all(c.batch == (1 if c.n == 65536 else 2) for c in mine
                   if (c.L, c.K) == C.DEGREE_SHAPE and c.n > 256)
    assert [c for c in cases if c.moduli == "small"] == [C.Case(32, 256, 3, 4, 2, False, 0, "small")]
    assert 33 % 32 and 33 % 16 and 3 % 2                            # partial workgroups, a half pair
    assert C.RANGE_N == (256, 4096, 8192) and C.RANGE_FILLS == ("top", "zero_p", "zero_q")
    assert set(C.RESCALE) == {(256, 1), (256, 3), (8192, 1), (8192, 3)}
    assert {(n, b) for n, b in C.FP_SIZES} == {(256, 1), (256, 33), (4096, 1), (8192, 1)}
    assert set(C.FP_SHAPES) == {(3, 2), (5, 1)}
    assert C.SCALE_N == (4096, 8192) and C.SCALE_SHAPE == (2, 1)
    assert {(b, n) for b, n, _, _ in C.LARGE} == {(32, 4096), (64, 65536)}
    for bits, n, L, K in C.LARGE:
        batch = C.large_batch(bits, n, L, K)
        assert batch * (L + K) * n * (bits // 8) > 1 << 32 >= (batch - 1) * (L + K) * n * (bits // 8)


def test_the_scale_cases_meet_the_rule_of_scale_cases():
    import scale_cases as S
    assert (C.MIN_WAVES, C.WAVE) == (S.MIN_WAVES, S.WAVE)
    rows = C.scale_cases()
    assert {(c.bits, c.n) for c in rows} == {(b, n) for b in (32, 64) for n in C.SCALE_N}
    seen = set()
    for case in rows:
        assert len(C.chunks(case)) == 1
        waves = C.launch_waves(case)
        assert list(waves) == C.sequence(case.n, case.bits)
        assert all(w >= S.MIN_WAVES for w in waves.values()), (case, waves)
        for key, (per, units, _) in C.units_per_block(case).items():
            assert per == 1 or units % per, (case, key)
        # the smallest such batch: one polynomial fewer misses the rule
        less = case._replace(batch=case.batch - 1)
        assert (min(C.launch_waves(less).values()) < S.MIN_WAVES
                or any(per > 1 and units % per == 0
                       for per, units, _ in C.units_per_block(less).values()))
        seen |= set(waves)
    ours = {k for k in nttmul.kernel_hashes(nttmul.MDNTT_LIB_PATH) if k.startswith("k_mdntt_")}
    # one case per new kernel template and word class: the other degrees of a template lie
    # between or beside the covered ones (scale_cases.SCALE_EXEMPT's reason for its twins)
    assert {k.split(",")[0] for k in seen if k.startswith("k_mdntt_")} == \
        {k.split(",")[0] for k in ours}


def test_every_entry_point_that_writes_caller_memory_has_a_footprint_row():
    rows = C.footprint_cases()
    named = {f.entry for f in rows}
    writers = {s for s in nttmul.mdntt_exported_symbols()
               if re.fullmatch(r"nttmul_mdntt_moddown(_device)?", s)}
    assert len(writers) == 2 and named == writers
    assert set(nttmul.mdntt_exported_symbols()) - writers == {
        "nttmul_mdntt_create", "nttmul_mdntt_destroy", "nttmul_mdntt_last_error",
        "nttmul_mdntt_get_info", "nttmul_mdntt_kernel_name"}       # no caller operand is written
    for entry in writers:
        got = {(f.case.bits, f.case.n, f.case.batch, f.case.L, f.case.K) for f in rows
               if f.entry == entry}
        assert got == {(b, n, batch, L, K) for b in (32, 64) for n, batch in C.FP_SIZES
                       for L, K in C.FP_SHAPES}
    assert all((f.host == "host") == (not f.entry.endswith("_device")) for f in rows)
    import guarded as G
    for f in rows:
        for per, units, words in C.units_per_block(f.case).values():
            assert C.fp_guard_words(f.case) >= max(per * words, G.guard_words(1))


def test_every_additional_kernel_is_launched_by_a_case_held_to_the_cpu_reference(hoist, mdntt):
    """The mirror reports the cases whose every output word a GPU test compares with the CPU
    reference (referenced_cases(): at every n, tests/full_ref.py); the cases full_ref.SUBSET holds
    on a part of their batch only do not count, and are at most one in ten.  Every kernel this
    library adds over its predecessor is launched by one of the rest."""
    import full_ref
    cases = C.referenced_cases()
    assert cases and all(c in C.all_cases() for c in cases[:8] + cases[-8:])
    whole = [c for c in cases if not full_ref.on_subset("mdntt", c)]
    assert 10 * (len(cases) - len(whole)) <= len(cases)
    held = {k for c in whole for k in C.kernels_of(c)}
    excused = {k for k in mdntt if any(re.fullmatch(pat, k) for pat, _ in
                                        getattr(C, "UNREACHABLE", ()))}
    extra = set(mdntt) - set(hoist)
    assert extra and sorted(extra - held - excused) == []
