"""The kernel ledger of lib/libnttmul_xconv.so, in the style of tests/test_mdntt_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_xconv.so = libnttmul_ctmul.so's kernels, bit for bit, plus k_xconv_fwd for
both operations at the five degrees up to 4096 and k_xconv_cols_fwd and k_xconv_rows at the four
splits above, in both word classes (36 kernels), and every one is launched by a case of
tests/xconv_cases.py (whose mirror test_gpu_xconv.py anchors to the library's kernel_name entry
point on the GPU)."""
import re
import subprocess

import pytest

import nttmul
import xconv_cases as C

OLDER = ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
         "GALOIS_LIB_PATH", "KS_LIB_PATH", "MACN_LIB_PATH", "HOIST_LIB_PATH", "MDNTT_LIB_PATH",
         "KSNTT_LIB_PATH", "LINTRANS_LIB_PATH", "CTMUL_LIB_PATH"]


@pytest.fixture(scope="module")
def ctmul():
    return nttmul.kernel_hashes(nttmul.CTMUL_LIB_PATH)


@pytest.fixture(scope="module")
def xconv():
    return nttmul.kernel_hashes(nttmul.XCONV_LIB_PATH)


def _launched():
    out = {}
    for case in C.all_cases():
        for key in C.kernels_of(case):
            out.setdefault(key, case)
    return out


def test_common_kernels_are_the_ctmul_librarys_bit_for_bit(ctmul, xconv):
    assert len(ctmul) > 400
    assert sorted(set(ctmul) - set(xconv)) == []
    assert {k: xconv[k] for k in ctmul} == ctmul


def test_the_additional_kernels_are_exactly_what_the_cases_launch(ctmul, xconv):
    extra = set(xconv) - set(ctmul)
    launched = _launched()
    ours = {k for k in launched if k.startswith("k_xconv_")}
    # the range check, mdntt.hip's inverse half and moddown's row pass, rnsmp.hip's column pass
    assert all(k in ctmul for k in set(launched) - ours)
    assert {k.split("<")[0] for k in set(launched) - ours} == {
        "k_rns_check_range", "k_mdntt_inv", "k_mdntt_inv_rows", "k_rnsmp_cols_inv", "k_mdntt_rows"}
    missing = sorted(k for k in extra if k not in launched)
    assert not missing, f"kernels no case launches: {missing}"
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    assert C.UNREACHABLE == ()
    classes = (("Arith32P", "u32"), ("Arith64", "u64"))
    want = {f"k_xconv_fwd<{cls},{io},{logn},{op}>" for cls, io in classes
            for logn in range(8, 13) for op in (0, 1)}
    want |= {f"{k}<{cls},{io},{l1}>" for cls, io in classes for l1 in range(1, 5)
             for k in ("k_xconv_cols_fwd", "k_xconv_rows")}
    assert extra == want and len(extra) == 36


@pytest.mark.parametrize("path", OLDER)
def test_the_older_libraries_do_not_grow(path):
    """The thirteen older libraries keep their ABI and kernels: the new entry points and the
    k_xconv_* kernels are in the fourteenth library only."""
    out = subprocess.run(["nm", "-D", "--defined-only", getattr(nttmul, path)],
                         capture_output=True, text=True, check=True).stdout
    assert not re.search(r"xconv", out)
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "xconv" in k]


def test_mirror_restates_the_selection_rules():
    for n in C.ALL_N:
        for bits, cls, io in ((32, "Arith32P", "u32"), (64, "Arith64", "u64")):
            for i, op in enumerate(C.OPS):
                if n <= 4096:
                    logn = n.bit_length() - 1
                    assert C.kernel_name(op, n, bits) == \
                        f"k_mdntt_inv<{cls},{io},{logn}> + k_xconv_fwd<{cls},{io},{logn},{i}>"
                else:
                    l1 = n.bit_length() - 13
                    last = ("k_xconv_rows", "k_mdntt_rows")[i]
                    assert C.kernel_name(op, n, bits) == (
                        f"k_mdntt_inv_rows<{cls},{io},{l1}> + k_rnsmp_cols_inv<{cls},{io},{l1}> + "
                        f"k_xconv_cols_fwd<{cls},{io},{l1}> + {last}<{cls},{io},{l1}>")
    with pytest.raises(AssertionError):
        C.kernel_name("moddown", 131072, 32)
    case = C.Case("extend", 64, 8192, 3, 2, 1, 1, True)
    assert C.kernels_of(case) == ["k_rns_check_range<u64>"] + C.sequence("extend", 8192, 64)
    assert C.units_per_block(C.Case("moddown", 32, 256, 33, 3, 2)) == {
        "k_mdntt_inv<Arith32P,u32,8>": (32, 33, 256), "k_xconv_fwd<Arith32P,u32,8,1>": (16, 33, 256)}
    assert C.grid_rows(C.Case("extend", 32, 8192, 1, 5, 3)) == {
        "k_mdntt_inv_rows<Arith32P,u32,1>": 3, "k_rnsmp_cols_inv<Arith32P,u32,1>": 3,
        "k_xconv_cols_fwd<Arith32P,u32,1>": 5, "k_xconv_rows<Arith32P,u32,1>": 5}


def test_the_sub_batch_rule():
    for case in C.subbatch_cases():
        want = [w for *_, w in C.SUBBATCH if sum(w) == case.batch][0]
        got = C.chunks(case)
        assert got == list(want) and len(got) == 3 and case.scratch_mb == 1
        assert len(C.chunks(case._replace(scratch_mb=0))) == 1
        assert C.kernels_of(case) == C.sequence(case.op, case.n, case.bits) * 3


def test_the_cases_cover_what_the_issue_names():
    cases = C.parity_cases()
    for op in C.OPS:
        for bits in (32, 64):
            for t in C.SCALES:
                mine = [c for c in cases if (c.op, c.bits, c.t) == (op, bits, t)]
                at = [c for c in mine if c.n == C.N]
                assert {(c.L, c.K) for c in at if c.batch in (3, 33)} == set(C.SHAPES)
                assert {(c.L, c.K) for c in at if c.batch == 1} >= set(C.WIDE)
                ks = {c.K for c in at if c.batch == 1 and c.L == C.CADENCE_L}
                assert ks == set(C.CADENCE_K[bits])
                cad = C.CADENCE[bits]
                # K + 1 products: below, at and above the cadence, and past the unfolded overflow
                assert {k + 1 for k in ks} >= {cad, cad + 1} and min(ks) + 1 <= cad
                assert max(ks) + 1 >= (5 if bits == 32 else 17)
                assert {c.n for c in mine if (c.L, c.K) == C.DEGREE_SHAPE and c.batch <= 2} == \
                    set(C.ALL_N)
                assert all(c.batch == (1 if c.n == 65536 else 2) for c in mine
                           if (c.L, c.K) == C.DEGREE_SHAPE and c.n > 256)
    assert C.SCALES == (1, 65537) and C.EDGE_N == (256, 8192) and C.EDGE_K == (1, 2, 5)
    assert C.CHAIN_N == (256, 8192)
    # the sample the scale file keeps: tests/test_full_ref.py holds its definition
    assert set(C.parity_cases()) <= set(C.referenced_cases())


def test_the_scale_cases_meet_the_rule_of_scale_cases():
    import scale_cases as S
    assert (C.MIN_WAVES, C.WAVE) == (S.MIN_WAVES, S.WAVE)
    rows = C.scale_cases()
    seen = set()
    for case in rows:
        assert len(C.chunks(case)) == 1
        waves = C.launch_waves(case)
        assert list(waves) == C.sequence(case.op, case.n, case.bits)
        assert all(w >= S.MIN_WAVES for w in waves.values()), (case, waves)
        for key, (per, units, _) in C.units_per_block(case).items():
            assert per == 1 or units % per, (case, key)
        seen |= set(waves)
    ours = {k for k in nttmul.kernel_hashes(nttmul.XCONV_LIB_PATH) if k.startswith("k_xconv_")}
    # one case per new kernel template (the operation is one of k_xconv_fwd's arguments) and class
    tmpl = lambda k: (k.split(",")[0], k.split(",")[3] if k.startswith("k_xconv_fwd") else "")
    assert {tmpl(k) for k in seen if k.startswith("k_xconv_")} == {tmpl(k) for k in ours}


def test_every_entry_point_that_writes_caller_memory_has_a_footprint_row():
    rows = C.footprint_cases()
    named = {f.entry for f in rows}
    writers = {s for s in nttmul.xconv_exported_symbols()
               if re.fullmatch(r"nttmul_xconv_(extend|moddown)(_device)?", s)}
    assert len(writers) == 4 and named == writers
    assert set(nttmul.xconv_exported_symbols()) - writers == {
        "nttmul_xconv_create", "nttmul_xconv_destroy", "nttmul_xconv_last_error",
        "nttmul_xconv_get_info", "nttmul_xconv_kernel_name", "nttmul_xconv_plan"}
    for entry in writers:
        got = {(f.case.bits, f.case.n, f.case.batch, f.case.L, f.case.K) for f in rows
               if f.entry == entry}
        assert got == {(b, n, batch, L, K) for b in (32, 64) for n, batch in C.FP_SIZES
                       for L, K in C.FP_SHAPES}
    assert all((f.host == "host") == (not f.entry.endswith("_device")) for f in rows)


def test_every_additional_kernel_is_launched_by_a_case_held_to_the_cpu_reference(ctmul, xconv):
    """The mirror reports the cases whose every output word a GPU test compares with the CPU
    reference (referenced_cases(): at every n, tests/full_ref.py); the cases full_ref.SUBSET holds
    on a part of their batch only do not count, and are at most one in ten.  Every kernel this
    library adds over its predecessor is launched by one of the rest."""
    import full_ref
    cases = C.referenced_cases()
    assert cases and all(c in C.all_cases() for c in cases[:8] + cases[-8:])
    whole = [c for c in cases if not full_ref.on_subset("xconv", c)]
    assert 10 * (len(cases) - len(whole)) <= len(cases)
    held = {k for c in whole for k in C.kernels_of(c)}
    excused = {k for k in xconv if any(re.fullmatch(pat, k) for pat, _ in
                                        getattr(C, "UNREACHABLE", ()))}
    extra = set(xconv) - set(ctmul)
    assert extra and sorted(extra - held - excused) == []
