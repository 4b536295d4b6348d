"""The kernel ledger of lib/libnttmul_level.so, in the style of tests/test_xconv_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_level.so = libnttmul_xconv.so's kernels, bit for bit, plus k_level_mac
(comps 1, 2), k_level_lintrans (comps 1, 2, unweighted and weighted), k_level_relin and
k_level_check_range in both word classes (16 kernels), and every one is launched by a case of
tests/level_cases.py (whose mirror test_gpu_level.py anchors to the library's kernel_name entry
point on the GPU)."""
import re
import subprocess

import pytest

import level_cases as C
import nttmul

OLDER = ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
         "GALOIS_LIB_PATH", "KS_LIB_PATH", "MACN_LIB_PATH", "HOIST_LIB_PATH", "MDNTT_LIB_PATH",
         "KSNTT_LIB_PATH", "LINTRANS_LIB_PATH", "CTMUL_LIB_PATH", "XCONV_LIB_PATH"]


@pytest.fixture(scope="module")
def xconv():
    return nttmul.kernel_hashes(nttmul.XCONV_LIB_PATH)


@pytest.fixture(scope="module")
def level():
    return nttmul.kernel_hashes(nttmul.LEVEL_LIB_PATH)


def _launched():
    out = {}
    for case in C.all_cases():
        for key in C.kernels_of(case):
            out.setdefault(key, case)
    return out


def test_common_kernels_are_the_xconv_librarys_bit_for_bit(xconv, level):
    assert len(xconv) > 400
    assert sorted(set(xconv) - set(level)) == []
    assert {k: level[k] for k in xconv} == xconv


def test_the_dense_kernels_the_views_copy_are_still_there_unchanged(xconv, level):
    """The view kernels are copies, not a shared template: the dense three keep their hashes."""
    dense = [k for k in xconv if re.match(r"k_(ksntt_mac|lintrans|ctmul_relin)<", k)]
    assert len(dense) == 4 + 8 + 2
    assert all(level[k] == xconv[k] for k in dense)


def test_the_additional_kernels_are_exactly_what_the_cases_launch(xconv, level):
    extra = set(level) - set(xconv)
    launched = _launched()
    ours = {k for k in launched if k.startswith("k_level_")}
    # the range check of the dense operands is libnttmul_rns.so's
    assert all(k in xconv for k in set(launched) - ours)
    assert {k.split("<")[0] for k in set(launched) - ours} == {"k_rns_check_range"}
    missing = sorted(k for k in extra if k not in launched)
    assert not missing, f"kernels no case launches: {missing}"
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    assert C.UNREACHABLE == ()
    classes = (("Arith32P", "u32"), ("Arith64", "u64"))
    want = {f"k_level_mac<{cls},{io},{c}>" for cls, io in classes for c in (1, 2)}
    want |= {f"k_level_lintrans<{cls},{io},{c},{w}>" for cls, io in classes for c in (1, 2)
             for w in (0, 1)}
    want |= {f"k_level_relin<{cls},{io}>" for cls, io in classes}
    want |= {f"k_level_check_range<{io}>" for _, io in classes}
    assert extra == want and len(extra) == 16


@pytest.mark.parametrize("path", OLDER)
def test_the_older_libraries_do_not_grow(path):
    """The fourteen older libraries keep their ABI and kernels: the new entry points and the
    k_level_* kernels are in the fifteenth library only."""
    out = subprocess.run(["nm", "-D", "--defined-only", getattr(nttmul, path)],
                         capture_output=True, text=True, check=True).stdout
    assert not re.search(r"nttmul_level|_view\b|k_level", out)
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "level" in k]


def test_mirror_restates_the_selection_rules():
    for bits, cls, io in ((32, "Arith32P", "u32"), (64, "Arith64", "u64")):
        for n in C.ALL_N:
            logn = n.bit_length() - 1
            for comps in C.COMPS:
                case = C.Case("mac", bits, n, 3, 3, comps, 3)
                assert C.kernel_name(case) == f"k_level_mac<{cls},{io},{comps}>" == \
                    nttmul.level_kernel_name("mac", logn, bits, comps)
                for w in (False, True):
                    case = C.Case("lintrans", bits, n, 3, 3, comps, 3, w, True)
                    assert C.kernel_name(case) == \
                        f"k_level_lintrans<{cls},{io},{comps},{int(w)}>" == \
                        nttmul.level_kernel_name("lintrans", logn, bits, comps, w)
            case = C.Case("relin", bits, n, 3, 3, 2, 1, pairs=3)
            assert C.kernel_name(case) == f"k_level_relin<{cls},{io}>" == \
                nttmul.level_kernel_name("relin", logn, bits)
    case = C.Case("lintrans", 64, 256, 5, 3, 2, 3, True, True, validate=True)
    assert C.kernels_of(case) == ["k_rns_check_range<u64>", "k_level_check_range<u64>",
                                  "k_level_check_range<u64>", "k_rns_check_range<u64>",
                                  "k_level_lintrans<Arith64,u64,2,1>"]
    case = C.Case("relin", 32, 256, 5, 3, 2, 1, validate=True)
    assert C.kernels_of(case) == ["k_rns_check_range<u32>", "k_level_check_range<u32>",
                                  "k_rns_check_range<u32>", "k_rns_check_range<u32>",
                                  "k_level_relin<Arith32P,u32>"]
    assert C.units_per_block(C.Case("mac", 32, 512, 3, 4, 1, 3)) == {
        "k_level_mac<Arith32P,u32,1>": (4, 6)}
    assert C.launch_waves(C.Case("relin", 64, 8192, 3, 4, 2, 1)) == {
        "k_level_relin<Arith64,u64>": 1 * 32 * 6 * 4}


def test_the_cases_cover_what_the_issue_names():
    cases = C.parity_cases()
    assert (C.L_TOP, C.K, C.ALPHA, C.TOP_TERMS) == (5, 2, 2, 3) and C.VIEW == (5, 3)
    assert C.LEVELS == (5, 4, 3, 1) and C.ALL_N == (256, 512, 8192)
    assert [C.terms_of(L) for L in C.LEVELS] == [3, 2, 2, 1]
    assert [C.alpha_of(L) for L in C.LEVELS] == [2, 2, 2, 1]
    for bits in (32, 64):
        q, p = C.chain_bases(bits)
        assert (len(q), len(p)) == (5, 2) and list(q) != sorted(q)          # unsorted limb sizes
        assert max(q).bit_length() - min(q).bit_length() >= 5               # and mixed
        for n in C.ALL_N:
            for L in C.LEVELS:
                mine = [c for c in cases if (c.bits, c.n, c.L) == (bits, n, L)]
                assert {c.batch for c in mine} == {5 if n == 256 else 3}
                assert {(c.comps, c.rots) for c in mine if c.op == "mac"} == \
                    {(c, r) for c in (1, 2) for r in (1, 3)}
                assert {(c.comps, c.rots, c.weighted, c.c0) for c in mine
                        if c.op == "lintrans"} == \
                    {(c, r, w, z) for c in (1, 2) for r in (1, 3) for w in (False, True)
                     for z in (False, True)}
                assert {c.pairs for c in mine if c.op == "relin"} == {1, 3}
            for rots in C.ROTS:
                ks = C.ks_of(n, rots)
                assert len(set(ks)) == rots and 1 not in ks
                assert all(k % 2 == 1 and 0 < k < 2 * n for k in ks)
    # a partial last workgroup for V = 4 wherever the batch can give one
    assert all(C.ends_partial(c) for c in cases if c.op != "mac" or c.n <= 512)
    assert C.CHAIN_N == (256, 8192) and C.CHAIN_LEVEL == 3


def test_the_scale_cases_meet_the_rule_of_scale_cases(level):
    import scale_cases as S
    assert (C.MIN_WAVES, C.WAVE) == (S.MIN_WAVES, S.WAVE)
    rows = C.scale_cases()
    seen = set()
    for case in rows:
        waves = C.launch_waves(case)
        assert list(waves) == [C.kernel_name(case)]
        assert all(w >= S.MIN_WAVES for w in waves.values()), (case, waves)
        assert C.ends_partial(case)
        smaller = case._replace(batch=case.batch - C.V)
        assert min(C.launch_waves(smaller).values()) < S.MIN_WAVES          # the smallest batch
        seen |= set(waves)
    ours = {k for k in level if k.startswith("k_level_") and "check_range" not in k}
    # one row per new kernel template and word class
    tmpl = lambda k: tuple(k.split(",")[:2])
    assert {tmpl(k) for k in seen} == {tmpl(k) for k in ours} and len(rows) == 6


def test_every_entry_point_that_writes_caller_memory_has_a_footprint_row():
    rows = C.footprint_cases()
    named = {f.entry for f in rows}
    writers = set(nttmul.level_exported_symbols()) - {"nttmul_level_kernel_name"}
    assert len(writers) == 6 and named == writers
    for entry in writers:
        got = {(f.case.bits, f.case.n, f.case.batch) for f in rows if f.entry == entry}
        assert got == {(b, n, batch) for b in (32, 64) for n, batch in C.FP_SIZES}
    assert all((f.host == "host") == (not f.entry.endswith("_device")) for f in rows)
    assert all(f.case.L < C.L_TOP for f in rows)


def test_every_additional_kernel_is_launched_by_a_case_held_to_the_cpu_reference(xconv, level):
    """The mirror reports the cases whose every output word a GPU test compares with the CPU
    reference (referenced_cases(): at every n, tests/full_ref.py); the cases full_ref.SUBSET holds
    on a part of their batch only do not count, and are at most one in ten.  Every kernel this
    library adds over its predecessor is launched by one of the rest."""
    import full_ref
    cases = C.referenced_cases()
    assert cases and all(c in C.all_cases() for c in cases[:8] + cases[-8:])
    whole = [c for c in cases if not full_ref.on_subset("level", c)]
    assert 10 * (len(cases) - len(whole)) <= len(cases)
    held = {k for c in whole for k in C.kernels_of(c)}
    excused = {k for k in level if any(re.fullmatch(pat, k) for pat, _ in
                                        getattr(C, "UNREACHABLE", ()))}
    extra = set(level) - set(xconv)
    assert extra and sorted(extra - held - excused) == []
