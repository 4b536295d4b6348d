"""The kernel ledger of lib/libnttmul_hoist.so, in the style of tests/test_macn_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_hoist.so = libnttmul_macn.so's kernels, bit for bit, plus
k_rns_hoist<*,*,*,{1,2}> at the five degrees up to 4096 and k_rnsmp_hoist<*,*,*,{1,2}> at the four
splits above, in both word classes (36 kernels), and every one is launched by a case of
tests/hoist_cases.py (whose mirror test_gpu_hoist.py anchors to the library's kernel_name entry
points on the GPU)."""
import re
import subprocess

import pytest

import hoist_cases as C
import nttmul
import rnsmp_cases as M

OLDER = ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
         "GALOIS_LIB_PATH", "KS_LIB_PATH", "MACN_LIB_PATH"]


@pytest.fixture(scope="module")
def macn():
    return nttmul.kernel_hashes(nttmul.MACN_LIB_PATH)


@pytest.fixture(scope="module")
def hoist():
    return nttmul.kernel_hashes(nttmul.HOIST_LIB_PATH)


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


def test_common_kernels_are_the_macn_librarys_bit_for_bit(macn, hoist):
    assert len(macn) > 269 + 56 + 9 + 2 + 18
    assert sorted(set(macn) - set(hoist)) == []
    assert {k: hoist[k] for k in macn} == macn


def test_the_additional_kernels_are_exactly_what_the_cases_launch(macn, hoist):
    extra = set(hoist) - set(macn)
    launched = _launched()
    ours = {k for k in launched if re.match(r"k_rns(mp)?_hoist<", k)}
    # the range check and the inverse column pass
    assert all(k in macn for k in set(launched) - ours)
    assert {k.split("<")[0] for k in set(launched) - ours} == {
        "k_rns_check_range", "k_rnsmp_cols_inv"}
    missing = sorted(k for k in extra if k not in launched and not _unreachable_reason(k))
    assert not missing, f"kernels no case launches and no rule excuses: {missing}"
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    assert not [k for k in launched if _unreachable_reason(k)]
    assert C.UNREACHABLE == ()
    classes = (("Arith32P", "u32"), ("Arith64", "u64"))
    want = {f"k_rns_hoist<{cls},{io},{logn},{comps}>" for cls, io in classes
            for logn in range(8, 13) for comps in (1, 2)}
    want |= {f"k_rnsmp_hoist<{cls},{io},{l1},{comps}>" for cls, io in classes
             for l1 in range(1, 5) for comps in (1, 2)}
    assert extra == want and len(extra) == 36


@pytest.mark.parametrize("path", OLDER)
def test_the_older_libraries_do_not_grow(path):
    """The eight older libraries keep their ABI and kernels: the new entry points and the hoist
    kernels are in the ninth library only."""
    out = subprocess.run(["nm", "-D", "--defined-only", getattr(nttmul, path)],
                         capture_output=True, text=True, check=True).stdout
    assert not re.search(r"_hoist", out)
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "_hoist" in k]


def test_mirror_restates_the_selection_rules():
    for n in C.ALL_N:
        for moduli, cls, io in ((C.cases_of(n).BASIS32, "Arith32P", "u32"),
                                (C.cases_of(n).BASIS64, "Arith64", "u64")):
            for comps in (1, 2):
                if n <= 4096:
                    logn = n.bit_length() - 1
                    assert C.kernel_name(n, moduli, comps) == \
                        f"k_rns_hoist<{cls},{io},{logn},{comps}>"
                else:
                    l1 = n.bit_length() - 13
                    assert C.kernel_name(n, moduli, comps) == (
                        f"k_rnsmp_hoist<{cls},{io},{l1},{comps}> + "
                        f"k_rnsmp_cols_inv<{cls},{io},{l1}>")
            for comps in (0, 3):
                with pytest.raises(AssertionError):
                    C.kernel_name(n, moduli, comps)
    with pytest.raises(AssertionError):
        C.kernel_name(131072, M.BASIS32, 2)
    case = C.Case(8192, M.BASIS64, 3, 2, 2, (5, 25), True)
    assert C.kernels_of(case) == ["k_rns_check_range<u64>"] * 2 + C.sequence(8192, M.BASIS64, 2)
    assert C.units_per_block(C.Case(256, C.cases_of(256).BASIS32, 17, 3, 2, (1, 5, 25))) == \
        {"k_rns_hoist<Arith32P,u32,8,2>": (16, 17, 256)}
    assert C.units_per_block(C.Case(65536, M.BASIS64, 3, 3, 1, (5, 25))) == \
        {"k_rnsmp_hoist<Arith64,u64,4,1>": (1, 96, 4096)}


def test_the_sub_batch_rule():
    """The chunk counts output units (p, r): the most whose units * comps polynomials fit
    scratch_mb, never less than one, whatever terms is (a_hat is read from caller memory)."""
    for (n, m, batch, terms, comps, rots, want), case in zip(C.SUBBATCH, C.subbatch_cases()):
        got = C.chunks(case)
        assert got == list(want) and len(got) >= 3 and sum(got) == batch * rots
        assert len(case.ks) == rots and case.scratch_mb == 1
        assert C.chunks(case._replace(terms=terms + 5)) == got
        assert len(C.chunks(case._replace(scratch_mb=0))) == 1          # the default scratch
    n, m = C.SUBBATCH[0][:2]
    poly = len(m) * n * 4
    assert (1 << 20) // (2 * poly) == 5 and (1 << 20) // poly == 10
    assert C.SUBBATCH[0][6][0] % C.SUBBATCH[0][5] != 0          # a border inside a batch entry
    n, m = C.SUBBATCH[2][:2]
    assert len(m) * n * 8 > 1 << 20                             # one unit above the limit
    assert C.chunks(C.Case(4096, C.cases_of(4096).BASIS32, 17, 7, 2, (1, 5), False, 1)) == [34]


def test_the_cases_cover_what_the_issue_names():
    cases = C.equality_cases()
    for n in C.ALL_N:
        T = C.cases_of(n)
        here = [c for c in cases if c.n == n]
        assert {c.batch for c in here} == {17 if n <= 4096 else 3} == {T.BATCH}
        for bits in (32, 64):
            mine = [c for c in here if C.word_bits(c.moduli) == bits]
            long_n = n in (256, 4096, 8192, 65536)
            assert {len(c.moduli) for c in mine} == {1, 3}
            assert {c.terms for c in mine} == ({1, 3, 7} if long_n else {1, 3}), (n, bits)
            for L in (1, 3):
                at = [c for c in mine if len(c.moduli) == L]
                assert {(c.comps, len(c.ks)) for c in at} == {(1, 1), (1, 3), (2, 1), (2, 3)}
                assert {k for c in at for k in c.ks} == set(C.pool(n))
        assert all(len(set(c.ks)) == len(c.ks) for c in here)
    assert C.pool(256) == (1, 5, 25, 511, 205) and 5 * 205 % 512 == 1
    assert 17 % (256 // (256 // 16)) != 0                      # n = 256 ends in a partial workgroup
    assert C.ORACLE_N == C.RANGE_N == (256, 4096, 8192, 65536)
    assert C.ORACLE_TERMS <= 3 and C.ORACLE_BATCH == 2 and C.RANGE_TERMS == 7
    assert all(2 * c.n - 1 in c.ks for c in C.all_cases()
               if c.batch == C.ORACLE_BATCH and c.terms == C.ORACLE_TERMS and len(c.ks) == 2)
    assert {(n, C.word_bits(m)) for n, m, _, _ in C.VALIDATE} == \
        {(512, 32), (256, 64), (8192, 32), (8192, 64)}
    assert {(C.family(n), C.word_bits(m)) for n, m in C.HOST} == \
        {(f, b) for f in ("rns", "rnsmp") for b in (32, 64)}
    assert C.CHAIN == ((256, "rns"), (8192, "rnsmp")) and C.CHAIN_SHAPE == (4, 2, 2)
    assert (C.CHAIN_BATCH, C.CHAIN_H, C.CHAIN_ROTS) == (2, 8, 3)
    assert C.MAX_COMPS == nttmul.MACN_MAX_COMPS == 2
    assert C.MAX_ROTS == nttmul.HOIST_MAX_ROTS == nttmul.GALOIS_MAX_COUNT == 16
    assert C.transforms(3, 8) == (19, 40)


def test_every_entry_point_that_writes_caller_memory_has_a_footprint_row():
    rows = C.footprint_cases()
    named = {f.entry for f in rows}
    writers = {s for s in nttmul.hoist_exported_symbols()
               if re.fullmatch(r"nttmul_rns(mp)?_hoist_ntt(_device)?", s)}
    assert len(writers) == 4 and named == writers
    assert set(nttmul.hoist_exported_symbols()) - writers == {
        "nttmul_rns_hoist_kernel_name", "nttmul_rnsmp_hoist_kernel_name"}  # at most cap bytes
    for entry in writers:
        sizes = C.FP_SIZES[:3] if "_rns_" in entry else C.FP_SIZES[3:]
        got = {(C.word_bits(f.case.moduli), f.case.n, f.case.batch) for f in rows
               if f.entry == entry}
        assert got == {(b, n, batch) for b in (32, 64) for n, batch in sizes}
    assert C.FP_SIZES == ((256, 1), (256, 5), (4096, 1), (8192, 1), (8192, 5))
    assert all((f.host == "host") == (not f.entry.endswith("_device")) for f in rows)
    assert all(f.case.comps == 2 and len(f.case.ks) == 3 and len(f.case.moduli) == 3
               for f in rows)
    import guarded as G
    for f in rows:
        (per, units, words), = C.units_per_block(f.case).values()
        if f.case.n == 256:
            assert units % per                                 # a partial workgroup
        assert C.fp_guard_words(f.case) >= max(per * words * f.case.comps, G.guard_words(1))
