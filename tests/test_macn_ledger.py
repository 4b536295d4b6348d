"""The kernel ledger of lib/libnttmul_macn.so, in the style of tests/test_ks_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_macn.so = libnttmul_ks.so's kernels, bit for bit, plus k_rns_macn<*,*,*,2>
at the five degrees up to 4096 and k_rnsmp_macn<*,*,*,2> at the four splits above, in both word
classes, and every one is launched by a case of tests/macn_cases.py (whose mirror
test_gpu_macn.py anchors to the library's kernel_name entry points on the GPU)."""
import re
import subprocess

import pytest

import macn_cases as C
import nttmul
import rnsmp_cases as M

OLDER = ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
         "GALOIS_LIB_PATH", "KS_LIB_PATH"]


@pytest.fixture(scope="module")
def ks():
    return nttmul.kernel_hashes(nttmul.KS_LIB_PATH)


@pytest.fixture(scope="module")
def macn():
    return nttmul.kernel_hashes(nttmul.MACN_LIB_PATH)


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


def test_common_kernels_are_the_ks_librarys_bit_for_bit(ks, macn):
    assert len(ks) > 269 + 56 + 9 + 2
    assert sorted(set(ks) - set(macn)) == []
    assert {k: macn[k] for k in ks} == ks


def test_the_additional_kernels_are_exactly_what_the_cases_launch(ks, macn):
    extra = set(macn) - set(ks)
    launched = _launched()
    ours = {k for k in launched if re.match(r"k_rns(mp)?_macn<", k)}
    # the range check, the contexts' own mac kernels (comps = 1) and the column passes
    assert all(k in ks for k in set(launched) - ours)
    assert {k.split("<")[0] for k in set(launched) - ours} == {
        "k_rns_check_range", "k_rns_mac", "k_rnsmp_mac", "k_rnsmp_cols_fwd", "k_rnsmp_cols_inv"}
    missing = sorted(k for k in extra if k not in launched and not _unreachable_reason(k))
    assert not missing, f"kernels no case launches and no rule excuses: {missing}"
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    assert not [k for k in launched if _unreachable_reason(k)]
    assert C.UNREACHABLE == ()
    classes = (("Arith32P", "u32"), ("Arith64", "u64"))
    want = {f"k_rns_macn<{cls},{io},{logn},2>" for cls, io in classes for logn in range(8, 13)}
    want |= {f"k_rnsmp_macn<{cls},{io},{l1},2>" for cls, io in classes for l1 in range(1, 5)}
    assert extra == want and len(extra) == 18


@pytest.mark.parametrize("path", OLDER)
def test_the_older_libraries_do_not_grow(path):
    """The seven older libraries keep their ABI and kernels: the new entry points and the macn
    kernels are in the eighth library only."""
    out = subprocess.run(["nm", "-D", "--defined-only", getattr(nttmul, path)],
                         capture_output=True, text=True, check=True).stdout
    assert not re.search(r"nttmul_\w*_macn_", out) and not re.search(r"k_\w*_macn", out)
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "_macn" in k]


def test_mirror_restates_the_selection_rules():
    for n in C.ALL_N:
        for moduli, cls, io in ((C.cases_of(n).BASIS32, "Arith32P", "u32"),
                                (C.cases_of(n).BASIS64, "Arith64", "u64")):
            if n <= 4096:
                logn = n.bit_length() - 1
                assert C.kernel_name(n, moduli, 1) == f"k_rns_mac<{cls},{io},{logn}>"
                assert C.kernel_name(n, moduli, 2) == f"k_rns_macn<{cls},{io},{logn},2>"
            else:
                l1 = n.bit_length() - 13
                assert C.kernel_name(n, moduli, 1) == M.kernel_name("mac", n, moduli)
                assert C.kernel_name(n, moduli, 2) == (
                    f"k_rnsmp_cols_fwd<{cls},{io},{l1},1> + k_rnsmp_macn<{cls},{io},{l1},2> + "
                    f"k_rnsmp_cols_inv<{cls},{io},{l1}>")
            for comps in (0, 3):
                with pytest.raises(AssertionError):
                    C.kernel_name(n, moduli, comps)
    with pytest.raises(AssertionError):
        C.kernel_name(131072, M.BASIS32, 2)
    case = C.Case(8192, M.BASIS64, 3, 2, 2, True, True)
    assert C.kernels_of(case) == ["k_rns_check_range<u64>"] * 2 + C.sequence(8192, M.BASIS64, 2)
    assert C.units_per_block(C.Case(256, C.cases_of(256).BASIS32, 17, 3)) == \
        {"k_rns_macn<Arith32P,u32,8,2>": (16, 17, 256)}
    assert C.units_per_block(C.Case(65536, M.BASIS64, 3, 3)) == \
        {"k_rnsmp_macn<Arith64,u64,4,2>": (1, 48, 4096)}


def test_the_sub_batch_rule():
    """The chunk keeps both batch * terms and batch * comps polynomials within scratch_mb; with
    comps = 1 it is the context's own rule (tests/rnsmp_cases.py chunks)."""
    for n, m, terms, batch, want in C.SUBBATCH:
        for shared in (True, False):
            got = C.chunks(C.Case(n, m, batch, terms, 2, shared, False, 1))
            assert got == list(want) and len(got) >= 3 and sum(got) == batch
        assert len(C.chunks(C.Case(n, m, batch, terms, 2))) == 1          # the default scratch
        assert C.chunks(C.Case(n, m, batch, terms, 1, True, False, 1)) == \
            M.chunks(M.Case("mac", n, m, batch, terms, True, scratch_mb=1))
    # the output bounds the chunk where comps > terms, a bounds it where terms > comps
    n, m = C.SUBBATCH[0][:2]
    poly = len(m) * n * 4
    assert (1 << 20) // (2 * poly) == 5 and (1 << 20) // (3 * poly) == 3
    # one polynomial above the limit: the scratch grows to hold it
    assert C.chunks(C.Case(65536, M.BASIS64, 2, 3, 2, True, False, 1)) == [1, 1]
    assert C.chunks(C.Case(4096, C.cases_of(4096).BASIS32, 17, 7, 2, True, False, 1)) == [17]


def test_the_cases_cover_what_the_issue_names():
    cases = C.equality_cases()
    for n in C.ALL_N:
        T = C.cases_of(n)
        here = [c for c in cases if c.n == n]
        assert {c.batch for c in here} == {17 if n <= 4096 else 3}
        for bits in (32, 64):
            mine = [c for c in here if C.word_bits(c.moduli) == bits and c.comps == 2]
            limbs = {len(c.moduli) for c in mine}
            terms = {c.terms for c in mine}
            long_n = n in (256, 4096, 8192, 65536)
            assert limbs == ({1, 3, 5} if long_n and bits == 32 else {1, 3}), (n, bits)
            assert terms == ({1, 3, 7} if long_n else {1, 3}), (n, bits)
            assert {c.shared for c in mine} == {True, False}
        assert any(c.comps == 1 for c in here)
        assert T.BATCH == here[0].batch
    assert 17 % (256 // (256 // 16)) != 0                      # n = 256 ends in a partial workgroup
    assert C.ORACLE_N == C.RANGE_N == (256, 4096, 8192, 65536)
    assert C.ORACLE_TERMS <= 3 and C.RANGE_TERMS == 7
    assert {(n, C.word_bits(m)) for n, m, _, _ in C.VALIDATE} == \
        {(512, 32), (256, 64), (8192, 32), (8192, 64)}
    assert {(C.family(n), C.word_bits(m)) for n, m in C.HOST} == \
        {(f, b) for f in ("rns", "rnsmp") for b in (32, 64)}
    assert C.CHAIN == ((256, "rns"), (8192, "rnsmp")) and C.CHAIN_SHAPE == (4, 2, 2)
    assert (C.CHAIN_BATCH, C.CHAIN_H) == (2, 8)
    assert C.SUBBATCH[0][:2] == M.SUBBATCH[0][:2] and C.SUBBATCH[0][0] == 8192
    assert C.MAX_COMPS == nttmul.MACN_MAX_COMPS == 2


def test_every_entry_point_that_writes_caller_memory_has_a_footprint_row():
    rows = C.footprint_cases()
    named = {f.entry for f in rows}
    writers = {s for s in nttmul.macn_exported_symbols()
               if re.fullmatch(r"nttmul_rns(mp)?_macn_ntt(_device)?", s)}
    assert len(writers) == 4 and named == writers
    assert set(nttmul.macn_exported_symbols()) - writers == {
        "nttmul_rns_macn_kernel_name", "nttmul_rnsmp_macn_kernel_name"}   # at most cap bytes
    for entry in writers:
        sizes = C.FP_SIZES[:3] if "_rns_" in entry else C.FP_SIZES[3:]
        got = {(C.word_bits(f.case.moduli), f.case.n, f.case.batch, f.case.shared)
               for f in rows if f.entry == entry}
        assert got == {(b, n, batch, s) for b in (32, 64) for n, batch in sizes
                       for s in (True, False)}
    assert C.FP_SIZES == ((256, 1), (256, 5), (4096, 1), (8192, 1), (8192, 5))
    assert all((f.host == "host") == (not f.entry.endswith("_device")) for f in rows)
    assert all(f.case.comps == 2 and len(f.case.moduli) == 3 for f in rows)
    import guarded as G
    for f in rows:
        (per, units, words), = C.units_per_block(f.case).values()
        if f.case.n == 256:
            assert units % per                                 # a partial workgroup
        assert C.fp_guard_words(f.case) >= max(per * words * f.case.comps, G.guard_words(1))
