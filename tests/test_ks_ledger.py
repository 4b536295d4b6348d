"""The kernel ledger of lib/libnttmul_ks.so, in the style of tests/test_galois_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_ks.so = libnttmul_galois.so's kernels, bit for bit (k_bconv<*,*>, which
ModDown launches at n up to 65536, included), plus k_ks_modup<u32> and <u64>, and both are launched
by a case of tests/ks_cases.py (whose mirror test_gpu_ks.py anchors to nttmul_ks_kernel_name on the
GPU)."""
import re
import subprocess

import pytest

import ks_cases as C
import nttmul


@pytest.fixture(scope="module")
def galois():
    return nttmul.kernel_hashes(nttmul.GALOIS_LIB_PATH)


@pytest.fixture(scope="module")
def ks():
    return nttmul.kernel_hashes(nttmul.KS_LIB_PATH)


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


def test_common_kernels_are_the_galois_librarys_bit_for_bit(galois, ks):
    assert len(galois) > 269 + 56 + 9
    assert sorted(set(galois) - set(ks)) == []
    assert {k: ks[k] for k in galois} == galois
    bconv = {k for k in galois if k.startswith("k_bconv<")}
    assert bconv == {f"k_bconv<{io},{op}>" for io in ("u32", "u64") for op in (0, 1)}


def test_bconv_kernels_are_the_bconv_librarys_bit_for_bit(ks):
    """Raising the internal degree bound of bconv.hip's dispatch changes host code only."""
    older = nttmul.kernel_hashes(nttmul.BCONV_LIB_PATH)
    assert {k: ks[k] for k in older} == older


def test_the_additional_kernels_are_exactly_what_the_cases_launch(galois, ks):
    extra = set(ks) - set(galois)
    launched = _launched()
    ours = {k for k in launched if k.startswith("k_ks_")}
    assert all(k in galois for k in set(launched) - ours)    # the range check and k_bconv<*,1>
    assert {k for k in launched if k.startswith("k_bconv")} == {"k_bconv<u32,1>", "k_bconv<u64,1>"}
    missing = sorted(k for k in extra if k not in launched and not _unreachable_reason(k))
    assert not missing, f"kernels no case launches and no rule excuses: {missing}"
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    assert not [k for k in launched if _unreachable_reason(k)]
    assert C.UNREACHABLE == ()
    assert extra == {"k_ks_modup<u32>", "k_ks_modup<u64>"}


@pytest.mark.parametrize("path", ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH",
                                  "RNSMP_LIB_PATH", "GALOIS_LIB_PATH"])
def test_the_older_libraries_do_not_grow(path):
    """The six older libraries keep their ABI and kernels: the new entry points and k_ks_modup are
    in the seventh library only."""
    out = subprocess.run(["nm", "-D", "--defined-only", getattr(nttmul, path)],
                         capture_output=True, text=True, check=True).stdout
    assert "nttmul_ks_" not in out and "k_ks_" not in out
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "k_ks_" in k]


def test_mirror_restates_the_selection_rules():
    for n in C.ALL_N:
        assert C.kernel_name("modup", n, 32) == "k_ks_modup<u32>"
        assert C.kernel_name("modup", n, 64) == "k_ks_modup<u64>"
        assert C.kernel_name("moddown", n, 32) == "k_bconv<u32,1>"
        assert C.kernel_name("moddown", n, 64) == "k_bconv<u64,1>"
    with pytest.raises(AssertionError):
        C.kernel_name("modup", 131072, 32)
    assert C.kernels_of(C.Case("modup", 64, 256, 2, 3, 2, 2, True)) == \
        ["k_rns_check_range<u64>", "k_ks_modup<u64>"]
    assert C.kernels_of(C.Case("moddown", 32, 65536, 1, 3, 2, 1)) == ["k_bconv<u32,1>"]
    with pytest.raises(AssertionError):
        C.kernels_of(C.Case("modup", 32, 256, 1, 3, 2, 4))                   # alpha > L
    with pytest.raises(AssertionError):
        C.kernels_of(C.Case("modup", 32, 256, 1, 3, 2, 0))
    with pytest.raises(AssertionError):
        C.word_bits((3, 5), (3,))                                            # a prime in both
    with pytest.raises(AssertionError):
        C.word_bits((2013265921,), ((1 << 61) + 1,))                         # mixed classes
    assert C.units_per_block(C.Case("modup", 32, 256, 5, 3, 2, 2)) == {"k_ks_modup<u32>": (4, 5, 256)}
    assert C.units_per_block(C.Case("modup", 64, 4096, 1, 3, 2, 2)) == \
        {"k_ks_modup<u64>": (1, 16, 256)}


def test_the_cases_cover_what_the_issue_names():
    assert C.SHAPES == ((1, 1, 1), (4, 2, 2), (5, 2, 2), (5, 3, 5), (6, 1, 1), (2, 1, 1), (3, 2, 2),
                        (60, 4, 15))
    assert (C.N, C.BATCH) == (256, 3)
    assert {L + K for L, K, _ in C.SHAPES} >= {C.TILE - 1, C.TILE + 1, C.MAX_LIMBS}
    assert C.CADENCE_ALPHA == {32: (1, 2, 3, 5, 9), 64: (3, 4, 5, 17)}
    for bits, alphas in C.CADENCE_ALPHA.items():
        cad = C.CADENCE[bits]
        assert {cad - 1, cad, cad + 1} <= set(alphas) | {0}
    assert C.DEGREES == ((4096, 2), (65536, 1)) and C.DEGREE_SHAPE == (4, 2, 2)
    assert C.MODDOWN == ((8192, 2), (65536, 1)) and C.MODDOWN_SHAPE == (3, 2)
    assert {n for n, _ in C.MODDOWN_BCONV} == {256, 4096}
    assert C.CHAIN == ((256, "rns"), (8192, "rnsmp"))
    assert (C.CHAIN_SHAPE, C.CHAIN_BATCH, C.CHAIN_H) == ((4, 2, 2), 2, 8)
    cases = C.modup_cases()
    for bits in (32, 64):
        for q in sum(C.moduli_of(C.Case("modup", bits, 65536, 1, 60, 4, 15)), ()):
            assert nttmul.is_prime(q) and (q - 1) % (1 << 17) == 0, q
        for n, batch in C.DEGREES:
            assert C.Case("modup", bits, n, batch, *C.DEGREE_SHAPE) in cases
    q, p = C.small_moduli()
    assert q[:3] == (7681, 12289, 786433) and C.word_bits(q, p) == 32
    assert any(c.moduli == "small" and c.n == 256 and C.moduli_of(c) == (q, p) for c in cases)


def test_every_entry_point_that_writes_caller_memory_has_a_footprint_row():
    rows = C.footprint_cases()
    named = {f.entry for f in rows}
    writers = {s for s in nttmul.ks_exported_symbols()
               if re.fullmatch(r"nttmul_ks_(modup|moddown)(_device)?", s)}
    assert len(writers) == 4 and named == writers
    for entry in writers:
        got = {(f.case.bits, f.case.n, f.case.batch, (f.case.L, f.case.K, f.case.alpha))
               for f in rows if f.entry == entry}
        assert got == {(b, n, batch, s) for b in (32, 64) for n, batch in C.FP_SIZES
                       for s in C.FP_SHAPES}
    assert C.FP_SIZES == ((256, 1), (256, 5), (4096, 1)) and C.FP_SHAPES == ((3, 2, 2), (5, 1, 5))
    assert all((f.host == "host") == (not f.entry.endswith("_device")) for f in rows)
    # on 32-bit words both batches at n = 256 end in a partial workgroup
    for f in rows:
        (per, units, _), = C.units_per_block(f.case).values()
        if f.case.bits == 32 and f.case.n == 256:
            assert units % per
    import guarded as G
    for f in rows:
        (per, _, words), = C.units_per_block(f.case).values()
        assert C.fp_guard_words(f.case) >= max(per * words, G.guard_words(1))
