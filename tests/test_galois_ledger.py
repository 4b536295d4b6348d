"""The kernel ledger of lib/libnttmul_galois.so, in the style of tests/test_rnsmp_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_galois.so = libnttmul_rnsmp.so's kernels, bit for bit, plus the k_galois_*
kernels, and every one of those is launched by a case of tests/galois_cases.py (whose mirror
test_gpu_galois.py anchors to nttmul_galois_kernel_name on the GPU)."""
import re
import subprocess

import pytest

import dispatch_cases as D
import galois_cases as C
import nttmul
import rnsmp_cases as R


@pytest.fixture(scope="module")
def rnsmp():
    return nttmul.kernel_hashes(nttmul.RNSMP_LIB_PATH)


@pytest.fixture(scope="module")
def galois():
    return nttmul.kernel_hashes(nttmul.GALOIS_LIB_PATH)


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


def test_common_kernels_are_the_rnsmp_librarys_bit_for_bit(rnsmp, galois):
    assert len(rnsmp) > 269 + 56
    assert sorted(set(rnsmp) - set(galois)) == []
    assert {k: galois[k] for k in rnsmp} == rnsmp


def test_the_additional_kernels_are_exactly_what_the_cases_launch(rnsmp, galois):
    extra = set(galois) - set(rnsmp)
    launched = _launched()
    assert all(k.startswith("k_galois_") for k in extra), sorted(extra)
    ours = {k for k in launched if not k.startswith("k_rns_check_range")}
    assert all(k.startswith("k_galois_") and k not in rnsmp for k in ours), sorted(ours)
    assert all(k in rnsmp for k in set(launched) - ours)     # the range check is the RNS library's
    missing = sorted(k for k in extra if k not in launched and not _unreachable_reason(k))
    assert not missing, f"kernels no case launches and no rule excuses: {missing}"
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    assert not [k for k in launched if _unreachable_reason(k)]
    assert C.UNREACHABLE == ()
    # per word: the coefficient kernel staged whole and split in 2 (and on 64-bit words 4)
    # classes, the gather and the scatter of the NTT order
    assert extra == ({f"k_galois_{k}<{io}>" for io in ("u32", "u64") for k in ("ntt", "ntt_many")}
                     | {f"k_galois_coeff<u32,{m}>" for m in (0, 1)}
                     | {f"k_galois_coeff<u64,{m}>" for m in (0, 1, 2)})


@pytest.mark.parametrize("path", ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH",
                                  "RNSMP_LIB_PATH"])
def test_the_older_libraries_do_not_grow(path):
    """The five older libraries keep their ABI and kernels: the new entry points and the
    k_galois_* kernels are in the sixth library only."""
    out = subprocess.run(["nm", "-D", "--defined-only", getattr(nttmul, path)],
                         capture_output=True, text=True, check=True).stdout
    assert "nttmul_galois" not in out and "k_galois" not in out
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "k_galois" in k]


def test_mirror_restates_the_selection_rules():
    # coefficient order: one limb polynomial staged whole while it fits 128 KiB, in 2^m classes above
    for n in C.ALL_N:
        assert C.kernel_name("coeff", n, R.BASIS32) == \
            f"k_galois_coeff<u32,{ {65536: 1}.get(n, 0)}>"
        assert C.kernel_name("coeff", n, R.BASIS64[:1]) == \
            f"k_galois_coeff<u64,{ {32768: 1, 65536: 2}.get(n, 0)}>"
        assert C.kernel_name("ntt", n, R.BASIS32) == "k_galois_ntt<u32>"
        assert C.kernel_name("ntt_many", n, R.BASIS64) == "k_galois_ntt_many<u64>"
    case = C.Case("ntt_many", 256, R.BASIS64, 3, C.many_ks(256, 16), True)
    assert C.kernels_of(case) == ["k_rns_check_range<u64>", "k_galois_ntt_many<u64>"]
    assert C.kernels_of(C.Case("coeff", 65536, R.BASIS32, 1, (3,))) == ["k_galois_coeff<u32,1>"]
    with pytest.raises(AssertionError):
        C.kernels_of(C.Case("ntt_many", 256, R.BASIS32, 1, C.many_ks(256, 16) + (3,)))   # 17
    with pytest.raises(AssertionError):
        C.kernels_of(C.Case("ntt", 256, R.BASIS32, 1, (3, 5)))
    with pytest.raises(AssertionError):
        C.kernels_of(C.Case("ntt", 256, R.BASIS32, 1, (4,)))                 # an even k
    with pytest.raises(AssertionError):
        C.kernels_of(C.Case("ntt", 256, R.BASIS32, 1, (513,)))               # k >= 2n
    with pytest.raises(AssertionError):
        C.kernel_name("ntt", 256, (D.Q31, D.Q62))                            # mixed classes
    with pytest.raises(AssertionError):
        C.kernel_name("ntt", 256, (D.Q32,))                                  # [2^31, 2^32)
    with pytest.raises(AssertionError):
        C.kernel_name("ntt", 131072, R.BASIS32)
    # units: four slices of 256 words per workgroup; the staged form whole polynomials
    assert C.units_per_block(C.Case("ntt", 256, R.BASIS32, 5, (3,))) == \
        {"k_galois_ntt<u32>": (4, 5, 256)}
    assert C.units_per_block(C.Case("coeff", 256, R.BASIS32, 5, (3,))) == \
        {"k_galois_coeff<u32,0>": (4, 5, 256)}
    assert C.units_per_block(C.Case("coeff", 512, R.BASIS32, 5, (3,))) == \
        {"k_galois_coeff<u32,0>": (2, 5, 512)}
    assert C.units_per_block(C.Case("coeff", 8192, R.BASIS64, 5, (3,))) == \
        {"k_galois_coeff<u64,0>": (1, 5, 8192)}
    assert C.units_per_block(C.Case("coeff", 65536, R.BASIS64, 5, (3,))) == \
        {"k_galois_coeff<u64,2>": (1, 20, 16384)}


def test_the_cases_cover_what_the_issue_names():
    assert C.GALOIS_N == (256, 4096, 8192, 65536) and C.FP_N == (256, 65536)
    assert C.BASES == R.BASES
    for basis in C.BASES:
        for q in basis:
            assert nttmul.is_prime(q) and (q - 1) % (1 << 17) == 0, q
    shapes = C.shapes()
    assert len(shapes) == len(set(shapes)) == 4 * 2 * 2 * 2
    # every n at which the coefficient kernel changes its split is a case, in both classes
    for bits, basis in ((32, R.BASIS32), (64, R.BASIS64)):
        steps = {n for n in C.ALL_N[1:] if C.coeff_lgm(n, bits) != C.coeff_lgm(n // 2, bits)}
        assert steps <= set(C.GALOIS_N + C.SPLIT_N) and len(steps) == (1 if bits == 32 else 2)
        # and so is the largest n staged whole
        assert max(n for n in C.ALL_N if not C.coeff_lgm(n, bits)) in C.SPLIT_N
        assert {(n, basis, C.SPLIT_BATCH) for n in C.SPLIT_N} <= set(C.split_shapes())
    for n in C.GALOIS_N:
        ks = C.ks_at(n)
        assert ks[:5] == (1, 3, n - 1, n + 1, 2 * n - 1)
        assert ks[5] == 5 and ks[6] * 125 % (2 * n) == 1
        assert all(k % 2 == 1 and 0 < k < 2 * n for k in C.many_ks(n, C.MAX_COUNT))
        assert len(set(C.many_ks(n, C.MAX_COUNT))) == C.MAX_COUNT
    # the largest products wrap 32 bits only at n = 65536
    assert (2 * 65536 - 1) * (2 * 65535 + 1) >= 1 << 32 > (2 * 32768 - 1) * (2 * 32767 + 1)
    for n, moduli, limb, other in C.VALIDATE:
        assert moduli[limb] < moduli[other]
    assert {R.word_bits(m) for _, m, _, _ in C.VALIDATE} == {32, 64}
    assert {R.word_bits(m) for _, m in C.HOST} == {32, 64}


def test_every_entry_point_that_writes_caller_memory_has_a_footprint_row():
    rows = C.footprint_cases()
    named = {f.entry for f in rows}
    writers = {s for s in nttmul.galois_exported_symbols()
               if re.fullmatch(r"nttmul_galois_(coeff|ntt|ntt_many)(_device)?", s)}
    assert len(writers) == 5 and named == writers
    # the rest: contexts, queries and the host-only tables (tests/test_galois_abi.py)
    rest = set(nttmul.galois_exported_symbols()) - writers
    assert rest == {"nttmul_galois_" + s for s in (
        "create", "destroy", "last_error", "get_info", "limb_info", "element", "plan",
        "kernel_name")}
    for entry in writers:
        got = {(f.case.n, C.word_bits(f.case.moduli), f.case.batch) for f in rows
               if f.entry == entry}
        assert got == {(n, b, batch) for n in C.FP_N for b in (32, 64) for batch in C.FP_BATCHES}
        assert all(len(f.case.moduli) == 3 for f in rows if f.entry == entry)
    assert all((f.host == "host") == (not f.entry.endswith("_device")) for f in rows)


def test_every_kernel_with_several_polynomials_per_workgroup_ends_a_row_partially():
    """Some footprint row of every such kernel has at least one whole workgroup and a partial last
    one; the kernels that never share a workgroup between polynomials are whole at every row."""
    several, partial = set(), set()
    for f in C.footprint_cases():
        (key, (per, units, _)), = C.units_per_block(f.case).items()
        if C.polys_per_block(f.case) > 1:
            several.add(key)
            if units > per and units % per:
                partial.add(key)
        else:
            assert units % per == 0, (key, f.case)
    assert several == {f"k_galois_{k}" for io in ("u32", "u64")
                       for k in (f"coeff<{io},0>", f"ntt<{io}>", f"ntt_many<{io}>")}
    assert partial == several


def test_guards_cover_a_workgroups_span():
    import guarded as G
    for f in C.footprint_cases():
        (per, _, words), = C.units_per_block(f.case).values()
        assert C.fp_guard_words(f.case) >= max(per * words, len(f.case.moduli) * f.case.n)
        assert C.fp_guard_words(f.case) >= G.guard_words(1)
