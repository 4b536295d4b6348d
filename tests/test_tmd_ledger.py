"""The kernel ledger of lib/libnttmul_tmd.so, in the style of tests/test_xconv_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names, per-kernel
hashes and the code objects' metadata only.  libnttmul_tmd.so = libnttmul_ctlin.so's kernels, bit
for bit, plus k_tmd_fwd at the five degrees up to 4096 and k_tmd_cols_fwd at the four splits
above, in both word classes (18 kernels); every one is launched by a case of tests/tmd_cases.py
(whose mirror test_gpu_tmd.py anchors to the library's kernel_name entry point on the GPU) or has
a reason in EXEMPT; none has a private segment; and the VGPR counts DESIGN.md quotes are the
listing's."""
import os
import re
import subprocess

import pytest

import nttmul
import tmd_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLDER = ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
         "GALOIS_LIB_PATH", "KS_LIB_PATH", "MACN_LIB_PATH", "HOIST_LIB_PATH", "MDNTT_LIB_PATH",
         "KSNTT_LIB_PATH", "LINTRANS_LIB_PATH", "CTMUL_LIB_PATH", "XCONV_LIB_PATH",
         "LEVEL_LIB_PATH", "CTLIN_LIB_PATH"]
CLASSES = (("Arith32P", "u32"), ("Arith64", "u64"))


@pytest.fixture(scope="module")
def ctlin():
    return nttmul.kernel_hashes(nttmul.CTLIN_LIB_PATH)


@pytest.fixture(scope="module")
def tmd():
    return nttmul.kernel_hashes(nttmul.TMD_LIB_PATH)


@pytest.fixture(scope="module")
def meta():
    return C.kernel_metadata(nttmul.TMD_LIB_PATH)


def _launched():
    out = {}
    for case in C.all_cases():
        for key in C.kernels_of(case):
            out.setdefault(key, case)
    return out


def test_common_kernels_are_the_ctlin_librarys_bit_for_bit(ctlin, tmd):
    assert len(ctlin) > 400
    assert sorted(set(ctlin) - set(tmd)) == []
    assert {k: tmd[k] for k in ctlin} == ctlin


def test_the_additional_kernels_are_exactly_what_the_cases_launch(ctlin, tmd):
    extra = set(tmd) - set(ctlin)
    launched = _launched()
    ours = {k for k in launched if k.startswith("k_tmd_")}
    # the range check, mdntt.hip's inverse half and row pass, rnsmp.hip's column pass
    assert all(k in ctlin for k in set(launched) - ours)
    assert {k.split("<")[0] for k in set(launched) - ours} == {
        "k_rns_check_range", "k_mdntt_inv", "k_mdntt_inv_rows", "k_rnsmp_cols_inv", "k_mdntt_rows"}
    missing = sorted(k for k in extra if k not in launched and k not in C.EXEMPT)
    assert not missing, f"kernels no case launches and no reason exempts: {missing}"
    assert all(C.EXEMPT.values()) and set(C.EXEMPT) <= extra
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    want = {f"k_tmd_fwd<{cls},{io},{logn}>" for cls, io in CLASSES for logn in range(8, 13)}
    want |= {f"k_tmd_cols_fwd<{cls},{io},{l1}>" for cls, io in CLASSES for l1 in range(1, 5)}
    assert extra == want and len(extra) == 18


@pytest.mark.parametrize("path", OLDER)
def test_the_older_libraries_do_not_grow(path):
    """The sixteen older libraries keep their ABI and kernels: the new entry points and the
    k_tmd_* kernels are in the seventeenth library only."""
    out = subprocess.run(["nm", "-D", "--defined-only", getattr(nttmul, path)],
                         capture_output=True, text=True, check=True).stdout
    assert not re.search(r"tmd", out)
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "tmd" in k]


def test_no_new_kernel_has_a_private_segment(ctlin, tmd, meta):
    """From the code object's metadata: no scratch, no spill."""
    assert set(meta) == set(tmd)
    new = sorted(set(tmd) - set(ctlin))
    assert len(new) == 18
    for k in new:
        m = meta[k]
        assert m[".private_segment_fixed_size"] == 0, k
        assert m[".vgpr_spill_count"] == 0, k
        assert not m.get(".uses_dynamic_stack", False), k
        assert m[".max_flat_workgroup_size"] == 256 and m[".wavefront_size"] == 64, k


def _design_rows():
    """The listing table of DESIGN.md's section on this library: {kernel_key: (VGPRs, waves per
    SIMD)} from the rows `| k_tmd_...<...> | vgprs | waves | ...`."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    rows = re.findall(r"^\| `(k_(?:tmd|mdntt)_\w+<[^>]+>)` \| (\d+) \| (\d+) \|", text, re.M)
    return {k: (int(v), int(w)) for k, v, w in rows}


def test_the_vgpr_counts_design_md_quotes_are_the_listings(ctlin, tmd, meta):
    rows = _design_rows()
    new = set(tmd) - set(ctlin)
    assert new <= set(rows), sorted(new - set(rows))
    for k, (vgprs, waves) in rows.items():
        assert k in meta, k
        assert meta[k][".vgpr_count"] == vgprs, (k, meta[k][".vgpr_count"])
        # 512 registers per SIMD lane, allocated in blocks of 8, at most 8 waves
        assert waves == min(8, 512 // (-(-vgprs // 8) * 8)), k
    # the aim: the 64-bit k_tmd_fwd keeps three waves per SIMD, as k_mdntt_fwd
    for logn in range(8, 13):
        assert rows[f"k_tmd_fwd<Arith64,u64,{logn}>"][1] == 3
        assert rows[f"k_mdntt_fwd<Arith64,u64,{logn}>"][1] == 3


def test_mirror_restates_the_selection_rules():
    for n in C.ALL_N:
        for bits, (cls, io) in zip((32, 64), CLASSES):
            if n <= 4096:
                logn = n.bit_length() - 1
                assert C.kernel_name(n, bits) == \
                    f"k_mdntt_inv<{cls},{io},{logn}> + k_tmd_fwd<{cls},{io},{logn}>"
            else:
                l1 = n.bit_length() - 13
                assert C.kernel_name(n, bits) == (
                    f"k_mdntt_inv_rows<{cls},{io},{l1}> + k_rnsmp_cols_inv<{cls},{io},{l1}> + "
                    f"k_tmd_cols_fwd<{cls},{io},{l1}> + k_mdntt_rows<{cls},{io},{l1}>")
    with pytest.raises(AssertionError):
        C.kernel_name(131072, 32)
    case = C.Case(64, 8192, 3, 2, 1, 3, True)
    assert C.kernels_of(case) == ["k_rns_check_range<u64>"] + C.sequence(8192, 64)
    assert C.units_per_block(C.Case(32, 256, 33, 3, 2, 3)) == {
        "k_mdntt_inv<Arith32P,u32,8>": (32, 33, 256), "k_tmd_fwd<Arith32P,u32,8>": (16, 33, 256)}
    assert C.grid_rows(C.Case(32, 8192, 1, 5, 3, 3)) == {
        "k_mdntt_inv_rows<Arith32P,u32,1>": 3, "k_rnsmp_cols_inv<Arith32P,u32,1>": 3,
        "k_tmd_cols_fwd<Arith32P,u32,1>": 5, "k_mdntt_rows<Arith32P,u32,1>": 5}


def test_the_sub_batch_rule():
    for case in C.subbatch_cases():
        want = [w for *_, w in C.SUBBATCH if sum(w) == case.batch][0]
        got = C.chunks(case)
        assert got == list(want) and len(got) == 3 and case.scratch_mb == 1 and case.n == 8192
        assert got[-1] < got[0]
        assert len(C.chunks(case._replace(scratch_mb=0))) == 1
        assert C.kernels_of(case) == C.sequence(case.n, case.bits) * 3


def test_the_cases_cover_what_the_issue_names():
    cases = C.parity_cases()
    for bits in (32, 64):
        ts = C.plain_moduli(bits)
        assert ts == (3, 65537, C.T_BOUND[bits] - 1) and all(t % 2 for t in ts)
        mine = [c for c in cases if c.bits == bits]
        assert {(c.n, c.L, c.K, c.t) for c in mine} == {
            (n, L, K, t) for n in (256, 512) for L, K in C.SHAPES for t in ts}
        assert all(c.batch == 3 for c in mine)
        cad = C.CADENCE[bits]
        # K + 1 products: a whole number of fold groups, a shorter last group, and both sides of
        # the cadence
        ks = {K + 1 for _, K in C.SHAPES}
        assert cad in ks and any(k % cad for k in ks) and min(ks) <= cad < max(ks)
        ident = [c for c in C.identity_cases() if c.bits == bits]
        assert {c.n for c in ident} == {256, 1024, 4096, 8192, 65536}
        assert all((c.batch, c.L, c.K) == (2, 3, 2) for c in ident)
    assert C.SHAPES == ((1, 1), (3, 1), (4, 2), (3, 3), (2, 5))
    assert C.CADENCE == {32: 2, 64: 4}
    assert C.EDGE_N == (256, 8192) and C.CHAIN_N == (256, 8192) and C.CHAIN_T == (3, 65537)
    assert C.BASES_N == (256, 8192) and (C.E2E_N, C.E2E_T) == (256, 65537)


def test_the_scale_cases_meet_the_rule_of_scale_cases():
    import scale_cases as S
    assert (C.MIN_WAVES, C.WAVE) == (S.MIN_WAVES, S.WAVE)
    rows = C.scale_cases()
    assert {(c.bits, c.n) for c in rows} == {(b, n) for b in (32, 64) for n in (4096, 8192)}
    seen = set()
    for case in rows:
        assert len(C.chunks(case)) == 1
        waves = C.launch_waves(case)
        assert list(waves) == C.sequence(case.n, case.bits)
        assert all(w >= S.MIN_WAVES for w in waves.values()), (case, waves)
        for key, (per, units, _) in C.units_per_block(case).items():
            assert per == 1 or units % per, (case, key)
        seen |= set(waves)
    ours = {k for k in nttmul.kernel_hashes(nttmul.TMD_LIB_PATH) if k.startswith("k_tmd_")}
    tmpl = lambda k: k.split(",")[0]                                          # noqa: E731
    assert {tmpl(k) for k in seen if k.startswith("k_tmd_")} == {tmpl(k) for k in ours}


def test_every_entry_point_that_writes_caller_memory_has_a_footprint_row():
    rows = C.footprint_cases()
    named = {f.entry for f in rows}
    writers = {s for s in nttmul.tmd_exported_symbols()
               if re.fullmatch(r"nttmul_tmd_moddown(_device)?", s)}
    assert len(writers) == 2 and named == writers
    assert set(nttmul.tmd_exported_symbols()) - writers == {
        "nttmul_tmd_create", "nttmul_tmd_destroy", "nttmul_tmd_last_error",
        "nttmul_tmd_get_info", "nttmul_tmd_kernel_name", "nttmul_tmd_plan"}
    for entry in writers:
        got = {(f.case.bits, f.case.n, f.case.batch, f.case.L, f.case.K) for f in rows
               if f.entry == entry}
        assert got == {(b, n, batch, L, K) for b in (32, 64) for n, batch in C.FP_SIZES
                       for L, K in C.FP_SHAPES}
    assert all((f.host == "host") == (not f.entry.endswith("_device")) for f in rows)


def test_every_additional_kernel_is_launched_by_a_case_held_to_the_cpu_reference(ctlin, tmd):
    """The mirror reports the cases whose every output word a GPU test compares with the CPU
    reference (referenced_cases(): at every n, tests/full_ref.py); the cases full_ref.SUBSET holds
    on a part of their batch only do not count, and are at most one in ten.  Every kernel this
    library adds over its predecessor is launched by one of the rest."""
    import full_ref
    cases = C.referenced_cases()
    assert cases and all(c in C.all_cases() for c in cases[:8] + cases[-8:])
    whole = [c for c in cases if not full_ref.on_subset("tmd", c)]
    assert 10 * (len(cases) - len(whole)) <= len(cases)
    held = {k for c in whole for k in C.kernels_of(c)}
    excused = {k for k in tmd if any(re.fullmatch(pat, k) for pat, _ in
                                        getattr(C, "UNREACHABLE", ()))}
    extra = set(tmd) - set(ctlin)
    assert extra and sorted(extra - held - excused) == []
