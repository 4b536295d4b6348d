"""The kernel ledger of lib/libnttmul_ctlin.so, in the style of tests/test_level_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_ctlin.so = libnttmul_level.so's kernels, bit for bit, plus k_ctlin_combine
(comps 1, 2, 3) and k_ctlin_tensor in both word classes (8 kernels), and every one is launched by a
case of tests/ctlin_cases.py (whose mirror test_gpu_ctlin.py anchors to the library's kernel_name
entry point on the GPU)."""
import os
import re
import subprocess

import pytest

import ctlin_cases as C
import nttmul

OLDER = ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
         "GALOIS_LIB_PATH", "KS_LIB_PATH", "MACN_LIB_PATH", "HOIST_LIB_PATH", "MDNTT_LIB_PATH",
         "KSNTT_LIB_PATH", "LINTRANS_LIB_PATH", "CTMUL_LIB_PATH", "XCONV_LIB_PATH",
         "LEVEL_LIB_PATH"]
CLASSES = (("Arith32P", "u32"), ("Arith64", "u64"))


@pytest.fixture(scope="module")
def level():
    return nttmul.kernel_hashes(nttmul.LEVEL_LIB_PATH)


@pytest.fixture(scope="module")
def ctlin():
    return nttmul.kernel_hashes(nttmul.CTLIN_LIB_PATH)


def _launched():
    out = {}
    for case in C.all_cases():
        for key in C.kernels_of(case):
            out.setdefault(key, case)
    return out


def expected_extra():
    want = {f"k_ctlin_combine<{cls},{io},{c}>" for cls, io in CLASSES for c in (1, 2, 3)}
    return want | {f"k_ctlin_tensor<{cls},{io}>" for cls, io in CLASSES}


def test_common_kernels_are_the_level_librarys_bit_for_bit(level, ctlin):
    assert len(level) > 400
    assert sorted(set(level) - set(ctlin)) == []
    assert {k: ctlin[k] for k in level} == level


def test_the_stream_kernel_this_one_follows_is_still_there_unchanged(level, ctlin):
    high = [k for k in level if k.startswith("k_ctmul_high<")]
    assert len(high) == 2 and all(ctlin[k] == level[k] for k in high)


def test_the_additional_kernels_are_exactly_what_the_cases_launch(level, ctlin):
    extra = set(ctlin) - set(level)
    launched = _launched()
    ours = {k for k in launched if k.startswith("k_ctlin_")}
    # the range check: a kernel of the older libraries
    assert {k.split("<")[0] for k in set(launched) - ours} == {"k_rns_check_range"}
    assert all(k in level for k in set(launched) - ours)
    missing = sorted(k for k in extra if k not in launched)
    assert not missing, f"kernels no case launches: {missing}"
    assert sorted(ours - extra) == [], "the mirror names kernels the library does not hold"
    assert C.UNREACHABLE == ()
    assert extra == expected_extra() and len(extra) == 8
    # every instantiation is hit at n = 256 by a parity case
    small = {C.kernel_name(c) for c in C.parity_cases() if c.n == 256}
    assert small == expected_extra()


def test_every_instantiation_in_the_source_has_a_case_and_the_reverse():
    """csrc/ctlin.hip: combine<A, IO, COMPS> for COMPS 1, 2, 3 through combine_comps<A, IO>, and
    tensor<A, IO>, per word class, each in the launch and in the dry run."""
    src = open(os.path.join(nttmul.PKG_DIR, "csrc", "ctlin.hip")).read()
    for op in ("combine_comps", "tensor"):
        assert src.count(f"{op}<Arith32P, uint32_t>(") == src.count(f"{op}<Arith64, uint64_t>(") == 2
    assert sorted(re.findall(r"return combine<A, IO, (\d)>", src)) == ["1", "2", "3"]
    assert set(re.findall(r"\(k_ctlin_(\w+)<A, IO", src)) == set(C.OPS)
    assert expected_extra() == {k for k in _launched() if k.startswith("k_ctlin_")}


@pytest.mark.parametrize("path", OLDER)
def test_the_older_libraries_do_not_grow(path):
    """The fifteen older libraries keep their ABI and kernels: the new entry points and the
    k_ctlin_* kernels are in the sixteenth library only."""
    out = subprocess.run(["nm", "-D", "--defined-only", getattr(nttmul, path)],
                         capture_output=True, text=True, check=True).stdout
    assert not re.search(r"ctlin", out)
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "ctlin" in k]


def test_mirror_restates_the_selection_and_the_grid():
    for bits, (cls, io) in zip((32, 64), CLASSES):
        for comps in (1, 2, 3):
            case = C.Case("combine", bits, 256, 1, comps, ((C.ONE, 0),))
            assert C.kernel_name(case) == f"k_ctlin_combine<{cls},{io},{comps}>"
        assert C.kernel_name(C.Case("tensor", bits, 256, 1, 3, ())) == f"k_ctlin_tensor<{cls},{io}>"
    with pytest.raises(AssertionError):
        C.kernel_name(C.Case("combine", 32, 256, 1, 4, ((C.ONE, 0),)))
    with pytest.raises(AssertionError):
        C.kernel_name(C.Case("combine", 32, 256, 1, 1, ()))
    with pytest.raises(AssertionError):
        C.grid(1, 131072, 32)
    # 256 vectors of 16 bytes per workgroup: ctmul_high_grid's figures
    assert C.grid(0, 256, 32) == dict(vectors=0, wgx=0, vec=4, per=4, tail=0)
    assert C.grid(1, 256, 32) == dict(vectors=64, wgx=1, vec=4, per=4, tail=64)
    assert C.grid(5, 256, 32) == dict(vectors=320, wgx=2, vec=4, per=4, tail=64)
    assert C.grid(5, 256, 64) == dict(vectors=640, wgx=3, vec=2, per=2, tail=128)
    assert C.grid(5, 512, 32) == dict(vectors=640, wgx=3, vec=4, per=2, tail=128)
    assert C.grid(5, 512, 64) == dict(vectors=1280, wgx=5, vec=2, per=1, tail=0)
    assert C.grid(3, 65536, 64) == dict(vectors=3 * 32768, wgx=384, vec=2, per=1, tail=0)
    assert [C.batches(n, 32) for n in (256, 512, 4096)] == [(1, 3, 5), (1, 3, 5), (1, 3, 2)]
    assert [C.batches(n, 64) for n in (256, 512, 4096)] == [(1, 3, 5), (1, 3, 2), (1, 3, 2)]
    case = C.Case("combine", 64, 256, 5, 2, C.VALIDATE_TERMS, validate=True)
    assert C.kernels_of(case) == ["k_rns_check_range<u64>"] * 5 + ["k_ctlin_combine<Arith64,u64,2>"]
    case = C.Case("combine", 32, 256, 5, 1, ((C.SCALAR, None), (C.ONE, 0)), validate=True)
    assert C.kernels_of(case) == ["k_rns_check_range<u32>"] * 2 + ["k_ctlin_combine<Arith32P,u32,1>"]
    case = C.Case("tensor", 32, 8192, 5, 3, (), 2, True, validate=True)
    assert C.kernels_of(case) == ["k_rns_check_range<u32>", "k_ctlin_tensor<Arith32P,u32>"]
    assert C.kernels_of(case._replace(square=False))[:-1] == ["k_rns_check_range<u32>"] * 2
    assert C.units_per_block(case) == {"k_ctlin_tensor<Arith32P,u32>": (1, 5, 1024)}
    assert C.grid_rows(case) == {"k_ctlin_tensor<Arith32P,u32>": 3}
    assert C.launch_waves(case) == {"k_ctlin_tensor<Arith32P,u32>": 5 * 8 * 3 * 4}
    small = C.Case("combine", 32, 256, 5, 3, ((C.ONE, 0),))
    assert C.units_per_block(small) == {"k_ctlin_combine<Arith32P,u32,3>": (4, 5, 256)}
    assert C.launch_waves(small) == {"k_ctlin_combine<Arith32P,u32,3>": 2 * 1 * 3 * 4}
    assert C.combine_byte_units(2, C.FP_TERMS) == 2 * 4 and C.tensor_byte_units(4) == 19


def test_the_cases_cover_what_the_issue_names():
    rows = C.parity_cases()
    assert C.PARITY_N == (256, 512, 4096, 8192) and set(rows) <= set(C.referenced_cases()) and C.L == 3
    for bits in (32, 64):
        for n in C.PARITY_N:
            mine = [c for c in rows if (c.bits, c.n, c.op) == (bits, n, "combine")]
            assert {c.batch for c in mine} == set(C.batches(n, bits)) >= {1, 3}
            assert {c.comps for c in mine} == {1, 2, 3}
            assert {len(c.terms) for c in mine} == {1, 2, 16}
            alone = {c.terms[0][0] for c in mine if len(c.terms) == 1}
            assert alone == {C.ONE, C.SCALAR, C.PLAIN}
            kinds = [{k for k, _ in c.terms} for c in mine]
            assert {C.ONE, C.SCALAR, C.PLAIN} in kinds                               # mixed
            consts = {k for c in mine for k, i in c.terms if i is None}
            assert consts == {C.SCALAR, C.PLAIN}                    # both constant terms
            assert any(len({i for _, i in c.terms}) < len(c.terms) and
                       None not in {i for _, i in c.terms} for c in mine)            # the same x twice
            if C.grid(1, n, bits)["per"] > 1:
                assert any(C.ends_partial(c) and c.batch > C.grid(1, n, bits)["per"] for c in mine)
            tens = [c for c in rows if (c.bits, c.n, c.op) == (bits, n, "tensor")]
            assert {c.pairs for c in tens} == {1, 3} and {c.square for c in tens} == {False, True}
        worst = [c for c in C.worst_cases() if c.bits == bits]
        assert {(c.n, c.terms[0][0], len(c.terms), c.comps) for c in worst} == \
            {(n, k, 16, 3) for n in (256, 4096) for k in (C.PLAIN, C.ONE)}
        inpl = [c for c in C.inplace_cases() if c.bits == bits]
        assert all(c.inplace == (0,) for c in inpl)
        assert {sum(i == 0 for _, i in c.terms) for c in inpl} == {1, 2}  # out == x_0 (== x_3)
    assert C.CHAIN_N == 256
    # no ONE constant term anywhere: it is NTTMUL_EINVAL
    assert not [c for c in C.all_cases() for k, i in c.terms if k == C.ONE and i is None]


def test_the_scale_cases_meet_the_rule_of_scale_cases(ctlin):
    import scale_cases as S
    assert (C.MIN_WAVES, C.WAVE) == (S.MIN_WAVES, S.WAVE)
    rows = C.scale_cases()
    seen = set()
    for case in rows:
        (key, waves), = C.launch_waves(case).items()
        assert key == C.kernel_name(case)
        assert waves >= S.MIN_WAVES, (case, waves)
        per, units, _ = C.units_per_block(case)[key]
        assert per > 1 and units % per, case                        # a partial last workgroup
        l = S.Launch(key, per, units, C.grid_rows(case)[key], 256, C.bpu(case), 1, 0)
        assert S.waves(l) == waves and S.wants_partial(l)
        # the smallest such batch: every smaller one is short of the rule or ends whole
        smaller = [case._replace(batch=b) for b in (case.batch - 1, case.batch - 2)]
        assert all(min(C.launch_waves(c).values()) < S.MIN_WAVES or not C.ends_partial(c)
                   for c in smaller)
        seen.add(key)
    # every kernel gets one row
    assert seen == {k for k in ctlin if k.startswith("k_ctlin_")} and len(rows) == 8


def test_every_exported_function_that_writes_caller_memory_has_a_footprint_row():
    EXEMPT = {"nttmul_ctlin_" + s for s in ("create", "destroy", "last_error", "get_info",
                                            "kernel_name")}      # no caller operand is written
    rows = C.footprint_cases()
    named = {f.entry for f in rows}
    exported = set(nttmul.ctlin_exported_symbols())
    writers = {s for s in exported if re.fullmatch(r"nttmul_ctlin_(combine|tensor)(_device)?", s)}
    assert len(writers) == 4 and named == writers
    assert EXEMPT == exported - writers
    for entry in writers:
        got = {(f.case.bits, f.case.n, f.case.batch) for f in rows if f.entry == entry}
        assert got == {(b, n, batch) for b in (32, 64) for n, batch in C.FP_SIZES}
    assert {f.case.inplace for f in rows if "combine" in f.entry} == {(), (0,)}   # the in-place call
    assert {f.case.square for f in rows if "tensor" in f.entry} == {False, True}
    assert all((f.host == "host") == (not f.entry.endswith("_device")) for f in rows)
    import guarded as G
    for f in rows:
        for per, units, words in C.units_per_block(f.case).values():
            assert C.fp_guard_words(f.case) >= max(per * words, G.guard_words(1))


def test_every_additional_kernel_is_launched_by_a_case_held_to_the_cpu_reference(level, ctlin):
    """The mirror reports the cases whose every output word a GPU test compares with the CPU
    reference (referenced_cases(): at every n, tests/full_ref.py); the cases full_ref.SUBSET holds
    on a part of their batch only do not count, and are at most one in ten.  Every kernel this
    library adds over its predecessor is launched by one of the rest."""
    import full_ref
    cases = C.referenced_cases()
    assert cases and all(c in C.all_cases() for c in cases[:8] + cases[-8:])
    whole = [c for c in cases if not full_ref.on_subset("ctlin", c)]
    assert 10 * (len(cases) - len(whole)) <= len(cases)
    held = {k for c in whole for k in C.kernels_of(c)}
    excused = {k for k in ctlin if any(re.fullmatch(pat, k) for pat, _ in
                                        getattr(C, "UNREACHABLE", ()))}
    extra = set(ctlin) - set(level)
    assert extra and sorted(extra - held - excused) == []
