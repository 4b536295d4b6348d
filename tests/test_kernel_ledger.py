"""The kernel ledger: which kernels of libnttmul.so the GPU suite's cases launch.

Runs without a GPU on the cross-compiled library.  It reads kernel symbol names only
(nttmul.kernel_hashes' keys), never machine code.  dispatch_cases.kernels_of restates the
library's selection rules; its product part is anchored to the library's own dispatch on the GPU
(tests/test_gpu_ledger.py), the transform, pointwise and utility part rests on reading
csrc/kernels.hip, since the library has no name query for those calls."""
import os
import re

import pytest

import dispatch_cases as D
import nttmul

pytestmark = pytest.mark.skipif(not os.path.exists(nttmul.LIB_PATH), reason="libnttmul.so not built")


@pytest.fixture(scope="module")
def library_kernels():
    return set(nttmul.kernel_hashes())


def _unreachable_reason(key):
    for pattern, reason in D.UNREACHABLE:
        if re.fullmatch(pattern, key):
            return reason
    return None


def _launched(cases):
    out = {}
    for case in cases:
        for key in D.kernels_of(case):
            out.setdefault(key, case)
    return out


def test_every_kernel_is_launched_by_a_case_or_listed_unreachable(library_kernels):
    """Each kernel of the library is produced by some case of tests/dispatch_cases.py or matched
    by an UNREACHABLE rule that says why no call can launch it; never both.  An instantiation
    added without a case fails here by name."""
    launched = _launched(D.all_cases())
    missing = sorted(k for k in library_kernels if k not in launched and not _unreachable_reason(k))
    assert not missing, f"{len(missing)} kernels no case launches and no rule excuses: {missing}"
    both = sorted(k for k in launched if _unreachable_reason(k))
    assert not both, f"listed unreachable but launched by a case: {both}"


def test_every_case_names_kernels_of_the_library(library_kernels):
    """What the mirror produces exists: a rule of kernels_of that drifts from the instantiations
    of csrc/kernels.hip names a kernel the library does not hold."""
    for key, case in _launched(D.all_cases()).items():
        assert key in library_kernels, (key, case)


def test_unreachable_rules_each_match_and_carry_a_reason(library_kernels):
    """No stale rule: each matches at least one kernel of the library, and says why.  The
    Arith64-on-u32 rule covers exactly the 43 instantiations the generic dispatch lambdas emit
    for the combination io_ok refuses."""
    counts = {}
    for key in library_kernels:
        for pattern, reason in D.UNREACHABLE:
            if re.fullmatch(pattern, key):
                counts[pattern] = counts.get(pattern, 0) + 1
                break
    for pattern, reason in D.UNREACHABLE:
        assert counts.get(pattern, 0) > 0, f"rule matches no kernel: {pattern}"
        assert reason.strip() and "\n" not in reason
    assert counts[D.UNREACHABLE[0][0]] == 43


def test_new_cases_reach_the_u64_kernels_on_32_bit_moduli(library_kernels):
    """The 32-bit arithmetic classes on u64 caller words: every such kernel of the library that
    is reachable at all is launched by a case of the new modules (dispatch_cases.new_cases)."""
    launched = _launched(D.new_cases())
    wanted = {k for k in library_kernels
              if re.match(r"k_\w+<Arith32\w*,", k) and "u64" in k and not _unreachable_reason(k)}
    assert len(wanted) > 60
    assert sorted(wanted - set(launched)) == []
    for util in ("k_bitrev<u64>", "k_bitrev_inplace<u64>", "k_check_range<u64>", "k_fill<u64>",
                 "k_server<Arith32P,9>", "k_server<Arith32P,10>"):
        assert util in launched, util


def test_mirror_restates_the_selection_rules():
    """Spot checks of kernels_of against names the library's dispatch is known to give
    (tests/test_gpu_parity.py pins these strings on the GPU)."""
    C = D.Case
    assert D.kernels_of(C("multiply", 4096, D.Q31, 32, 65536)) == ["k_rows<Arith32P3,u32,u32,12,0,false>"]
    assert D.kernels_of(C("multiply", 4096, D.Q31, 64, 0)) == ["k_rows<Arith32P3,u64,u64,12,0,false>"]
    assert D.kernels_of(C("multiply", 1024, D.Q31, 32, 4096)) == ["k_rows<Arith32P,u32,u32,10,0,true>"]
    assert D.kernels_of(C("multiply", 1024, D.Q31, 32, 4096, prio_ok=0)) == \
        ["k_rows<Arith32P,u32,u32,10,0,false>"]
    assert D.kernels_of(C("multiply", 65536, D.Q62, 64, 1024)) == \
        ["k_cols8<Arith64,u64,u64,0,2>", "k_rows<Arith64,u64,u64,8,8,false>", "k_cols8<Arith64,u64,u64,1,1>"]
    assert D.kernels_of(C("multiply", 65536, D.Q32, 64, 3)) == \
        ["k_cols_fwd<Arith32W,u64,4,2>", "k_rows<Arith32W,u32,u32,12,4,false>", "k_cols_inv<Arith32W,u64,4>"]
    assert D.kernels_of(C("transform", 8192, D.Q31, 64, 2, mode=2)) == \
        ["k_bitrev<u64>", "k_cols_fwd<Arith32P,u64,1,1>", "k_xform<Arith32P,u32,u64,12,1,0>",
         "k_bitrev_inplace<u64>"]
    assert D.kernels_of(C("transform", 8192, D.Q31, 64, 2, mode=3, validate=True)) == \
        ["k_check_range<u64>", "k_xform<Arith32P,u64,u32,12,1,1>", "k_cols_inv<Arith32P,u64,1>"]
    assert D.kernels_of(C("pointwise", 256, D.Q20, 64, 1)) == ["k_pointwise<Arith32,u64>"]
    assert D.kernels_of(C("multiply", 512, D.Q31, 32, 2, path="server")) == ["k_server<Arith32P,9>"]
    assert D.xform_upg(4096, D.Q32) == 2 and D.xform_upg(8192, D.Q32) == 1 and D.xform_upg(256, D.Q62) == 1
    # p3_fold_ok over the whole Plantard range the library serves at n = 4096
    assert all(D.p3_fold_ok(q) for q in (D.Q0, D.Q20, D.Q30, D.Q31, D.Q31LO, D.Q31HI, (1 << 31) - 1))
    assert not D.p3_fold_ok(1 << 31)
    with pytest.raises(AssertionError):
        D.kernels_of(C("multiply", 1024, D.Q62, 32, 1))
