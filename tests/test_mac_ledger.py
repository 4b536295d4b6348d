"""The kernel ledger of lib/libnttmul_mac.so, in the style of tests/test_kernel_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_mac.so = libnttmul.so's kernels, bit for bit, plus the k_mac kernels, and
every one of those is launched by a case of tests/mac_cases.py (whose mirror
test_gpu_mac.py anchors to nttmul_mac_kernel_name on the GPU)."""
import re

import pytest

import dispatch_cases as D
import mac_cases as M
import nttmul


@pytest.fixture(scope="module")
def base():
    return nttmul.kernel_hashes(nttmul.LIB_PATH)


@pytest.fixture(scope="module")
def mac():
    return nttmul.kernel_hashes(nttmul.MAC_LIB_PATH)


def _launched():
    out = {}
    for case in M.all_cases():
        for key in M.kernels_of(case):
            out.setdefault(key, case)
    return out


def _unreachable_reason(key):
    for pattern, reason in M.UNREACHABLE:
        if re.fullmatch(pattern, key):
            return reason
    return None


def test_common_kernels_are_the_product_librarys_bit_for_bit(base, mac):
    assert len(base) > 200
    assert sorted(set(base) - set(mac)) == []
    assert {k: mac[k] for k in base} == base


def test_the_additional_kernels_are_exactly_what_the_cases_launch(base, mac):
    extra = set(mac) - set(base)
    launched = _launched()
    new = {k for k in launched if k not in base}
    assert all(k.startswith("k_mac<") for k in extra), sorted(extra)
    missing = sorted(k for k in extra if k not in new and not _unreachable_reason(k))
    assert not missing, f"kernels no case launches and no rule excuses: {missing}"
    assert sorted(new - extra) == [], "the mirror names kernels the library does not hold"
    assert not [k for k in new if _unreachable_reason(k)]
    # what a case launches besides k_mac is a kernel of both libraries (the range check)
    assert all(k in base for k in launched if not k.startswith("k_mac<"))
    for pattern, reason in M.UNREACHABLE:
        assert any(re.fullmatch(pattern, k) for k in extra), f"rule matches no kernel: {pattern}"
        assert reason.strip() and "\n" not in reason
    assert len(extra) == 25     # 5 class-by-word combinations x 5 sizes


def test_mirror_restates_the_selection_rules():
    assert M.mac_kernel(4096, D.Q31, 32) == "k_mac<Arith32P,u32,u32,12>"   # not Arith32P3
    assert M.mac_kernel(256, D.Q32, 64) == "k_mac<Arith32W,u64,u64,8>"
    assert M.mac_kernel(1024, D.Q62, 64) == "k_mac<Arith64,u64,u64,10>"
    assert M.kernels_of(M.Case(512, D.Q20, 64, 3, True, 5, validate=True)) == \
        ["k_check_range<u64>", "k_check_range<u64>", "k_mac<Arith32P,u64,u64,9>"]
    # the shared form is a stride of the same kernel
    assert M.kernels_of(M.Case(512, D.Q20, 32, 3, True)) == M.kernels_of(M.Case(512, D.Q20, 32, 3, False))
    with pytest.raises(AssertionError):
        M.mac_kernel(1024, D.Q62, 32)
    with pytest.raises(AssertionError):
        M.mac_kernel(8192, D.Q31, 32)
    assert all((q - 1) % (2 * n) == 0 for n in M.MAC_N for q in M.moduli_at(n))
