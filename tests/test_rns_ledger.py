"""The kernel ledger of lib/libnttmul_rns.so, in the style of tests/test_mac_ledger.py.

Runs without a GPU on the cross-compiled libraries and reads kernel symbol names and per-kernel
hashes only.  libnttmul_rns.so = libnttmul_mac.so's kernels, bit for bit, plus the k_rns_* kernels,
and every one of those is launched by a case of tests/rns_cases.py (whose mirror test_gpu_rns.py
anchors to nttmul_rns_kernel_name on the GPU)."""
import re

import pytest

import dispatch_cases as D
import nttmul
import rns_cases as R


@pytest.fixture(scope="module")
def mac():
    return nttmul.kernel_hashes(nttmul.MAC_LIB_PATH)


@pytest.fixture(scope="module")
def rns():
    return nttmul.kernel_hashes(nttmul.RNS_LIB_PATH)


def _launched():
    out = {}
    for case in R.all_cases():
        for key in R.kernels_of(case):
            out.setdefault(key, case)
    return out


def _unreachable_reason(key):
    for pattern, reason in R.UNREACHABLE:
        if re.fullmatch(pattern, key):
            return reason
    return None


def test_common_kernels_are_the_mac_librarys_bit_for_bit(mac, rns):
    assert len(mac) > 225
    assert sorted(set(mac) - set(rns)) == []
    assert {k: rns[k] for k in mac} == mac
    base = nttmul.kernel_hashes(nttmul.LIB_PATH)
    assert {k: rns[k] for k in base} == base


def test_the_additional_kernels_are_exactly_what_the_cases_launch(mac, rns):
    extra = set(rns) - set(mac)
    launched = _launched()
    assert all(k.startswith("k_rns_") for k in extra), sorted(extra)
    assert all(k.startswith("k_rns_") and k not in mac for k in launched), sorted(launched)
    missing = sorted(k for k in extra if k not in launched and not _unreachable_reason(k))
    assert not missing, f"kernels no case launches and no rule excuses: {missing}"
    assert sorted(set(launched) - extra) == [], "the mirror names kernels the library does not hold"
    assert not [k for k in launched if _unreachable_reason(k)]
    for pattern, reason in R.UNREACHABLE:
        assert any(re.fullmatch(pattern, k) for k in extra), f"rule matches no kernel: {pattern}"
        assert reason.strip() and "\n" not in reason
    # per class (2) and n (5): one product, two transforms, one mac; one range check per word
    assert len(extra) == 2 * 5 * 4 + 2
    # rows at n = 4096 on 32-bit words exist as Arith32P3 only
    assert "k_rns_rows<Arith32P3,u32,12>" in extra and "k_rns_rows<Arith32P,u32,12>" not in extra
    assert not [k for k in extra if "Arith32W" in k]


def test_mirror_restates_the_selection_rules():
    assert R.rns_kernel("multiply", 4096, R.BASIS32) == "k_rns_rows<Arith32P3,u32,12>"
    assert R.rns_kernel("multiply", 2048, R.BASIS32_5) == "k_rns_rows<Arith32P,u32,11>"
    assert R.rns_kernel("multiply", 4096, R.BASIS64) == "k_rns_rows<Arith64,u64,12>"
    assert R.rns_kernel("forward", 4096, R.BASIS32) == "k_rns_xform<Arith32P,u32,12,0>"   # not P3
    assert R.rns_kernel("inverse", 256, R.BASIS64[:1]) == "k_rns_xform<Arith64,u64,8,1>"
    assert R.rns_kernel("mac", 4096, R.BASIS32) == "k_rns_mac<Arith32P,u32,12>"
    assert R.kernels_of(R.Case("mac", 512, R.BASIS64, 3, 2, True, True)) == \
        ["k_rns_check_range<u64>"] * 2 + ["k_rns_mac<Arith64,u64,9>"]
    assert R.kernels_of(R.Case("forward", 512, R.BASIS32, 3, 1, False, True)) == \
        ["k_rns_check_range<u32>", "k_rns_xform<Arith32P,u32,9,0>"]
    # the shared form is a stride of the same kernel
    assert R.kernels_of(R.Case("mac", 512, R.BASIS32, 5, 3, True)) == \
        R.kernels_of(R.Case("mac", 512, R.BASIS32, 5, 3, False))
    with pytest.raises(AssertionError):
        R.rns_kernel("multiply", 1024, (D.Q31, D.Q62))          # mixed classes
    with pytest.raises(AssertionError):
        R.rns_kernel("multiply", 1024, (D.Q31, D.Q32))          # [2^31, 2^32)
    with pytest.raises(AssertionError):
        R.rns_kernel("multiply", 1024, (D.Q31, D.Q31))          # two equal primes
    with pytest.raises(AssertionError):
        R.rns_kernel("mac", 8192, R.BASIS32)


def test_the_bases_serve_every_n():
    """Each modulus is prime with 2 * 4096 | q - 1, the bases hold distinct primes of one word
    class, and the validate cases' bad value is in range for the neighbour they name."""
    for basis in (R.BASIS32_5, R.BASIS64):
        assert len(set(basis)) == len(basis)
        for q in basis:
            assert nttmul.is_prime(q) and (q - 1) % (2 * 4096) == 0, q
    assert R.word_bits(R.BASIS32_5) == 32 and R.word_bits(R.BASIS64) == 64
    for n, moduli, limb, other in R.VALIDATE:
        assert moduli[limb] < moduli[other]
